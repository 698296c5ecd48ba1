"""Torch-CPU restatement of the biases in front of a row draw -- what ``dh_beam_bias_logits`` and
``generate_batch(..., sequence_bias=S)`` must compute, bit for bit -- and the kernel test cases.

For one row with history ``h[0 .. s)`` (token ids, ``s = pos``) and fp32 logits ``x[0 .. V)``, and a list of ``(phrase, bias)`` pairs:

1. a phrase ``w`` of ``l`` ids fires iff ``l - 1 <= s`` and ``h[s-l+1 .. s) == w[0 .. l-1)`` (``l == 1``: at every position);
2. a fired phrase adds ``float32(bias)`` to ``x[w[l-1]]``; several phrases that fire on one column are added one after the other IN
   LIST ORDER, each addition its own round-to-nearest fp32 add: ``x = ((x + b1) + b2) ...``; ``-inf`` stays ``-inf``.  A last id
   outside ``[0, V)`` is never a column; the other ids are compared as they are;
3. group maxima: every group of ``group_cols`` columns that holds a column rule 2 STORED to (whether or not its value changed)
   becomes the maximum of the edited row over the group's real columns ``< V``; other groups keep their word.

``brute_*`` are the slow, literal versions (every phrase at every offset of the history, numpy fp32 scalars) the restatement is
checked against (tests/test_sequence_bias_cpu.py).  ``sort_pairs`` / ``flatten_sorted`` restate the host compiler's layout."""
import numpy as np
import torch

NEG_INF = float("-inf")
EOS, UNK = 3, 1
MAX_BAD_LEN = 32


def brute_fired(history, pairs):
    """Literal scan: every phrase at EVERY offset ``j`` of ``history`` (a list of ints); the phrase's first ``l - 1`` ids sitting at
    ``j`` fire iff they end exactly where the history ends.  Returns the list indices of the fired pairs, in list order."""
    s = len(history)
    out = []
    for i, (w, _) in enumerate(pairs):
        l = len(w)
        for j in range(s + 1):
            if j + (l - 1) == s and list(history[j:j + l - 1]) == list(w[:l - 1]):
                out.append(i)
    return out


def brute_bias_row(x, history, pairs, group_max=None, group_cols=64):
    """The three rules by Python loops on a 1-D fp32 tensor ``x`` (copied), the additions on numpy fp32 scalars.  Returns ``(x,
    group_max, stored columns sorted)``."""
    y = x.clone().numpy()
    v = y.shape[0]
    stored = set()
    with np.errstate(all="ignore"):
        for i in brute_fired(history, pairs):
            w, b = pairs[i]
            t = int(w[-1])
            if 0 <= t < v:
                y[t] = np.float32(y[t]) + np.float32(b)
                stored.add(t)
    y = torch.from_numpy(y)
    if group_max is not None:
        group_max = group_max.clone()
        for g in sorted({t // group_cols for t in stored}):
            group_max[g] = y[g * group_cols:min(v, (g + 1) * group_cols)].max()
    return y, group_max, sorted(stored)


def fires(history, pos, w):
    """bool ``[rows]``: phrase ``w`` matches the rows' history tails at ``pos`` (whatever its last id is)."""
    l = len(w)
    if l - 1 > pos:
        return torch.zeros(history.shape[0], dtype=torch.bool)
    if l == 1:
        return torch.ones(history.shape[0], dtype=torch.bool)
    return (history[:, pos - l + 1:pos].to(torch.int64) == torch.tensor(list(w[:l - 1]), dtype=torch.int64)[None, :]).all(1)


def bias_logits(logits, history, pos, pairs, group_max=None, group_cols=64, active=None):
    """The restatement.  ``logits [rows, V]`` fp32, ``history [rows, >= pos]`` integer, ``pos`` the history length of every row,
    ``pairs`` a sequence of ``(phrase, bias)``, ``group_max [rows, G]`` fp32 or None, ``active`` bool ``[rows]`` or None (all): rows
    that are not active keep every word.  Nothing is modified in place; returns ``(logits, group_max, stored bool [rows, V])``."""
    rows, v = logits.shape
    out = logits.clone().float()
    s = int(pos)
    act = torch.ones(rows, dtype=torch.bool) if active is None else active.to(torch.bool)
    stored = torch.zeros((rows, v), dtype=torch.bool)
    for w, b in pairs:                                     # list order: one fp32 add per fired pair and row
        t = int(w[-1])
        if not 0 <= t < v:
            continue
        hit = act & fires(history, s, w)
        col = out[:, t]
        out[:, t] = torch.where(hit, col + torch.tensor(float(b), dtype=torch.float64).to(torch.float32), col)
        stored[:, t] |= hit
    gm = None
    if group_max is not None:
        gm = group_max.clone()
        g_all = (v + group_cols - 1) // group_cols
        pad = torch.full((rows, g_all * group_cols), NEG_INF)
        pad[:, :v] = out
        true_max = pad.view(rows, g_all, group_cols).max(-1).values
        spad = torch.zeros((rows, g_all * group_cols), dtype=torch.bool)
        spad[:, :v] = stored
        touched = spad.view(rows, g_all, group_cols).any(-1)
        gm[:, :g_all] = torch.where(touched, true_max, gm[:, :g_all])
    return out, gm, stored


def bits(x):
    """fp32 tensor -> its int32 words: equality of these is equality bit for bit (``-0.0`` is not ``0.0``, a NaN is its payload)."""
    return x.contiguous().view(torch.int32)


# ---- the host compiler's layout ---------------------------------------------------------------------------------------------------
def sort_pairs(pairs):
    """``(order, run_off)``: the list indices stably sorted by the phrases' last ids (equal last ids keep their list order), and the
    starts of the runs of equal last ids in that order, with ``len(pairs)`` as the last entry."""
    order = [i for _, i in sorted((int(w[-1]), i) for i, (w, _) in enumerate(pairs))]      # (the index breaks ties: list order)
    run_off = [0]
    for k in range(1, len(order)):
        if pairs[order[k]][0][-1] != pairs[order[k - 1]][0][-1]:
            run_off.append(k)
    return order, run_off + [len(order)]


def flatten_sorted(pairs):
    """``(words int32, offsets int32 [n + 1], bias fp32 [n], run_off int32 [n_runs + 1])``: the layout ``dh_beam_bias_logits`` reads."""
    order, run_off = sort_pairs(pairs)
    offs = [0]
    for i in order:
        offs.append(offs[-1] + len(pairs[i][0]))
    return (torch.tensor([t for i in order for t in pairs[i][0]], dtype=torch.int32), torch.tensor(offs, dtype=torch.int32),
            torch.tensor([float(pairs[i][1]) for i in order], dtype=torch.float64).to(torch.float32), torch.tensor(run_off, dtype=torch.int32))


# ---- the kernel test cases ----------------------------------------------------------------------------------------------------------
N_PHRASES = 300
CASE_VS = (130, 1000, 4133)
CASE_POS = (0, 1, 5, 40)
ORDER_BIASES = (1e-3, 7.25, -3.1)


def make_case(v, pos, first_step=False, seed=0):
    """One kernel case: ``dict(logits [rows, v], table [rows * mult, w] int32, mult, pos, rows, rpi, pairs, v, named)``.

    12 rows (4 images x beam 3, ``mult = 1``), or the dense first step: 4 rows whose histories are rows 0, 3, 6, 9 of the table
    (``mult = 3``; the rows between hold other tokens).  Histories are random over ``[0, v - 2)`` -- ids ``v - 2`` and ``v - 1`` never
    occur in one, so a phrase with ``v - 2`` in its prefix fires in no row -- with tails planted as below (``P`` = ``pos``; a tail
    that does not fit is not planted, which makes its phrase one that is longer than ``pos + 1``).  The logits are random, times 3,
    with column 69 = 11.0 the row maximum, column 70 = 9.0 its group's second value, column 4 = ``-inf`` and column 10 = -2.3:

    ==========================================  ===================================================================
    pair                                        fires
    ==========================================  ===================================================================
    ``O1 = ([5, 10], +1e-3)``                   rows 0 and 5 (``h[P-1] = 5``)
    ``O2 = ([10], +7.25)``, ``O3 = ([10], -3.1)``  everywhere: with O1 three pairs on column 10 whose order changes the bits
    ``D = ([6, 12], +0.5)`` twice               row 2 (``h[P-1] = 6``): the same phrase twice, each one counts
    ``([5, v - 1], +2.0)``                      rows 0 and 5: column ``V - 1``, the last (partial) group
    ``([69], -9.0)``                            everywhere: the row maximum falls to 2.0, below column 70's 9.0
    ``([8], +40.0)``                            everywhere: a new maximum of group 0 (and of the row)
    ``([6, 7], +50.0)``                         row 2: a new maximum in that row only
    ``([4], +5.0)``                             everywhere, on a ``-inf`` column: it stays ``-inf`` and is stored
    ``([5, v + 3], +1.0)``                      rows 0 and 5, but its last id is no column: nothing is stored
    ``B = ([11, 12, 13, 14, 20], -2.5)``        rows 1 and 7 (``P >= 4``); row 3 holds ``11 12 99 14``: the last prefix id matches,
                                                the one before does not
    ``C`` (32 ids, last 21, ``+3.0``)           row 4 at ``P = 40`` (``P >= 31``)
    ``([v - 2, 23], +1.0)``, ``([v - 2, 9, 24], +1.0)``  never
    filler: random 2- and 3-id phrases          by chance; random biases in ``[-4, 4)``
    ==========================================  ===================================================================

    (Row numbers are those of the 12-row case; the first-step case plants them modulo 4.)  300 pairs, the planted ones LAST, at list
    indices >= 256.  The filler's last ids: for ``v > 130`` all distinct, ``128 + 3 k`` -- so the sorted list has more than 256 runs,
    the kernel's 256-thread stride loop over the runs takes a second trip, and the runs of column ``V - 1`` and of the id ``v + 3``
    are in it --; for ``v = 130`` all 128: ONE run of some 280 phrases on one column, walked in list order by one thread."""
    g = torch.Generator().manual_seed(7000 * v + 10 * pos + int(first_step) + seed)
    rows, mult = (4, 3) if first_step else (12, 1)
    width = max(pos, 1) + 2
    table = torch.randint(0, v - 2, (rows * mult, width), generator=g, dtype=torch.int32)
    used = table[::mult].clone()
    O1, O2, O3, D, B = [5, 10], [10], [10], [6, 12], [11, 12, 13, 14, 20]
    C = [(3 * k + 17) % (v - 2) for k in range(31)] + [21]
    last = lambda r: r % rows                                         # (the first-step case has 4 rows: plant modulo)
    if pos >= 1:
        used[:, pos - 1] = 30                                         # no accidental 5 / 6 in front of the draw
        for r in (0, 5):
            used[last(r), pos - 1] = 5
        used[last(2), pos - 1] = 6
    if pos >= 4:
        for r in (1, 7):
            used[last(r), pos - 4:pos] = torch.tensor(B[:4], dtype=torch.int32)
        used[3, pos - 4:pos] = torch.tensor([11, 12, 99 % (v - 2), 14], dtype=torch.int32)
    if pos >= 31 and not first_step:
        used[4, pos - 31:pos] = torch.tensor(C[:31], dtype=torch.int32)
    table[::mult] = used
    logits = (torch.randn(rows, v, generator=g) * 3).clamp(max=8.5)      # (below the two planted values of group 1)
    logits[:, 69], logits[:, 70], logits[:, 4], logits[:, 10], logits[:, 0] = 11.0, 9.0, NEG_INF, -2.3, 0.0
    key = [(O1, ORDER_BIASES[0]), (O2, ORDER_BIASES[1]), (O3, ORDER_BIASES[2]), (D, 0.5), ([5, v - 1], 2.0), ([69], -9.0), ([8], 40.0),
           ([6, 7], 50.0), ([4], 5.0), ([5, v + 3], 1.0), (B, -2.5), (C, 3.0), ([v - 2, 23], 1.0), ([v - 2, 9, 24], 1.0), (D, 0.5)]
    pairs = []
    while len(pairs) + len(key) < N_PHRASES:
        k = len(pairs)
        l = 2 + int(torch.randint(0, 2, (1,), generator=g))
        b = float(torch.rand(1, generator=g)) * 8.0 - 4.0
        pairs.append((torch.randint(0, v - 2, (l - 1,), generator=g).tolist() + [128 + 3 * k if v > 130 else 128], b))
    pairs += [(list(w), b) for w, b in key]
    assert len(pairs) == N_PHRASES
    return dict(v=v, pos=pos, rows=rows, mult=mult, rpi=1, logits=logits, table=table, pairs=pairs,
                named=dict(O1=O1, O2=O2, O3=O3, D=D, B=B, C=C, never=[[v - 2, 23], [v - 2, 9, 24]]))


def kernel_cases(v):
    """Every case of one ``V``: 12 rows at each ``pos`` of ``CASE_POS``, and the dense first step (4 rows, ``tok_row_mult = 3``) at
    ``pos = 5``."""
    return [make_case(v, pos) for pos in CASE_POS] + [make_case(v, 5, first_step=True)]
