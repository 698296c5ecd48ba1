"""Torch-CPU restatement of the bans in front of a row draw -- what ``dh_beam_constrain_logits`` and
``generate_batch(..., min_len=m, bad_words_ids=W)`` must compute, bit for bit -- and the kernel test cases.

For one row with history ``h[0 .. s)`` (token ids, ``s = pos``) and fp32 logits ``x[0 .. V)``:

1. ``s < min_len`` and ``0 <= eos < V``: ``x[eos] = -inf``;
2. for every phrase ``w`` of ``l`` ids: if ``l - 1 <= s`` and ``h[s-l+1 .. s) == w[0 .. l-1)`` then ``x[w[l-1]] = -inf`` (``l == 1``:
   at every position).  A last id outside ``[0, V)`` is never a column; the other ids are compared as they are;
3. group maxima: every group of ``group_cols`` columns that holds a column rule 1 or 2 STORED to becomes the maximum of the edited
   row over the group's real columns ``< V`` (``-inf`` if all are); other groups keep their word.

``brute_*`` are the slow, literal versions (every phrase at every offset of the history) the restatement is checked against
(tests/test_constraints_cpu.py)."""
import torch

NEG_INF = float("-inf")
EOS, UNK = 3, 1
MAX_BAD_LEN = 32


def brute_banned(history, phrases, min_len=0, eos=-1):
    """Literal scan: every phrase at EVERY offset ``j`` of ``history`` (a list of ints); the phrase's first ``l - 1`` ids sitting at
    ``j`` ban its last id iff they end exactly where the history ends.  Returns the set of banned ids (not yet guarded to
    ``[0, V)``)."""
    s = len(history)
    out = set()
    if s < min_len and eos >= 0:
        out.add(eos)
    for w in phrases:
        l = len(w)
        for j in range(s + 1):
            if j + (l - 1) == s and list(history[j:j + l - 1]) == list(w[:l - 1]):
                out.add(w[l - 1])
    return out


def brute_constrain_row(x, history, phrases, min_len=0, eos=-1, group_max=None, group_cols=64):
    """The three rules by Python loops on a 1-D fp32 tensor ``x`` (copied).  Returns ``(x, group_max, stored columns sorted)``."""
    x = x.clone()
    v = x.shape[0]
    stored = sorted(t for t in brute_banned(history, phrases, min_len, eos) if 0 <= t < v)
    for t in stored:
        x[t] = NEG_INF
    if group_max is not None:
        group_max = group_max.clone()
        for g in sorted({t // group_cols for t in stored}):
            group_max[g] = x[g * group_cols:min(v, (g + 1) * group_cols)].max()
    return x, group_max, stored


def constrain_logits(logits, history, pos, phrases, min_len=0, eos=-1, group_max=None, group_cols=64, active=None):
    """The restatement.  ``logits [rows, V]`` fp32, ``history [rows, >= pos]`` integer, ``pos`` the history length of every row,
    ``phrases`` a sequence of sequences of ints, ``group_max [rows, G]`` fp32 or None, ``active`` bool ``[rows]`` or None (all):
    rows that are not active keep every word.  Nothing is modified in place; returns ``(logits, group_max, stored bool [rows, V])``."""
    rows, v = logits.shape
    out = logits.clone().float()
    s = int(pos)
    h = history[:, :s].to(torch.int64)
    act = torch.ones(rows, dtype=torch.bool) if active is None else active.to(torch.bool)
    stored = torch.zeros((rows, v), dtype=torch.bool)
    if s < min_len and 0 <= eos < v:
        stored[:, eos] |= act
    for w in phrases:
        l, t = len(w), int(w[-1])
        if l - 1 > s or not 0 <= t < v:
            continue
        hit = act if l == 1 else act & (h[:, s - l + 1:s] == torch.tensor(list(w[:l - 1]), dtype=torch.int64)[None, :]).all(1)
        stored[:, t] |= hit
    out = torch.where(stored, torch.full_like(out, NEG_INF), out)
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


def fires(history, pos, w):
    """bool ``[rows]``: phrase ``w`` matches the rows' history tails at ``pos`` (whatever its last id is)."""
    l = len(w)
    if l - 1 > pos:
        return torch.zeros(history.shape[0], dtype=torch.bool)
    if l == 1:
        return torch.ones(history.shape[0], dtype=torch.bool)
    return (history[:, pos - l + 1:pos].to(torch.int64) == torch.tensor(list(w[:l - 1]), dtype=torch.int64)[None, :]).all(1)


# ---- host scans of finished captions ------------------------------------------------------------------------------------------------
def banned_phrase_in(tokens, phrases, start=0):
    """The first ``(phrase, end index)`` of ``tokens`` (a list of ints) that holds a phrase of ``phrases`` as a contiguous run ENDING at an
    index ``>= start`` (``start``: the first generated column; a prompt may hold what it likes), or None."""
    n = len(tokens)
    for w in phrases:
        l = len(w)
        for e in range(max(start, l - 1), n):
            if list(tokens[e - l + 1:e + 1]) == list(w):
                return tuple(w), e
    return None


def eos_below(tokens, min_len, eos, start=0):
    """True iff ``tokens`` holds ``eos`` at a generated index ``start <= s < min_len``."""
    return any(t == eos for t in tokens[start:min_len])


# ---- the kernel test cases ----------------------------------------------------------------------------------------------------------
N_PHRASES = 300
CASE_VS = (130, 1000, 4133)
CASE_POS = (0, 1, 5, 40)


def make_case(v, pos, first_step=False, seed=0):
    """One kernel case: ``dict(logits [rows, v], table [rows * mult, w] int32, mult, pos, rows, rpi, phrases, eos, v)``.

    12 rows (4 images x beam 3, ``mult = 1``), or the dense first step: 4 rows whose histories are rows 0, 3, 6, 9 of the table
    (``mult = 3``; the rows between hold other tokens).  Histories are random over ``[0, v - 2)`` -- ids ``v - 2`` and ``v - 1`` never
    occur in one, so a phrase with ``v - 2`` in its prefix fires in no row -- with tails planted as below (``P`` = ``pos``; a
    tail that does not fit is not planted, which makes its phrase one that is longer than ``pos + 1``):

    ====================================  ===================================================================
    phrase                                fires
    ====================================  ===================================================================
    ``[0]``, ``[UNK]``, ``[64] .. [127]``    everywhere (all 64 real columns of group 1: the group's maximum is ``-inf``)
    ``A = [5, 10]`` (twice: a duplicate)   rows 0 and 5 (``h[P-1] = 5``)
    ``A2 = [6, 10]`` (same last id)        row 2 (``h[P-1] = 6``)
    ``[5, v - 1]``                         rows 0 and 5: column ``V - 1``, the last (partial) group
    ``[5, v + 3]``                         rows 0 and 5, but its last id is no column: nothing is stored
    ``B = [11, 12, 13, 14, 20]``           rows 1 and 7 (``P >= 4``); row 3 holds ``11 12 99 14``: the last prefix id matches, the
                                          one before does not
    ``C`` (32 ids, last 21)               row 4 at ``P = 40`` (``P >= 31``)
    ``[v - 2, 23]``, ``[v - 2, 9, 24]``     never
    filler: random 2- and 3-id phrases    by chance
    ====================================  ===================================================================

    (Row numbers are those of the 12-row case; the first-step case plants them modulo 4.)  300 phrases; group 1's singles come first and the planted phrases LAST, at indices >= 256: the second trip of the kernel's
    256-thread stride loop.  The logits make column 69 the row maximum and hold ``-inf``, ``0.0`` and a finite ``<eos>``."""
    g = torch.Generator().manual_seed(1000 * v + 10 * pos + int(first_step) + seed)
    rows, mult = (4, 3) if first_step else (12, 1)
    width = max(pos, 1) + 2
    table = torch.randint(0, v - 2, (rows * mult, width), generator=g, dtype=torch.int32)
    used = table[::mult].clone()
    A, A2, B = [5, 10], [6, 10], [11, 12, 13, 14, 20]
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
    logits = torch.randn(rows, v, generator=g) * 3
    logits[:, 69] = 11.0
    logits[:, 0] = 0.0
    logits[:, 4] = NEG_INF
    logits[:, EOS] = 2.5
    phrases = [[64 + c] for c in range(64)] + [[0], [UNK], list(A)]
    key = [list(A2), [5, v - 1], [5, v + 3], list(B), list(C), [v - 2, 23], [v - 2, 9, 24], list(A)]
    while len(phrases) + len(key) < N_PHRASES:
        l = 2 + int(torch.randint(0, 2, (1,), generator=g))
        phrases.append(torch.randint(0, v - 2, (l,), generator=g).tolist()[:l - 1] + [int(torch.randint(128, v, (1,), generator=g)) if v > 130 else 128])
    phrases += key
    assert len(phrases) == N_PHRASES
    return dict(v=v, pos=pos, rows=rows, mult=mult, rpi=1, logits=logits, table=table, phrases=phrases, eos=EOS,
                named=dict(A=A, A2=A2, B=B, C=C, never=[[v - 2, 23], [v - 2, 9, 24]]))


def kernel_cases(v):
    """Every case of one ``V``: 12 rows at each ``pos`` of ``CASE_POS``, and the dense first step (4 rows, ``tok_row_mult = 3``) at
    ``pos = 5``.  Each is run with ``min_len`` above ``pos`` and at-or-below it (``min_lens``)."""
    cases = [make_case(v, pos) for pos in CASE_POS] + [make_case(v, 5, first_step=True)]
    for c in cases:
        c["min_lens"] = (c["pos"] + 2, c["pos"], 0)
    return cases


def flatten(phrases):
    """``(words int32 [sum of lengths], offsets int32 [n + 1])``: the layout ``dh_beam_constrain_logits`` reads."""
    offs = [0]
    for w in phrases:
        offs.append(offs[-1] + len(w))
    return torch.tensor([t for w in phrases for t in w], dtype=torch.int32), torch.tensor(offs, dtype=torch.int32)
