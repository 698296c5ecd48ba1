"""Torch-CPU restatement of the history-dependent logit edits in front of a row draw -- what ``dh_beam_history_logits`` and
``generate_batch(..., no_repeat_ngram_size=n, repetition_penalty=p)`` must compute, bit for bit.

For one row with history ``h[0 .. L)`` (token ids; ids outside ``[0, V)`` are never a column, but take part in the n-gram
comparison as they are) and fp32 logits ``x[0 .. V)``:

1. ``penalty != 1``: for every DISTINCT token ``t`` of ``h``: ``x[t] = x[t] * penalty if x[t] < 0 else x[t] / penalty`` (fp32,
   IEEE division; once per token however often it occurs; ``-inf`` stays ``-inf``);
2. ``ngram = n >= 1`` and ``L >= n``: with ``p = h[L-n+1 .. L)`` (the last ``n - 1`` tokens), for every ``j`` in ``[0, L - n]``
   with ``h[j .. j+n-1) == p``: ``x[h[j+n-1]] = -inf`` (``n == 1``: every token of ``h``).  After step 1, so a ban wins;
3. group maxima: for every group of ``group_cols`` columns that holds a column step 1 or 2 STORED to (step 1 stores to every
   in-range token of the history, whether the value moves or not), the maximum over the group's real columns ``< V`` of the
   edited row; other groups keep their word.

``brute_*`` are the slow, literal versions the vectorised restatement is checked against (tests/test_repeat_cpu.py)."""
import torch

NEG_INF = float("-inf")


def banned_tokens(history, n):
    """Brute-force Python scan: the tokens that would complete an n-gram ``history`` (a list of ints) already holds."""
    L = len(history)
    if n < 1 or L < n:
        return set()
    tail = history[L - n + 1:]
    return {history[j + n - 1] for j in range(L - n + 1) if history[j:j + n - 1] == tail}


def brute_edit_row(x, history, n, penalty, group_max=None, group_cols=64):
    """The three rules, one Python loop each, on a 1-D fp32 tensor ``x`` (copied) and a list of ints ``history``; ``group_max``: the
    row's 1-D group words (copied) or None.  Returns ``(x, group_max, stored columns as a sorted list)``."""
    x = x.clone()
    v = x.shape[0]
    pen = torch.tensor(penalty, dtype=torch.float32)
    stored = set()
    if penalty != 1.0:
        for t in sorted({t for t in history if 0 <= t < v}):
            x[t] = x[t] * pen if bool(x[t] < 0) else x[t] / pen
            stored.add(t)
    for t in banned_tokens(history, n):
        if 0 <= t < v:
            x[t] = NEG_INF
            stored.add(t)
    if group_max is not None:
        group_max = group_max.clone()
        for g in sorted({t // group_cols for t in stored}):
            group_max[g] = x[g * group_cols:min(v, (g + 1) * group_cols)].max()
    return x, group_max, sorted(stored)


def edit_logits(logits, history, length, n=0, penalty=1.0, group_max=None, group_cols=64, active=None):
    """Vectorised restatement.  ``logits [rows, V]`` fp32, ``history [rows, >= length]`` integer, ``length`` the history length
    ``L`` of every row, ``group_max [rows, G]`` fp32 or None, ``active`` bool ``[rows]`` or None (all): rows that are not active
    keep every word.  Nothing is modified in place; returns ``(logits, group_max, stored bool [rows, V])``."""
    rows, v = logits.shape
    out = logits.clone().float()
    L = int(length)
    h = history[:, :L].to(torch.int64)
    act = torch.ones(rows, dtype=torch.bool) if active is None else active.to(torch.bool)
    stored = torch.zeros((rows, v), dtype=torch.bool)
    ok = (h >= 0) & (h < v) & act[:, None]
    hc = h.clamp(0, v - 1)
    if penalty != 1.0 and L > 0:
        # (a count, not scatter_ of the flags: an out-of-range position clamped onto a column must not clear another position's True)
        seen = torch.zeros((rows, v), dtype=torch.int32).scatter_add_(1, hc, ok.to(torch.int32)) > 0
        pen = torch.tensor(penalty, dtype=torch.float32)
        damped = torch.where(out < 0, out * pen, out / pen)
        out = torch.where(seen, damped, out)
        stored |= seen
    if n >= 1 and L >= n:
        m = n - 1
        cnt = L - n + 1                                            # candidate starts j = 0 .. L - n
        eq = torch.ones((rows, cnt), dtype=torch.bool)
        for k in range(m):
            eq &= h[:, k:k + cnt] == h[:, L - m + k:L - m + k + 1]
        tgt, tok = hc[:, m:m + cnt], ok[:, m:m + cnt]
        ban = torch.zeros((rows, v), dtype=torch.int32).scatter_add_(1, tgt, (eq & tok).to(torch.int32)) > 0
        out = torch.where(ban, torch.full_like(out, NEG_INF), out)
        stored |= ban
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


def repeated_ngrams(tokens, n):
    """The n-grams that occur more than once in ``tokens`` (a list of ints)."""
    seen, twice = set(), set()
    for j in range(len(tokens) - n + 1):
        g = tuple(tokens[j:j + n])
        (twice if g in seen else seen).add(g)
    return twice
