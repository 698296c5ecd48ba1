"""Restatement of the sampled beam step (``csrc/beam.hip``): which row kernel a call runs, the Philox noise of ``common.h``, the row
draw, the sampled candidate select and the final draw -- numpy / torch-CPU, fp64 wherever arithmetic happens.  The yardstick of
``tests/test_row_draw_routes_gpu.py``; ``tests/test_row_draw_ref_cpu.py`` holds it against the oracle and golden G4.

Picks are compared for equality, so every function that ranks also returns a *margin*: the smallest relative gap between consecutive
``q = p / noise`` among the ``beam + 1`` largest.  The fp32 kernels evaluate ``q`` to a few 1e-6 relative (one rounding of ``x / T``,
two-ulp ``expf`` / ``logf``, a six-level sum), so a test admits only inputs whose margin is >= ``MARGIN`` -- a condition on the
INPUTS, met on the CPU before a GPU is asked anything."""
import numpy as np
import torch

from beam_search_ref import candidates
from nucleus_ref import nucleus_keep

ERR_ALL_FILTERED, ERR_OVERFLOW, ERR_TOO_FEW, ERR_NONFINITE = 1, 2, 4, 8
MAX_SURVIVORS, MAX_BEAMS = 1024, 64          # DH_BEAM_MAX_SURVIVORS, DH_BEAM_MAX_BEAMS
MARGIN = 1e-4
GROUP_COLS = 64
# route -> (EPT, NT) of beam_row_sample_fast_kernel<EPT, NT, ..>
FAST = {"f8": (8, 512), "f16": (16, 1024), "f36": (36, 1024), "f64": (64, 1024)}
ROUTES = ("f8", "f16", "f36", "f64", "general", "groups")
M32 = np.uint64(0xFFFFFFFF)


def n_groups(v):
    """hip.n_groups: the group maxima dh_vocab_logits leaves per row."""
    return 2 * ((v + 127) // 128)


def groups_allowed(v, top_k):
    """row_sample_groups_launch: "n_groups > 0 && n_groups <= 1024 && top_k <= n_groups"."""
    return n_groups(v) <= 1024 and top_k <= n_groups(v)


def route(v, top_k, exact=False, groups=False):
    """The row kernel a call runs.  ``groups``: dh_beam_row_sample_groups[_prompted], or the nucleus entry with group maxima;
    ``exact``: the *_exact entry points / the nucleus entry's flag.
      dh_beam_row_sample_nucleus: "if (group_max && !exact)" -> row_sample_groups_launch: beam_row_sample_groups_kernel<256, ..>
      row_sample_launch:
        "if (!exact && top_k <= 256 && V <= 512 * 8) DH_FAST(8, 512, 4);"
        "else if (!exact && top_k <= 256 && V <= 1024 * 16) DH_FAST(16, 1024, 8);"
        "else if (!exact && top_k <= 256 && V <= 1024 * 36) DH_FAST(36, 1024, 8);"
        "else if (!exact && top_k <= 256 && V <= 1024 * 64) DH_FAST(64, 1024, 4);"
        else beam_row_sample_kernel (256 threads, radix select over the row in memory)"""
    if groups and not exact:
        return "groups"
    if not exact and top_k <= 256:
        if v <= 512 * 8:
            return "f8"
        if v <= 1024 * 16:
            return "f16"
        if v <= 1024 * 36:
            return "f36"
        if v <= 1024 * 64:
            return "f64"
    return "general"


# ---- Philox (common.h) ------------------------------------------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32(counter, key):
    """Philox4x32-10 of common.h, vectorised: ``counter`` four and ``key`` two (arrays of) 32-bit words -> four uint32 arrays.
    Integer arithmetic only: exact."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in counter])
    k0, k1 = _u64(key[0]), _u64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def philox_u(o0):
    """"u = ((float)(o[0] >> 9) + 0.5f) * (1.0f / 8388608.0f)": exact in fp32, strictly inside (0, 1)."""
    return ((np.asarray(o0, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def philox_exp1(seed, img, step, kind, row, idx):
    """common.h philox_exp1 in fp64: counter (idx, row, step, kind), key (lo32(seed) ^ img * 0x9E3779B1, hi32(seed) + img).
    ``seed`` is the kernels' ``seed ^ *seed_ptr``; every other argument may be an array (broadcast)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    img = _u64(img)
    k0 = np.uint64(seed & 0xFFFFFFFF) ^ ((img * np.uint64(0x9E3779B1)) & M32)
    k1 = (np.uint64(seed >> 32) + img) & M32
    o = philox4x32((idx, row, _u64(step), _u64(kind)), (k0, k1))
    return -np.log(philox_u(o[0]))


def row_noise(seed, img0, step, rows, rows_per_img, v):
    """Stream kind 0, the row draw's table ``[rows, v]``: row ``rc`` is image ``img0 + rc // rows_per_img``, row ``rc % rows_per_img``."""
    rc = np.arange(rows)
    return philox_exp1(seed, (img0 + rc // rows_per_img)[:, None], step, 0, (rc % rows_per_img)[:, None], np.arange(v)[None, :])


def select_noise(seed, img0, step_index, n_img, beam):
    """Stream kind 1, the select's table ``[n_img, beam * beam]``: row 0, idx = candidate number."""
    return philox_exp1(seed, (img0 + np.arange(n_img))[:, None], step_index, 1, 0, np.arange(beam * beam)[None, :])


def final_noise(seed, img0, n_img, beam):
    """Stream kind 2, the final draw's table ``[n_img, beam]``: step 0xFFFFFFFF, idx = beam."""
    return philox_exp1(seed, (img0 + np.arange(n_img))[:, None], 0xFFFFFFFF, 2, 0, np.arange(beam)[None, :])


# ---- the row draw -----------------------------------------------------------------------------------------------------------------
def race_margin(q, n_top):
    """Smallest relative gap between consecutive values among the ``n_top + 1`` largest of ``q`` (descending); pairs that are both 0
    (dead: equal in every precision) and entries below 0 (cut from the race) do not count."""
    s = np.sort(np.asarray(q, dtype=np.float64))[::-1][:n_top + 1]
    m = float("inf")
    for a, b in zip(s[:-1], s[1:]):
        if a > 0 and b >= 0:
            m = min(m, (a - b) / a)
    return m


def row_draw(logits, noise, temperature, beam, top_k, unk, top_p=None):
    """``logits`` fp32 ``[rows, V]``, ``noise`` ``[rows, V]`` -> ``(picks int64 [rows, beam], values fp64 [rows, beam], flags [rows],
    margin [rows])``.

    Threshold = the ``top_k``-th largest by fp32 comparison (ties kept, ``-0.0 == +0.0``; a NaN of either sign is the largest of
    all, as ``torch.topk`` has it); ``unk`` dropped; ``p = softmax(x / T)`` over the survivors in fp64; with ``top_p`` the mask of
    ``nucleus_ref.nucleus_keep``; winners = the ``beam`` largest ``p / noise``, equal ``q`` to the lower token; values =
    log_softmax over the winners' untempered logits.  Flags: ALL_FILTERED no survivor; NONFINITE a NaN or +inf among the survivors
    (or nothing but ``-inf``): picks (0, 0.0), where the reference's ``torch.multinomial`` raises; TOO_FEW fewer than ``beam``
    survivors above ``-inf`` -- the slots behind them are dead: value ``-inf``, token unspecified (``-1`` here)."""
    x32 = torch.as_tensor(logits).detach().cpu().float().numpy()
    nz = np.asarray(torch.as_tensor(noise).detach().cpu().double().numpy() if not isinstance(noise, np.ndarray) else noise, dtype=np.float64)
    rows, v = x32.shape
    picks = np.zeros((rows, beam), dtype=np.int64)
    vals = np.zeros((rows, beam), dtype=np.float64)
    flags, margins = [0] * rows, [float("inf")] * rows
    for r in range(rows):
        x = x32[r]
        nan = np.isnan(x)
        xk = np.where(nan, np.float32(np.inf), x)
        kth = np.partition(xk, v - top_k)[v - top_k]
        surv = xk >= kth
        if 0 <= unk < v:
            surv[unk] = False
        idx = np.nonzero(surv)[0]
        if idx.size == 0:
            flags[r] = ERR_ALL_FILTERED
            continue
        xs = x[idx].astype(np.float64)
        if nan[idx].any() or (xs == np.inf).any() or xs.max() == -np.inf:
            flags[r] = ERR_NONFINITE
            continue
        y = xs / float(temperature)
        p = np.exp(y - y.max())
        p /= p.sum()
        q = p / nz[r, idx]
        if top_p is not None:
            filt = torch.full((1, v), float("-inf"))
            filt[0, idx] = torch.from_numpy(x[idx])
            keep, nm = nucleus_keep(filt, temperature, top_p, beam)
            q = np.where(keep[0].numpy()[idx], q, -1.0)
            margins[r] = nm
        order = np.argsort(-q, kind="stable")[:beam]             # stable: equal q keeps the lower token first
        live = int((xs > -np.inf).sum())
        n = min(beam, live)
        win = idx[order[:n]]
        picks[r, :n] = win
        picks[r, n:] = -1
        lx = x[win].astype(np.float64)
        vals[r, :n] = lx - (lx.max() + np.log(np.exp(lx - lx.max()).sum()))
        vals[r, n:] = -np.inf
        if live < beam:
            flags[r] |= ERR_TOO_FEW
        margins[r] = min(margins[r], race_margin(q, beam))
    return torch.from_numpy(picks), torch.from_numpy(vals), flags, margins


def fast_candidates(row, top_k, rt):
    """How many values of ``row`` (1-D fp32, finite) pass the single-pass kernels' cheap bound -- "the k-th largest of the per-thread
    maxima", thread ``i % NT`` holding columns ``i, i + NT, ..`` -- i.e. what the kernel compacts before ``if (s_cnt > CAP)``."""
    ept, nt = FAST[rt]
    x = np.full(ept * nt, -np.inf, dtype=np.float32)
    x[:len(row)] = np.asarray(row, dtype=np.float32)
    tmax = np.sort(x.reshape(ept, nt).max(0))[::-1]
    return int((x >= tmax[top_k - 1]).sum())


def f2key(x):
    """beam.hip f2key for non-NaN fp32 values."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, ~u & M32, u | np.uint64(0x80000000))


def group_candidates(row, top_k):
    """The same for the group-guided kernel: the bound is the lower edge of the 16-bit key bucket of the ``min(top_k, n_groups)``-th
    largest group maximum; every value >= it inside a group whose maximum reaches it is compacted."""
    v, ng = len(row), n_groups(len(row))
    x = np.full(ng * GROUP_COLS, -np.inf, dtype=np.float32)
    x[:v] = np.asarray(row, dtype=np.float32)
    keys = f2key(x).reshape(ng, GROUP_COLS)
    gk = np.sort(keys.max(1))[::-1]
    bound = gk[min(top_k, ng) - 1] & np.uint64(0xFFFF0000)
    return int((keys[:, :] >= bound).sum())       # (a value >= bound lifts its group's maximum to >= bound: the group is selected)


# ---- the sampled select and the final draw ---------------------------------------------------------------------------------------
def select_sampled(state, pick_idx, pick_val, noise, temperature, first, write_pos, t, step_index, eos, first_pos=None,
                   first_sets_ended=True):
    """``dh_beam_select`` / ``dh_beam_select_prompted`` on ``state`` (``beam_search_ref.State``) IN PLACE; returns the per-image race
    margins.  ``beam_search_ref.select_best`` with two differences: ``keep`` = the ``beam`` winners of ``softmax(cand / T) / noise``
    in fp64, equal ``q`` to the lower candidate (a first step keeps pick order), ``noise[img * beam * beam + c]``; and
    ``hparent = base + c // beam`` -- "rnn_models.py:135-137: dense B*B layout index", as the kernel's comment says."""
    b = state.beam
    pick_idx = torch.as_tensor(pick_idx).reshape(-1).tolist()
    pick_val = torch.as_tensor(pick_val).to(torch.float32).reshape(-1).numpy()
    noise = np.asarray(noise, dtype=np.float64).reshape(-1)
    tok_ld = state.tokens.shape[1]
    margins = []
    for img in range(state.n_img):
        base = img * b
        is_first, pk_row = bool(first), img
        margins.append(float("inf"))
        if first_pos is not None:
            fp = int(first_pos[img])
            if step_index < fp:
                state.parent[base:base + b] = base
                state.hparent[base:base + b] = base
                if state.src is not None:
                    state.src[base:base + b, t] = base
                continue
            is_first, pk_row = step_index == fp, base
        if state.done[img]:
            continue
        toks, scores, pars, ends = candidates(state, img, pick_idx, pick_val, is_first, first_sets_ended, eos, pk_row)
        if is_first:
            keep = list(range(b))
        else:
            y = np.array(scores, dtype=np.float32).astype(np.float64) / float(temperature)
            p = np.exp(y - y.max())
            q = (p / p.sum()) / noise[img * b * b: img * b * b + len(scores)]
            keep = np.argsort(-q, kind="stable")[:b].tolist()
            margins[-1] = race_margin(q, b)
        while len(keep) < b:
            keep.append(min(len(keep), len(scores) - 1))
        old_tok = state.tokens[base:base + b].clone()
        old_src = None if state.src is None else state.src[base:base + b].clone()
        all_ended = True
        for slot, c in enumerate(keep):
            par = pars[c]
            state.tokens[base + slot] = old_tok[par]
            if write_pos < tok_ld:
                state.tokens[base + slot, write_pos] = toks[c]
            if state.src is not None:
                state.src[base + slot, :t] = old_src[par, :t]
                state.src[base + slot, t] = base + par
            state.vals[base + slot] = float(scores[c])
            state.ended[base + slot] = ends[c]
            state.parent[base + slot] = base + par
            state.hparent[base + slot] = base + c // b
            all_ended = all_ended and bool(ends[c])
        if all_ended and not is_first:
            state.done[img] = 1
            state.end_step[img] = step_index
    return margins


def final_draw(vals, noise, temperature):
    """``vals`` fp32 ``[n_img, beam]``, ``noise [n_img, beam]`` -> ``(beam drawn per image, margins)``: arg-max of
    ``softmax(vals / T) / noise``, the first index on ties."""
    y = torch.as_tensor(vals).detach().cpu().double().numpy() / float(temperature)
    nz = np.asarray(noise, dtype=np.float64).reshape(y.shape)
    drawn, margins = [], []
    for r in range(y.shape[0]):
        p = np.exp(y[r] - y[r].max())
        q = (p / p.sum()) / nz[r]
        drawn.append(int(np.argmax(q)))
        margins.append(race_margin(q, 1))
    return drawn, margins
