"""Torch-CPU restatement of ``search="beam"`` with ``num_beam_groups`` / ``diversity_penalty`` (``dh_beam_select_groups``), built on
``beam_search_ref`` and ``length_penalty_ref``: the select step with its two separately rounded fp32 operations in numpy, a second,
independent statement of one group step that ranks over the WHOLE vocabulary (no picks), and a whole-search driver.

The ``beam`` slots of an image are ``G`` groups of ``Bg = beam // G``: slots ``g * Bg .. g * Bg + Bg - 1`` are group ``g``.  The
candidate list and the keys ``q = fp32(score * w[L])`` are ``length_penalty_ref``'s; candidate ``c`` belongs to group ``parent // Bg``,
at an image's first step to every group.  For ``g = 0 .. G - 1``: ``said`` holds the tokens kept at this position by the groups before;
a candidate of a live row with a finite key gets ``pen = fp32(q - fp32(lam * fp32(count of its token in said)))``, every other ``pen =
q``; the ``Bg`` largest ``pen`` (equal values to the lower candidate index, ``-inf`` and NaN last) go to slots ``g * Bg + rank``; their
tokens join ``said`` unless the candidate is an ended beam's or its key is not ``> -inf``.  What is stored is not penalised."""
import numpy as np
import torch

import beam_search_ref as R
import length_penalty_ref as LP

f32 = np.float32
new_state = LP.new_state
finalize_norm = LP.finalize_norm
weights = LP.weights


def penalised(q, lam, count):
    """``fp32(q - fp32(lam * fp32(count)))``: two roundings, never one fused operation."""
    with np.errstate(all="ignore"):
        d = f32(f32(lam) * f32(count))
        return f32(f32(q) - d)


def group_keep(toks, keys, pars, live, first, beam, n_groups, lam):
    """The candidates kept by one image's step, slot by slot (``beam`` candidate indices): ``toks`` / ``keys`` (fp32) / ``pars`` the
    candidate list, ``live[c]`` False for an ended beam's single candidate."""
    bg = beam // n_groups
    said, keep = [], []
    for g in range(n_groups):
        mine = [c for c in range(len(toks)) if first or pars[c] // bg == g]
        pen = []
        for c in mine:
            k = f32(keys[c])
            if live[c] and np.isfinite(k):
                pen.append(penalised(k, lam, sum(1 for s in said if s == toks[c])))
            else:
                pen.append(k)
        order = R.rank_desc(torch.tensor(np.array(pen, dtype=np.float32)))[:bg]
        kept = [mine[i] for i in order]
        assert len(kept) == bg                      # (a group's rows bring at least one candidate each)
        keep += kept
        said += [toks[c] for c in kept if live[c] and f32(keys[c]) > f32(R.NEG)]
    return keep


def select_groups(state, pick_idx, pick_val, first, write_pos, t, step_index, eos, len_w, n_groups, lam, first_col=0, first_pos=None,
                  first_sets_ended=True):
    """``dh_beam_select_groups`` on ``state`` (with ``state.keys``) IN PLACE: the arguments of ``length_penalty_ref.select_best_norm``
    plus ``n_groups`` and ``lam``."""
    b = state.beam
    pick_idx = torch.as_tensor(pick_idx).reshape(-1).tolist()
    pick_val = torch.as_tensor(pick_val).to(torch.float32).reshape(-1).numpy()
    len_w = torch.as_tensor(len_w).to(torch.float32).numpy()
    tok_ld = state.tokens.shape[1]
    for img in range(state.n_img):
        base = img * b
        is_first, pk_row, col0 = bool(first), img, int(first_col)
        if first_pos is not None:
            fp = int(first_pos[img])
            col0 = fp
            if step_index < fp:
                state.parent[base:base + b] = base
                state.hparent[base:base + b] = base
                if state.src is not None:
                    state.src[base:base + b, t] = base
                continue
            is_first, pk_row = step_index == fp, base
        if state.done[img]:
            continue
        w = len_w[min(max(write_pos + 1 - col0, 0), tok_ld)]
        toks, scores, pars, ends = R.candidates(state, img, pick_idx, pick_val, is_first, first_sets_ended, eos, pk_row)
        if is_first:
            keys = [LP.key_of(s, w) for s in scores]
            live = [True] * len(toks)
        else:
            keys, live, c = [], [], 0
            for k in range(b):
                if state.ended[base + k]:
                    keys.append(f32(state.keys[base + k]))
                    live.append(False)
                    c += 1
                else:
                    keys += [LP.key_of(scores[c + j], w) for j in range(b)]
                    live += [True] * b
                    c += b
            assert c == len(scores)
        keep = group_keep(toks, keys, pars, live, is_first, b, n_groups, lam)
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
            state.vals[base + slot] = float(scores[c])               # NOT penalised
            state.keys[base + slot] = float(keys[c])                 # NOT penalised
            state.ended[base + slot] = ends[c]
            state.parent[base + slot] = base + par
            state.hparent[base + slot] = base + par
            all_ended = all_ended and bool(ends[c])
        if all_ended and not is_first:
            state.done[img] = 1
            state.end_step[img] = step_index
    return state


def group_step_whole_vocab(logp, vals, keys, ended, first, beam, n_groups, lam, w, unk=-1):
    """The second statement, for ONE image and from full rows -- no picks, no candidate list: ``logp`` fp32 ``[1 or beam, V]`` the
    rows' log-probabilities (``-inf``: not eligible), ``vals`` / ``keys`` / ``ended`` the image's ``beam`` slots.  Every group ranks
    ``(row, token)`` over the whole vocabulary of its rows (a first step: of the one row) and returns, slot by slot, ``(parent slot,
    token or None for an ended beam's candidate, raw score fp32, key fp32)``.  Order among equals: the lower row, then the better
    rank inside the row (larger log-probability, then the lower token), which is the candidate list's order."""
    bg = beam // n_groups
    logp = np.asarray(logp, dtype=np.float32)
    v = logp.shape[1]
    said, out = [], []
    for g in range(n_groups):
        items = []                                  # (pen, parent, row order, token, score, key, live)
        rows = [0] if first else range(g * bg, g * bg + bg)
        for k in rows:
            if not first and ended[k]:
                items.append((f32(keys[k]), k, 0, None, f32(vals[k]) + f32(0.0), f32(keys[k]), False))
                continue
            order = sorted((tok for tok in range(v) if tok != unk), key=lambda tok: (-logp[k, tok], tok))
            for rank, tok in enumerate(order):
                with np.errstate(all="ignore"):
                    score = f32(logp[k, tok]) if first else f32(f32(vals[k]) + f32(logp[k, tok]))
                key = LP.key_of(score, w)
                pen = penalised(key, lam, sum(1 for s in said if s == tok)) if np.isfinite(key) else key
                items.append((pen, k, rank, tok, score, key, True))
        items.sort(key=lambda it: (-it[0] if not np.isnan(it[0]) else np.inf, it[1], it[2]))
        kept = items[:bg]
        out += [(it[1], it[3], it[4], it[5]) for it in kept]
        said += [it[3] for it in kept if it[6] and it[5] > f32(R.NEG)]
    return out


def beam_search_groups(logits_fn, n_img, beam, max_len, n_groups, lam, length_penalty=0.0, temperature=1.0, unk=1, eos=3, pad_index=0,
                       len_bias_done=1):
    """``length_penalty_ref.beam_search_norm`` (dense, no prefix) with groups: ``(finalize_norm's dict, error bits, state)``."""
    state = new_state(n_img, beam, max_len, pad_index=pad_index)
    len_w = weights(length_penalty, max_len)
    err = 0
    for pos in range(max_len):
        first = pos == 0
        rows = state.tokens[::beam] if first else state.tokens
        logits = logits_fn(rows, pos, 1 if first else beam)
        picks, vals, errs = R.row_best(logits, temperature, beam, unk)
        for e in errs:
            err |= e
        select_groups(state, picks, vals.to(torch.float32), first, pos, 0, pos, eos, len_w, n_groups, lam, first_col=0)
    return finalize_norm(state, len_bias_done, max_len, pad_index, eos), err, state


def group_best(result, n_groups):
    """Per image the best slot of every group of a ``finalize_norm`` dict: ``[N, G]`` slot numbers (the first slot in score order
    whose ``beam_index // Bg`` is the group)."""
    idx = result["beam_index"]
    n, b = idx.shape
    bg = b // n_groups
    out = torch.zeros(n, n_groups, dtype=torch.int64)
    for i in range(n):
        for g in range(n_groups):
            out[i, g] = next(s for s in range(b) if int(idx[i, s]) // bg == g)
    return out
