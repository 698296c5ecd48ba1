"""Torch-CPU restatement of ``search="beam"`` with ``length_penalty`` (``dh_beam_select_best_norm``), built on ``beam_search_ref``: the
weight table, the select step on ``key = fp32(score * w[L])`` in bit-exact fp32 numpy arithmetic, the final ordering on the keys, and a
whole-search driver.  At ``length_penalty = 0`` every weight is 1 and all of it is ``beam_search_ref``'s, bit for bit.

``L`` is the number of columns the search has written to a beam, counted from the image's first generated column: a live candidate of
a step that writes column ``write_pos`` has ``L = write_pos + 1 - first column``; an ended beam's candidate keeps the key it was kept
with.  Order: larger key first, equal keys to the lower candidate index, ``-inf`` last."""
import copy

import numpy as np
import torch

import beam_search_ref as R

f32 = np.float32


def weights(length_penalty, max_len):
    """fp32 ``[max_len + 1]``: ``w[0] = 1``, ``w[L] = float32(float64(L) ** -length_penalty)``."""
    w = np.ones(max_len + 1, dtype=np.float64)
    for n in range(1, max_len + 1):
        w[n] = np.float64(n) ** np.float64(-float(length_penalty))
    return torch.from_numpy(w.astype(np.float32))


def new_state(n_img, beam, max_len, src_len=0, pad_index=0):
    """``beam_search_ref.State`` plus the per-row ``keys`` (zeros)."""
    s = R.State(n_img, beam, max_len, src_len, pad_index)
    s.keys = torch.zeros(n_img * beam, dtype=torch.float32)
    return s


def key_of(score, w):
    """ONE fp32 multiply of the fp32 score; ``-inf`` stays ``-inf`` (``w`` is a positive normal number)."""
    with np.errstate(all="ignore"):
        return f32(f32(score) * f32(w))


def select_best_norm(state, pick_idx, pick_val, first, write_pos, t, step_index, eos, len_w, first_col=0, first_pos=None,
                     first_sets_ended=True):
    """``dh_beam_select_best_norm`` on ``state`` (with ``state.keys``) IN PLACE; the arguments of ``beam_search_ref.select_best`` plus
    ``len_w`` (fp32 ``[tok_ld + 1]``) and ``first_col`` (dense; a prompted batch counts from ``first_pos[img]``)."""
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
            keys = [key_of(s, w) for s in scores]
            keep = list(range(b))
        else:
            keys, c = [], 0
            for k in range(b):                    # the candidate list's own order: an ended beam brings one, a live beam `beam`
                if state.ended[base + k]:
                    keys.append(f32(state.keys[base + k]))
                    c += 1
                else:
                    keys += [key_of(scores[c + j], w) for j in range(b)]
                    c += b
            assert c == len(scores)
            keep = R.rank_desc(torch.tensor(np.array(keys, dtype=np.float32)))[:b]
        while len(keep) < b:
            keep.append(keep[-1])
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
            state.keys[base + slot] = float(keys[c])
            state.ended[base + slot] = ends[c]
            state.parent[base + slot] = base + par
            state.hparent[base + slot] = base + par
            all_ended = all_ended and bool(ends[c])
        if all_ended and not is_first:
            state.done[img] = 1
            state.end_step[img] = step_index
    return state


def finalize_norm(state, len_bias_done, full_len, pad_index=0, eos=3, pos=0, first_pos=None, out_ld=None):
    """``beam_search_ref.finalize_best`` with ``state.keys`` in the place of ``vals``: ``scores`` are the keys."""
    by_key = copy.copy(state)
    by_key.vals = state.keys
    return R.finalize_best(by_key, len_bias_done, full_len, pad_index, eos, pos, first_pos, out_ld)


def beam_search_norm(logits_fn, n_img, beam, max_len, length_penalty, temperature=1.0, unk=1, eos=3, pad_index=0, len_bias_done=1):
    """``beam_search_ref.beam_search`` (dense, no prefix) with ``length_penalty``: ``(finalize_norm's dict, error bits, state)``."""
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
        select_best_norm(state, picks, vals.to(torch.float32), first, pos, 0, pos, eos, len_w, first_col=0)
    return finalize_norm(state, len_bias_done, max_len, pad_index, eos), err, state
