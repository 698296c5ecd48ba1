"""Torch-CPU restatement of ``search="beam"`` with ``early_stopping`` (``dh_beam_select_pool`` / ``dh_beam_finalize_pool``), built on
``beam_search_ref`` and ``length_penalty_ref``: the select step with its finished-hypothesis pool, the finalize, and a whole-search
driver, in bit-exact fp32 numpy arithmetic (one add, one multiply).

The pool of an image: ``pool_tokens [beam, max_len]``, ``pool_keys`` / ``pool_vals [beam]``, ``pool_len [beam]``, ``pool_n``; physically
sorted, slot 0 the largest key, equal keys in order of arrival.  ``state.ended`` marks DEAD slots here (``vals = keys = -inf``).

A step of an image that is neither done nor forced: the candidates in ``beam_search_ref.candidates``' order with their keys; ranked by
key (larger first, equal keys to the lower candidate index, ``-inf`` last; a first step keeps pick order); down the ranking a candidate
whose token is ``<eos>`` never takes a slot -- with rank ``< beam`` and key ``> -inf`` it is offered to the pool --, every other candidate
with key ``> -inf`` takes the next live slot until ``beam`` are taken; the slots left over are dead (their own row with token 0, ``-inf``,
``parent = hparent = src[.., t]`` themselves -- at a first step the image's base row, the only one with decoder state behind it); then
the done rule."""
import numpy as np
import torch

import beam_search_ref as R
import length_penalty_ref as LP

f32 = np.float32
NEG = float("-inf")


def new_state(n_img, beam, max_len, src_len=0, pad_index=0):
    """``length_penalty_ref.new_state`` plus an empty pool per image."""
    s = LP.new_state(n_img, beam, max_len, src_len, pad_index)
    s.pool_tokens = torch.zeros(n_img, beam, max_len, dtype=torch.int32)
    s.pool_keys = torch.full((n_img, beam), NEG, dtype=torch.float32)
    s.pool_vals = torch.zeros(n_img, beam, dtype=torch.float32)
    s.pool_len = torch.zeros(n_img, beam, dtype=torch.int32)
    s.pool_n = torch.zeros(n_img, dtype=torch.int32)
    return s


POOL_FIELDS = ("pool_tokens", "pool_keys", "pool_vals", "pool_len", "pool_n")


def fields(state):
    """Every tensor ``select_pool`` may write."""
    d = dict(state.fields(), keys=state.keys)
    d.update({k: getattr(state, k) for k in POOL_FIELDS})
    return d


def pool_insert(state, img, row, key, val, length):
    """Behind every entry whose key is ``>=`` ``key``; entry ``beam`` falls off.  Returns whether it went in."""
    b = state.beam
    n = int(state.pool_n[img])
    at = sum(1 for j in range(n) if f32(state.pool_keys[img, j]) >= f32(key))
    if at >= b:
        return False
    for j in range(min(n, b - 1), at, -1):                # from the bottom up
        state.pool_tokens[img, j] = state.pool_tokens[img, j - 1]
        state.pool_keys[img, j] = state.pool_keys[img, j - 1]
        state.pool_vals[img, j] = state.pool_vals[img, j - 1]
        state.pool_len[img, j] = state.pool_len[img, j - 1]
    state.pool_tokens[img, at] = row
    state.pool_keys[img, at] = float(key)
    state.pool_vals[img, at] = float(val)
    state.pool_len[img, at] = int(length)
    state.pool_n[img] = min(n + 1, b)
    return True


def select_pool(state, pick_idx, pick_val, first, write_pos, t, step_index, eos, len_w, early_stopping, first_col=0, first_pos=None):
    """``dh_beam_select_pool`` on ``state`` (``new_state``'s layout) IN PLACE; ``early_stopping`` is ``True`` or ``False``."""
    assert isinstance(early_stopping, bool)
    b = state.beam
    pick_idx = torch.as_tensor(pick_idx).reshape(-1).tolist()
    pick_val = torch.as_tensor(pick_val).to(torch.float32).reshape(-1).numpy()
    len_w = torch.as_tensor(len_w).to(torch.float32).numpy()
    tok_ld = state.tokens.shape[1]
    assert 0 <= write_pos < tok_ld
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
        toks, scores, pars, _ = R.candidates(state, img, pick_idx, pick_val, is_first, False, eos, pk_row)
        if is_first:
            keys = [LP.key_of(s, w) for s in scores]
            order = list(range(b))
        else:
            keys, c = [], 0
            for k in range(b):                            # a dead slot brings its one candidate with the key it holds
                if state.ended[base + k]:
                    keys.append(f32(state.keys[base + k]))
                    c += 1
                else:
                    keys += [LP.key_of(scores[c + j], w) for j in range(b)]
                    c += b
            assert c == len(scores)
            order = R.rank_desc(torch.tensor(np.array(keys, dtype=np.float32)))
        old_tok = state.tokens[base:base + b].clone()
        old_src = None if state.src is None else state.src[base:base + b].clone()
        kept, offers = [], []
        # (the walk looks at 2 * beam ranks: a row's picks are distinct tokens, so at most `beam` candidates are <eos> and the first
        #  2 * beam ranks hold `beam` others, or reach the -inf tail)
        for rank, c in enumerate(order[:2 * b]):
            if not keys[c] > NEG:
                continue
            if toks[c] == eos:
                if rank < b:
                    offers.append(c)
            elif len(kept) < b:
                kept.append(c)
        for slot in range(b):
            dead = slot >= len(kept)
            c = None if dead else kept[slot]
            # (a first step: only the base row has decoder state behind it, so a dead slot points there; it holds the same prefix)
            par = (0 if is_first else slot) if dead else pars[c]
            state.tokens[base + slot] = old_tok[par]
            state.tokens[base + slot, write_pos] = 0 if dead else toks[c]
            if state.src is not None:
                state.src[base + slot, :t] = old_src[par, :t]
                state.src[base + slot, t] = base + par
            state.vals[base + slot] = NEG if dead else float(scores[c])
            state.keys[base + slot] = NEG if dead else float(keys[c])
            state.ended[base + slot] = int(dead)
            state.parent[base + slot] = base + par
            state.hparent[base + slot] = base + par
        for c in offers:
            row = old_tok[pars[c]].clone()
            row[write_pos] = eos
            pool_insert(state, img, row, keys[c], scores[c], write_pos + 1)
        if int(state.pool_n[img]) == b:
            top = f32(keys[kept[0]]) if kept else f32(NEG)
            if early_stopping or f32(state.pool_keys[img, b - 1]) >= top:
                state.done[img] = 1
                state.end_step[img] = step_index
    return state


def finalize_pool(state, full_len, pad_index=0, out_ld=None):
    """``dh_beam_finalize_pool``: ``dict(tokens [N, B, T], lengths, scores, beam_index [N, B], drawn [N] = 0, row_lengths [N])``.  The
    pool and the state are left as they are."""
    n, b = state.n_img, state.beam
    tok_ld = state.tokens.shape[1]
    out_ld = tok_ld if out_ld is None else out_ld
    cap = min(out_ld, tok_ld)
    tokens = torch.full((n, b, out_ld), pad_index, dtype=torch.int64)
    lengths = torch.zeros(n, b, dtype=torch.int64)
    scores = torch.zeros(n, b, dtype=torch.float32)
    index = torch.zeros(n, b, dtype=torch.int64)
    llen = min(max(full_len, 0), cap)
    for img in range(n):
        base = img * b
        entries = []                                      # (key, row, length, beam_index) in order of arrival
        for j in range(int(state.pool_n[img])):
            entries.append((f32(state.pool_keys[img, j]), state.pool_tokens[img, j], min(max(int(state.pool_len[img, j]), 0), cap), -1))
        offered = set()
        if not state.done[img]:
            for k in range(b):
                if not state.ended[base + k]:
                    key = f32(state.keys[base + k])
                    entries.append((f32(NEG) if np.isnan(key) else key, state.tokens[base + k], llen, k))
                    offered.add(k)
        order = R.rank_desc(torch.tensor(np.array([e[0] for e in entries], dtype=np.float32))) if entries else []
        result = [entries[i] for i in order][:b]
        for k in range(b):                                # the slots that were not offered follow at -inf
            if len(result) < b and k not in offered:
                result.append((f32(NEG), state.tokens[base + k], llen, k))
        for slot, (key, row, ln, idx) in enumerate(result):
            tokens[img, slot, :ln] = row[:ln].long()
            lengths[img, slot] = ln
            scores[img, slot] = float(key)
            index[img, slot] = idx
    return dict(tokens=tokens, lengths=lengths, scores=scores, beam_index=index, drawn=torch.zeros(n, dtype=torch.int64),
                row_lengths=lengths[:, 0].clone())


def beam_search_pool(logits_fn, n_img, beam, max_len, length_penalty, early_stopping, temperature=1.0, unk=1, eos=3, pad_index=0,
                     trace=None):
    """``length_penalty_ref.beam_search_norm`` with the pool: ``(finalize_pool's dict, error bits, state)``.  A done image takes no
    further step; the loop ends when every image is done (what ``early_stop_every=1`` does).  ``trace`` (a list) collects ``(pos,
    done as a list)`` after every step."""
    state = new_state(n_img, beam, max_len, pad_index=pad_index)
    len_w = LP.weights(length_penalty, max_len)
    err = 0
    for pos in range(max_len):
        first = pos == 0
        rows = state.tokens[::beam] if first else state.tokens
        logits = logits_fn(rows, pos, 1 if first else beam)
        picks, vals, errs = R.row_best(logits, temperature, beam, unk)
        for e in errs:
            err |= e
        select_pool(state, picks, vals.to(torch.float32), first, pos, 0, pos, eos, len_w, early_stopping, first_col=0)
        if trace is not None:
            trace.append((pos, state.done.tolist()))
        if bool(state.done.all()):
            break
    return finalize_pool(state, max_len, pad_index), err, state
