"""Torch-CPU restatement of ``search="beam"`` (the reference has no such search, so this is the yardstick): the row step in fp64, the
select step in fp32 with the engine's single add -- bit-exact --, the final ordering, and a whole-search driver over a logits function.

Order everywhere: larger first, equal values to the lower index, ``-inf`` last.  ``torch.sort(stable=True, descending=True)`` is that
order (``-0.0 == +0.0`` compare equal and keep their index order)."""
import numpy as np
import torch

ERR_ALL_FILTERED, ERR_TOO_FEW, ERR_NONFINITE = 1, 4, 8
NEG = float("-inf")


def row_best(logits, temperature, beam, unk):
    """``logits`` fp32 ``[rows, V]`` -> ``(picks int64 [rows, beam], vals fp64 [rows, beam], err int per row)``.

    ``lse = logsumexp(x / T)`` over every column in fp64; the picks are the ``beam`` columns with the largest stored logit, never
    ``unk`` or ``-inf``; ``val = x / T - lse``.  A NaN / +inf row: NONFINITE, picks 0 at 0.  Nothing eligible: ALL_FILTERED, picks 0 at
    0.  Fewer than ``beam``: TOO_FEW, the rest token 0 at ``-inf``."""
    x = logits.detach().cpu().float()
    rows, v = x.shape
    picks = torch.zeros(rows, beam, dtype=torch.int64)
    vals = torch.zeros(rows, beam, dtype=torch.float64)
    err = [0] * rows
    y = x.double() / float(temperature)
    for r in range(rows):
        if bool(torch.isnan(x[r]).any()) or bool((x[r] == float("inf")).any()):
            err[r] = ERR_NONFINITE
            continue
        elig = x[r].clone()
        if 0 <= unk < v:
            elig[unk] = NEG
        n = int((elig > NEG).sum())
        if n == 0:
            err[r] = ERR_ALL_FILTERED
            continue
        lse = torch.logsumexp(y[r], 0)
        order = torch.sort(elig, stable=True, descending=True).indices[:min(beam, n)]
        picks[r, :len(order)] = order
        vals[r, :len(order)] = y[r, order] - lse
        if n < beam:
            err[r] = ERR_TOO_FEW
            vals[r, n:] = NEG
    return picks, vals, err


def rank_desc(scores):
    """Indices of ``scores`` (1-D), largest first, equal scores in index order, NaN as ``-inf``."""
    s = torch.as_tensor(scores).clone()
    s[torch.isnan(s)] = NEG
    return torch.sort(s, stable=True, descending=True).indices.tolist()


class State:
    """The engine's beam state of ``n_img`` images x ``beam`` beams on the CPU, as ``BeamSearchHelper`` lays it out."""

    def __init__(self, n_img, beam, max_len, src_len=0, pad_index=0):
        r = n_img * beam
        self.n_img, self.beam = n_img, beam
        self.tokens = torch.full((r, max_len), pad_index, dtype=torch.int32)
        self.vals = torch.zeros(r, dtype=torch.float32)
        self.ended = torch.zeros(r, dtype=torch.uint8)
        base = (torch.arange(r, dtype=torch.int32) // beam) * beam
        self.src = base[:, None].expand(r, src_len).contiguous() if src_len else None
        self.parent = torch.zeros(r, dtype=torch.int32)
        self.hparent = torch.zeros(r, dtype=torch.int32)
        self.done = torch.zeros(n_img, dtype=torch.uint8)
        self.end_step = torch.zeros(n_img, dtype=torch.int32)

    @classmethod
    def of(cls, tokens, vals, ended, done, end_step, beam, src=None, parent=None, hparent=None):
        """From snapshots of the engine's tensors (copied)."""
        s = cls.__new__(cls)
        c = lambda t, dt: None if t is None else t.detach().cpu().to(dt).clone()
        s.tokens, s.vals, s.ended = c(tokens, torch.int32), c(vals, torch.float32), c(ended, torch.uint8)
        s.done, s.end_step, s.src = c(done, torch.uint8), c(end_step, torch.int32), c(src, torch.int32)
        r = s.tokens.shape[0]
        s.parent = c(parent, torch.int32) if parent is not None else torch.zeros(r, dtype=torch.int32)
        s.hparent = c(hparent, torch.int32) if hparent is not None else torch.zeros(r, dtype=torch.int32)
        s.beam, s.n_img = beam, r // beam
        return s

    def fields(self):
        return dict(tokens=self.tokens, vals=self.vals, ended=self.ended, src=self.src, parent=self.parent, hparent=self.hparent,
                    done=self.done, end_step=self.end_step)


def candidates(state, img, pick_idx, pick_val, first, first_sets_ended, eos, pk_row):
    """The candidate list of one image in the engine's order: ``(tokens, scores fp32, parents, ended)``.  ``pick_idx`` / ``pick_val``
    are the FLAT pick tables (``[rows * beam]``); a first step reads the ``beam`` picks of flat row ``pk_row``."""
    b, base = state.beam, img * state.beam
    f32 = np.float32
    toks, scores, pars, ends = [], [], [], []
    if first:
        for j in range(b):
            tok = int(pick_idx[pk_row * b + j])
            toks.append(tok)
            scores.append(f32(pick_val[pk_row * b + j]))
            pars.append(0)
            ends.append(int(bool(first_sets_ended) and tok == eos))
        return toks, scores, pars, ends
    for k in range(b):
        vb = f32(state.vals[base + k])
        if state.ended[base + k]:
            toks.append(0)
            scores.append(f32(vb + f32(0.0)))
            pars.append(k)
            ends.append(1)
            continue
        for j in range(b):
            tok = int(pick_idx[(base + k) * b + j])
            toks.append(tok)
            scores.append(f32(vb + f32(pick_val[(base + k) * b + j])))        # ONE fp32 add, as the kernel
            pars.append(k)
            ends.append(int(tok == eos))
    return toks, scores, pars, ends


def select_best(state, pick_idx, pick_val, first, write_pos, t, step_index, eos, first_pos=None, first_sets_ended=True):
    """``dh_beam_select_best`` on ``state`` IN PLACE.  ``pick_idx`` int / ``pick_val`` fp32 ``[rows, beam]`` (or flat) as the row step
    left them; dense: ``first`` for the whole batch, its picks at flat row ``img``; ``first_pos`` (list of ints): the prompted phases
    against ``step_index``, an image's first step reads the picks of its base row."""
    b = state.beam
    pick_idx = torch.as_tensor(pick_idx).reshape(-1).tolist()
    pick_val = torch.as_tensor(pick_val).to(torch.float32).reshape(-1).numpy()
    tok_ld = state.tokens.shape[1]
    for img in range(state.n_img):
        base = img * b
        is_first, pk_row = bool(first), img
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
        keep = list(range(b)) if is_first else rank_desc(torch.tensor(np.array(scores, dtype=np.float32)))[:b]
        while len(keep) < b:                  # (fewer candidates than beams cannot happen: a live beam brings `beam` of them)
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
            state.ended[base + slot] = ends[c]
            state.parent[base + slot] = base + par
            state.hparent[base + slot] = base + par
            all_ended = all_ended and bool(ends[c])
        if all_ended and not is_first:
            state.done[img] = 1
            state.end_step[img] = step_index
    return state


def finalize_best(state, len_bias_done, full_len, pad_index=0, eos=3, pos=0, first_pos=None, out_ld=None):
    """``dh_beam_finalize_beams``' score order without its draw: ``dict(tokens [N, B, T], lengths [N, B], scores [N, B], beam_index
    [N, B], drawn [N] = 0, row_lengths [N])``; slot 0 is the caption ``search="beam"`` returns."""
    n, b = state.n_img, state.beam
    tok_ld = state.tokens.shape[1]
    out_ld = tok_ld if out_ld is None else out_ld
    tokens = torch.full((n, b, out_ld), pad_index, dtype=torch.int64)
    lengths = torch.zeros(n, b, dtype=torch.int64)
    scores = torch.zeros(n, b, dtype=torch.float32)
    index = torch.zeros(n, b, dtype=torch.int64)
    row_len = torch.zeros(n, dtype=torch.int64)
    for img in range(n):
        base = img * b
        ln = int(state.end_step[img]) + len_bias_done if state.done[img] else full_len
        ln = min(ln, out_ld, tok_ld)
        row_len[img] = ln
        p0 = pos if first_pos is None else int(first_pos[img])
        for slot, k in enumerate(rank_desc(state.vals[base:base + b])):
            row = state.tokens[base + k, :ln].long()
            tokens[img, slot, :ln] = row
            scores[img, slot] = state.vals[base + k]
            index[img, slot] = k
            hits = [i for i in range(p0, ln) if int(row[i]) == eos]
            lengths[img, slot] = hits[0] + 1 if hits else ln
    return dict(tokens=tokens, lengths=lengths, scores=scores, beam_index=index, drawn=torch.zeros(n, dtype=torch.int64), row_lengths=row_len)


def candidate_gaps(state, picks, vals64, first, first_pos=None, step_index=0):
    """Per image, in fp64: the difference between the ``beam``-th and the ``(beam + 1)``-th largest candidate score of the step that
    ``select_best`` is about to make on ``state`` (``inf`` where there is no ``(beam + 1)``-th, where the image takes no step, and
    where both are ``-inf``: dead candidates tie exactly in every precision).  A step whose gap is tiny is a coin toss between the
    fp32 engine and an fp64 restatement; everything else must agree."""
    b = state.beam
    picks, vals64 = torch.as_tensor(picks).reshape(-1, b), torch.as_tensor(vals64).double().reshape(-1, b)
    gaps = []
    for img in range(state.n_img):
        base = img * b
        is_first, pk_row = bool(first), img
        if first_pos is not None:
            is_first, pk_row = step_index == int(first_pos[img]), base
            if step_index < int(first_pos[img]):
                gaps.append(float("inf"))
                continue
        if state.done[img] or is_first:
            gaps.append(float("inf"))             # (a first step keeps its row's `beam` picks as they are: nothing is ranked)
            continue
        scores = []
        for k in range(b):
            vb = float(state.vals[base + k])
            scores += [vb] if state.ended[base + k] else [vb + float(v) for v in vals64[base + k]]
        scores.sort(reverse=True)
        if len(scores) <= b or scores[b] == NEG:
            gaps.append(float("inf"))
        else:
            gaps.append(scores[b - 1] - scores[b])
    return gaps


def beam_search(logits_fn, n_img, beam, max_len, temperature=1.0, unk=1, eos=3, pad_index=0, len_bias_done=1, gaps=None):
    """The whole dense search: ``logits_fn(tokens int32 [rows, max_len], pos, rows_per_img) -> fp32 [rows, V]`` gives the logits of
    position ``pos`` for the first row of every image (``rows_per_img = 1``: the first step) or for every beam row.  A token per
    position ``0 .. max_len - 1`` (the engine skips the Transformer decoders' step at ``max_len``, which writes none);
    ``len_bias_done``: 1 for the LSTM decoders (a finished image's row keeps its last ``<eos>``), 0 for the Transformer decoders.  Returns ``finalize_best``'s dict and the OR of the
    rows' error bits; ``gaps`` (a list) collects ``(pos, candidate_gaps)``.  The row step's fp64 values are rounded to fp32 once,
    where the kernel stores them."""
    state = State(n_img, beam, max_len, pad_index=pad_index)
    err = 0
    for pos in range(max_len):
        first = pos == 0
        rows = state.tokens[::beam] if first else state.tokens
        logits = logits_fn(rows, pos, 1 if first else beam)
        picks, vals, errs = row_best(logits, temperature, beam, unk)
        for e in errs:
            err |= e
        if gaps is not None:
            gaps.append((pos, candidate_gaps(state, picks, vals, first)))
        select_best(state, picks, vals.to(torch.float32), first, pos, 0, pos, eos)
    return finalize_best(state, len_bias_done, max_len, pad_index, eos), err
