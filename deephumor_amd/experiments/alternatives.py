"""What the model would rather have said: the most likely tokens at every position of GIVEN captions.

``explain_captions`` says how likely each token of a caption was; the question asked next about a low-scoring one is what the model
expected there instead -- the ``top_logprobs=k`` of the LLM APIs.  The pieces are launches the package already has: the decoder's own
teacher-forced fp32 logits (``scoring._pass_logits``, the forward call of ``explain_captions``' logits route) and ``dh_beam_row_best``,
the row step of ``search="beam"``, which leaves the ``beam`` largest columns of a row with their ``x / T - logsumexp(x / T)``.  Two
metrics come from the same data and belong beside perplexity: top-k token accuracy and calibration."""
import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from .. import hip
from ..data import SPECIAL_TOKENS
from ..models.beam import BeamSearchHelper
from .scoring import _check_explain_args, _pass_logits


class TokenAlternatives(NamedTuple):
    """What ``token_alternatives`` returns for ``n`` captions of ``L`` positions.  Device tensors:

    ``tokens`` int64 ``[n, L, top]``   the ``j``-th most likely token of position ``p``, most likely first; equal logits go to the lower id;
    ``logprobs`` fp32 ``[n, L, top]``  its ``log_softmax(logits[i, p] / temperature)``.  A slot behind the row's last finite column holds
                                       token 0 at ``-inf``;
    ``rank`` int64 ``[n, L]``          the slot ``j`` with ``tokens[i, p, j] == captions[i, p]``, -1 when the target is not among the ``top``.
    At a pad position: ``tokens`` -1, ``logprobs`` exactly 0.0, ``rank`` -1."""
    tokens: torch.Tensor
    logprobs: torch.Tensor
    rank: torch.Tensor

    def map(self, fn):
        """``TokenAlternatives`` of ``fn(field)`` (``clone``, ``cpu`` ...)."""
        return TokenAlternatives(*(fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The captions of several results with the same ``top``, in order."""
        return TokenAlternatives(*(torch.cat(ts, 0) for ts in zip(*list(parts))))


# Rows of a pass that one ``dh_beam_row_best`` launch sweeps: None, the whole pass in one launch.  A workgroup owns a row, so the cut
# changes no bit.  ``tools/time_alternatives.py`` measured chunks of 2,048 / 1,024 / 512 rows against it (profiles/alternatives/timing.txt)
# and reaches them through here: each was slower than the whole pass, by more than the spread between rounds.
_ROW_CHUNK = None


def _aligned_rows(logits):
    """``logits`` fp32 ``[rows, V]`` with every row on a 16-byte boundary.  ``dh_beam_row_best``'s sweep walks a row as up to 3 scalars in
    front of the first 16-byte boundary, then 16-byte loads: which lane adds which column to the ``logsumexp`` depends on where the row
    starts, and with ``V % 4 != 0`` in a dense buffer that is the row's index in the pass modulo 4 -- a caption's last bit would move
    with ``batch_size`` and with the captions in front of it.  The one route pinned here: every row starts on a boundary (the walk with
    no scalars in front).  Large 16-bit logits come padded that way from the classifier; the others are copied once into rows padded
    to a multiple of 4 columns (the pad columns are never read)."""
    rows, v = logits.shape
    if logits.stride(1) == 1 and logits.stride(0) % 4 == 0 and logits.data_ptr() % 16 == 0:
        return logits
    buf = torch.empty((rows, (v + 3) // 4 * 4), dtype=torch.float32, device=logits.device)
    buf[:, :v].copy_(logits)
    return buf[:, :v]


def _check_alternatives_args(model, top, temperature, unk_index):
    """The rules of the arguments ``token_alternatives`` adds to ``explain_captions``' -> ``(temperature as float, unk_index or -1)``."""
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= hip.MAX_BEAMS:
        raise ValueError(f"top must be an int with 1 <= top <= {hip.MAX_BEAMS}, got {top!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real) or not (0.0 < float(temperature) < math.inf):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if unk_index is None:
        return float(temperature), -1
    if isinstance(unk_index, bool) or not isinstance(unk_index, int):
        raise TypeError(f"unk_index must be None or an int, not {type(unk_index).__name__}")
    if not 0 <= unk_index < model.decoder.classifier.out_features:
        raise IndexError("index out of range in self")                            # (check_ids' / nn.Embedding's)
    return float(temperature), unk_index


def token_alternatives(model, template_images, template_index, captions, lengths, labels=None, batch_size=256, pad_index=0, top=5,
                       temperature=1.0, unk_index=None):
    """For GIVEN captions, the ``top`` most likely tokens of every position with their log-probabilities, and the rank of the token the
    caption holds there -> ``TokenAlternatives`` (``tokens`` int64 ``[n, L, top]``, ``logprobs`` fp32 ``[n, L, top]``, ``rank`` int64
    ``[n, L]``).  Inputs and position convention are ``explain_captions``': output position ``p`` predicts ``captions[:, p]``, position
    0 is the image slot, ``labels [T, l]`` for the label models; the encoder sees each template once.

    Per pass of ``batch_size`` captions: the decoder's own teacher-forced fp32 logits ``[bs, L, V]`` (``forward``, as ``explain_captions``'
    logits route calls it -- a 16-bit model's classifier writes fp32 logits too) and ONE ``dh_beam_row_best`` sweep of the ``bs * L``
    rows: per row the ``top`` columns with the largest logit, largest first, equal logits (``-0.0 == +0.0``) to the lower id, and their
    ``x / temperature - logsumexp(x / temperature)`` over every column.  ``unk_index``: an id that is never listed (its mass still
    counts in the ``logsumexp``; a target equal to it has rank -1); None excludes nothing.  The rank is found on the device among the
    ``top`` picks; where it is ``>= 0``, ``logprobs[i, p, rank[i, p]]`` IS the target's log-probability on this route
    (``explain_captions`` may take the fused route, whose values differ in the last bits).  A caption's values do not depend on
    ``batch_size``, ``n``, the order of the captions or its neighbours.

    The kernel's error word is read once per call: a NaN or ``+inf`` among a row's logits raises the ``RuntimeError`` that ``generate``
    raises for non-finite logits; a row with fewer than ``top`` finite columns is no error -- the slots behind them hold token 0 at
    ``-inf``.  ``top <= 64`` (``MAX_BEAMS``).  Arguments are validated before the encoder runs.

    Calling this at several ``temperature`` values and reading ``calibration_table``'s expected calibration error is the temperature
    fit of a model."""
    template_index, lengths = _check_explain_args(model, template_images, template_index, captions, lengths, batch_size, pad_index, False)
    temperature, unk = _check_alternatives_args(model, top, temperature, unk_index)
    enc, dec = model.encoder, model.decoder
    v = dec.classifier.out_features
    with torch.no_grad():
        feats = enc(template_images, labels) if labels is not None else enc(template_images)
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        dev = feats.device
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        parts = []
        for lo in range(0, captions.shape[0], batch_size):
            hi = min(lo + batch_size, captions.shape[0])
            idx = template_index[lo:hi].to(dev)
            emb = feats.index_select(0, idx)
            sp = None if spatial is None else spatial.index_select(0, idx)
            tgt = captions[lo:hi].to(dev).contiguous()
            bs, l = tgt.shape
            logits, _ = _pass_logits(dec, emb, sp, tgt)
            rows = bs * l
            logits = _aligned_rows(logits.reshape(rows, -1))                     # (a view of the classifier's output wherever one exists)
            pick_idx = torch.empty((rows, top), dtype=torch.int32, device=dev)
            pick_val = torch.empty((rows, top), dtype=torch.float32, device=dev)
            step = rows if _ROW_CHUNK is None else _ROW_CHUNK
            for r0 in range(0, rows, step):
                r1 = min(r0 + step, rows)
                hip.beam_row_best(logits[r0:r1], v, r1 - r0, 1, top, temperature, unk, 0, pick_idx[r0:r1], pick_val[r0:r1], err)
            pad = (tgt == pad_index).view(rows)
            toks = pick_idx.long()
            hit = (toks == tgt.view(rows, 1)) & (pick_val > -math.inf)            # (a dead slot's token 0 is no pick)
            rank = torch.where(hit.any(-1), hit.int().argmax(-1), torch.full((), -1, dtype=torch.int64, device=dev))
            parts.append(TokenAlternatives(toks.masked_fill(pad[:, None], -1).view(bs, l, top),
                                           pick_val.masked_fill(pad[:, None], 0.0).view(bs, l, top),
                                           rank.masked_fill(pad, -1).view(bs, l)))
        # ERR_TOO_FEW is informational (dead slots, as the header says); the two others raise generate's errors
        BeamSearchHelper.raise_for(int(err.item()) & (hip.ERR_NONFINITE | hip.ERR_ALL_FILTERED))
        return TokenAlternatives.cat(parts)


def _host(alts, captions):
    """``(tokens, logprobs, rank, captions)`` as numpy arrays on the host, shapes checked."""
    toks, lps, rank = (t.detach().cpu().numpy() for t in alts)
    caps = captions.detach().cpu().numpy()
    if toks.ndim != 3 or toks.shape != lps.shape or rank.shape != toks.shape[:2] or caps.shape != rank.shape:
        raise ValueError(f"alts [n, L, top] and captions [n, L] must describe the same captions, got {toks.shape}, {lps.shape}, "
                         f"{rank.shape} and {caps.shape}")
    return toks, lps, rank, caps


def alternatives_to_texts(alts, captions, vocab):
    """The readable form of ``token_alternatives``, the sibling of ``token_scores``: for every caption a list of ``(target text, rank,
    [(alternative text, log-prob), ...])`` up to and including its ``<eos>`` (the whole row without one; a row ends at its first pad).
    The alternatives come most likely first; a dead slot (``-inf``) is left out."""
    toks, lps, rank, caps = _host(alts, captions)
    eos, pad = vocab.stoi[SPECIAL_TOKENS['EOS']], vocab.stoi[SPECIAL_TOKENS['PAD']]
    out = []
    for i, row in enumerate(caps.tolist()):
        items = []
        for p, tok in enumerate(row):
            if tok == pad:
                break
            alt = [(vocab.itos[t], v) for t, v in zip(toks[i, p].tolist(), lps[i, p].tolist()) if t >= 0 and v > -math.inf]
            items.append((vocab.itos[tok], int(rank[i, p]), alt))
            if tok == eos:
                break
        out.append(items)
    return out


def topk_accuracy(alts, captions, ks=(1, 5), pad_index=0):
    """Top-k token accuracy of given captions: ``{k: share of the non-pad positions with 0 <= rank < k}`` in fp64 (NaN without a
    non-pad position).  ``k`` must be an int with ``1 <= k <= top`` (``ValueError``): the rank is only known among the ``top`` picks."""
    toks, _, rank, caps = _host(alts, captions)
    top = toks.shape[2]
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= top:
            raise ValueError(f"every k must be an int with 1 <= k <= top = {top}, got {k!r}")
    real = caps != pad_index
    n = int(real.sum())
    r = rank[real]
    return {k: (float(((r >= 0) & (r < k)).sum()) / n if n else math.nan) for k in ks}


def calibration_table(alts, captions, bins=10, pad_index=0):
    """Calibration of the model's first choice over the non-pad positions: confidence ``exp(logprobs[..., 0])``, correct where ``rank ==
    0`` -> ``(table, ece)``: ``table`` a list of ``bins`` rows ``(count, mean confidence, accuracy)`` -- an empty bin is ``(0, 0.0, 0.0)``
    -- and ``ece`` the expected calibration error ``sum_b count_b / N * |accuracy_b - mean confidence_b|`` (NaN without a non-pad
    position).  fp64.  ``bins`` equal-width bins over [0, 1]: bin ``b`` holds ``b / bins <= confidence < (b + 1) / bins``, compared
    against the fp64 edges ``b / bins`` themselves; the right edge is closed only in the last bin (which also takes a confidence
    that rounding put above 1).

    ``token_alternatives`` at several ``temperature`` values, each read here, is the temperature fit: keep the one with the smallest
    ``ece``."""
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 1:
        raise ValueError(f"bins must be an int >= 1, got {bins!r}")
    _, lps, rank, caps = _host(alts, captions)
    real = caps != pad_index
    conf = np.exp(lps[..., 0].astype(np.float64))[real]
    correct = (rank[real] == 0).astype(np.float64)
    edges = np.arange(bins + 1, dtype=np.float64) / bins
    which = np.clip(np.searchsorted(edges, conf, side="right") - 1, 0, bins - 1)
    n = conf.shape[0]
    table, ece = [], 0.0 if n else math.nan
    for b in range(bins):
        sel = which == b
        count = int(sel.sum())
        if count == 0:
            table.append((0, 0.0, 0.0))
            continue
        mean_conf, acc = float(conf[sel].sum() / count), float(correct[sel].sum() / count)
        table.append((count, mean_conf, acc))
        ece += count / n * abs(acc - mean_conf)
    return table, ece
