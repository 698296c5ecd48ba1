"""Reading ``score_pairs``' matrix ``log p(caption i | template t)``: which template fits a text (``rank_templates``, with
``template_accuracy`` the top-k metric of template recommendation), and which candidate captions are specific to a template
(``rank_captions``).  Pure tensor functions on the matrix's own device: fp64 keys, stable sorts, no kernels.

Why ``rank_templates`` has no ``normalize``: for ONE caption, dividing by its length or subtracting its average-template likelihood
(PMI) changes every template's key by the same per-caption constant (a positive factor, an offset), so the order of the templates
cannot change.  Both matter only where captions are compared with each other: ``rank_captions``."""
import math
from typing import NamedTuple

import torch

from .scoring import PairScores


class TemplateRanks(NamedTuple):
    """``rank_templates``' result for ``n`` captions: ``index`` int64 ``[n, top]`` the templates, best first; ``score`` fp32 ``[n, top]``
    their keys ``logprob + log(prior)``; ``probability`` fp32 ``[n, top]`` the posterior over ALL ``T`` templates at those entries."""
    index: torch.Tensor
    score: torch.Tensor
    probability: torch.Tensor


class CaptionRanks(NamedTuple):
    """``rank_captions``' result for ``T`` templates: ``index`` int64 ``[T, top]`` the captions, best first; ``score`` fp32 ``[T, top]``."""
    index: torch.Tensor
    score: torch.Tensor


def _matrix(scores):
    lp = scores.logprob if isinstance(scores, PairScores) else scores
    if not torch.is_tensor(lp) or lp.dim() != 2 or not lp.dtype.is_floating_point or lp.shape[0] < 1 or lp.shape[1] < 1:
        raise ValueError("scores must be a PairScores or its logprob, a floating-point tensor [n, T] with n >= 1 and T >= 1")
    return lp


def _top(top, limit, what):
    if isinstance(top, bool) or not isinstance(top, int) or top < 1:
        raise ValueError(f"top must be an int >= 1, got {top!r}")
    if top > limit:
        raise ValueError(f"top = {top} exceeds the {limit} {what}")
    return top


def rank_templates(scores, top=5, prior=None):
    """For every caption its ``top`` best templates -> ``TemplateRanks``.  ``key = logprob + log(prior)`` in fp64: ``prior [T]`` is any
    positive weighting of the templates (their corpus frequencies, say), normalised to sum 1; ``None`` is the uniform one.  Largest key
    first, equal keys to the lower template index (a stable sort).  ``probability`` is the softmax of the key over all ``T`` templates:
    the posterior ``p(template | caption)`` under that prior."""
    lp = _matrix(scores)
    n, t = lp.shape
    top = _top(top, t, "templates")
    if prior is None:
        log_prior = torch.full((t,), -math.log(t), dtype=torch.float64, device=lp.device)
    else:
        prior = torch.as_tensor(prior).to(device=lp.device, dtype=torch.float64)
        if tuple(prior.shape) != (t,):
            raise ValueError(f"prior must have shape [{t}] (one weight per template), got {tuple(prior.shape)}")
        if not bool((torch.isfinite(prior) & (prior > 0)).all()):
            raise ValueError("prior must be positive and finite for every template")
        log_prior = (prior / prior.sum()).log()
    key = lp.double() + log_prior
    val, index = torch.sort(key, dim=1, descending=True, stable=True)
    prob = torch.softmax(key, dim=1).gather(1, index[:, :top])
    return TemplateRanks(index[:, :top].contiguous(), val[:, :top].float(), prob.float())


def rank_captions(scores, lengths, top=5, normalize=None):
    """For every template its ``top`` best candidate captions -> ``CaptionRanks``.  The key, in fp64:
      ``normalize=None``      ``logprob[i, t]``;
      ``"length"``            ``logprob[i, t] / lengths[i]``: per token, so that short captions do not win by being short;
      ``"pmi"``               ``logprob[i, t] - log mean_t' exp(logprob[i, t'])``: how much likelier the caption is under THIS template than
                              under the average one -- a caption that is likely everywhere scores 0 everywhere.
    Largest key first, equal keys to the lower caption index.  ``lengths [n]``: the captions' lengths, as ``score_pairs`` took them."""
    lp = _matrix(scores)
    n, t = lp.shape
    top = _top(top, n, "captions")
    if normalize not in (None, "length", "pmi"):
        raise ValueError(f"normalize must be None, 'length' or 'pmi', got {normalize!r}")
    lengths = torch.as_tensor(lengths)
    if tuple(lengths.shape) != (n,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool or int(lengths.min()) < 1:
        raise ValueError(f"lengths must be an integer tensor of shape [{n}] (one per caption) with every entry >= 1")
    key = lp.double()
    if normalize == "length":
        key = key / lengths.to(lp.device).double()[:, None]
    elif normalize == "pmi":
        key = key - (torch.logsumexp(key, dim=1, keepdim=True) - math.log(t))
    val, index = torch.sort(key, dim=0, descending=True, stable=True)
    return CaptionRanks(index[:top].t().contiguous(), val[:top].t().float().contiguous())


def template_accuracy(ranks, true_index, ks=(1, 5)):
    """Top-k template accuracy: for each ``k`` of ``ks`` the share of captions whose true template ``true_index[i]`` is among the first
    ``k`` ranks -> ``{k: float}``.  ``ranks``: the ``TemplateRanks`` or its ``index [n, top]``; every ``k`` must be within ``top``."""
    index = ranks.index if isinstance(ranks, TemplateRanks) else ranks
    if not torch.is_tensor(index) or index.dim() != 2 or index.shape[0] < 1:
        raise ValueError("ranks must be a TemplateRanks or its index, an integer tensor [n, top]")
    n, top = index.shape
    true_index = torch.as_tensor(true_index).to(index.device)
    if tuple(true_index.shape) != (n,) or true_index.dtype.is_floating_point or true_index.dtype == torch.bool:
        raise ValueError(f"true_index must be an integer tensor of shape [{n}] (one template per caption), got {tuple(true_index.shape)}")
    out = {}
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > top:
            raise ValueError(f"every k must be an int in 1 .. top = {top}, got {k!r}")
        out[k] = float((index[:, :k] == true_index[:, None]).any(1).double().mean())
    return out
