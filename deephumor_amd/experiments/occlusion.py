"""Occlusion maps of given captions: which image regions a caption's score rests on.

An attention map says where the decoder looked; it does not say what the score depends on -- a patch can carry weight and change
nothing, and three of the five kinds have no map.  Occlusion is the faithful answer: hide one region, score the same caption again,
report the log-probability lost.  Every (template, variant) is a pseudo-template of ``score_pairs``' pass machinery
(``scoring._score_feature_pairs``): the captions of a template meet its ``R + 1`` variants -- the unoccluded one and one per region --
in template-major passes."""
import numbers
from typing import NamedTuple, Optional

import torch

from .. import hip
from . import scoring
from .scoring import _check_explain_args, _score_feature_pairs


class OcclusionScores(NamedTuple):
    """What ``occlusion_maps`` returns for ``n`` captions of ``L`` positions and ``R`` regions.  Device tensors:

    ``base`` fp32 ``[n]``              caption ``i``'s log-probability under its unoccluded template: the fp64 sum of its fp32 per-token row
                                       (``explain_captions``' ``logprobs[i]``), rounded once -- ``score_pairs``' ``logprob[i, template_index[i]]``;
    ``drop`` fp32 ``[n, R]``           ``base - occluded``: the difference of the two fp64 sums, rounded once.  Positive: the region
                                       supports the caption;
    ``token_drop`` fp32 ``[n, L, R]``  or None: the same per token, exactly 0 at pads."""
    base: torch.Tensor
    drop: torch.Tensor
    token_drop: Optional[torch.Tensor] = None

    def map(self, fn):
        """``OcclusionScores`` of ``fn(field)`` for every field that is there (``clone``, ``cpu`` ...)."""
        return OcclusionScores(*(None if t is None else fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The captions of several results over the same regions, in order."""
        parts = list(parts)
        return OcclusionScores(*(None if ts[0] is None else torch.cat(ts, 0) for ts in zip(*parts)))


def region_edges(size, parts):
    """The ``parts + 1`` edges that cut ``size`` pixels into ``parts`` runs: run ``a`` is ``[a * size // parts, (a + 1) * size // parts)``
    -- never empty for ``1 <= parts <= size``, the runs differ by at most one pixel."""
    return [a * size // parts for a in range(parts + 1)]


def _check_occlusion_args(model, template_images, level, grid, fill, return_tokens):
    """The rules of the arguments ``occlusion_maps`` adds to ``explain_captions``' -> ``fill`` as a python list of one float per
    channel (``level="pixel"``; None otherwise)."""
    if level not in ("patch", "pixel"):
        raise ValueError(f"level must be 'patch' or 'pixel', got {level!r}")
    if not isinstance(return_tokens, bool):
        raise TypeError(f"return_tokens must be a bool, not {type(return_tokens).__name__}")
    dec = model.decoder
    if level == "patch":
        if not getattr(dec, "_cross", False):
            raise TypeError(f'level="patch": {type(model).__name__} has no encoder attention (only CaptioningTransformer and '
                            'CaptioningTransformerWithLabels attend over the image patches); level="pixel" works for every kind')
        if getattr(dec, "pad_index", 0) == 1:
            raise NotImplementedError('level="patch" with pad_index == 1: that decoder masks the real patch rows and attends over the '
                                      "padded ones (_forward_modules): a zeroed row is not a hidden patch there")
        if getattr(dec, "pad_index", 0) != 0:
            raise ValueError(f'level="patch": a decoder with pad_index = {dec.pad_index} masks no image key, so a zeroed row is not a '
                             'hidden patch; use level="pixel"')
        return None
    if not torch.is_tensor(template_images) or template_images.dim() != 4:
        raise ValueError('level="pixel": template_images must be a tensor [T, C, H, W]')
    c, h, w = template_images.shape[1:]
    ok = isinstance(grid, (tuple, list)) and len(grid) == 2 and all(isinstance(g, int) and not isinstance(g, bool) for g in grid)
    if not ok or not (1 <= grid[0] <= h and 1 <= grid[1] <= w):
        raise ValueError(f"grid must be two ints (gh, gw) with 1 <= gh <= {h} and 1 <= gw <= {w}, got {grid!r}")
    if torch.is_tensor(fill):
        fill = fill.detach().cpu().tolist()
    vals = [fill] * c if isinstance(fill, numbers.Real) and not isinstance(fill, bool) else fill
    if (not isinstance(vals, (tuple, list)) or len(vals) != c
            or not all(isinstance(v, numbers.Real) and not isinstance(v, bool) and v == v and abs(v) != float("inf") for v in vals)):
        raise ValueError(f"fill must be one finite real number or one per channel ({c}), got {fill!r}")
    return [float(v) for v in vals]


def occluded_images(image, grid, fill):
    """``image [C, H, W]`` -> ``[1 + gh * gw, C, H, W]``: the image itself, then one copy per region ``(a, b)`` (index ``a * gw + b``)
    with pixel rows ``[a * H // gh, (a + 1) * H // gh)`` and columns likewise set to ``fill`` (a list of one value per channel)."""
    gh, gw = grid
    c, h, w = image.shape
    ys, xs = region_edges(h, gh), region_edges(w, gw)
    out = image.unsqueeze(0).repeat(1 + gh * gw, 1, 1, 1)
    value = torch.tensor(fill, dtype=image.dtype, device=image.device).view(c, 1, 1)
    for a in range(gh):
        for b in range(gw):
            out[1 + a * gw + b, :, ys[a]:ys[a + 1], xs[b]:xs[b + 1]] = value
    return out


def occlusion_maps(model, template_images, template_index, captions, lengths, labels=None, batch_size=256, pad_index=0, level="patch",
                   grid=(7, 7), fill=0.0, return_tokens=False):
    """How much of each caption's log-probability rests on each image region: hide the region, score the same caption again, report
    what was lost -> ``OcclusionScores`` (``base [n]``, ``drop [n, R]``, ``token_drop [n, L, R]`` with ``return_tokens=True``).  Inputs
    and position convention are ``explain_captions``'.  ``attention_to_heatmaps(drop, grid=...)`` turns ``drop`` into images.

    ``level="patch"`` (the two kinds with encoder attention; ``TypeError`` otherwise, ``NotImplementedError`` for a ``pad_index == 1``
    decoder, ``ValueError`` for ``pad_index >= 2``, which masks nothing): ``R = S``, the rows of the encoder's spatial output (49 at
    224 x 224, row-major 7 x 7; ``S >= 2``).  The encoder runs once per distinct template.  Variant ``s`` is the template with row ``s``
    of its spatial features set to exactly 0 in the model's dtype -- by the model's own rule (a feature row that holds a zero is a
    masked key) the patch is hidden from every cross-attention.  The global feature / start embedding is NOT changed: this measures
    what the decoder's cross-attention draws from the patch, not what the pooled embedding carries of it.  A patch the model's rule
    masks already has ``drop == 0.0`` exactly.  ``grid`` and ``fill`` are ignored.

    ``level="pixel"`` (all five kinds): ``grid = (gh, gw)``, ``R = gh * gw``, region ``(a, b)`` has index ``a * gw + b`` and covers pixel
    rows ``[a * H // gh, (a + 1) * H // gh)`` and columns likewise; ``fill`` -- one real number, or one per channel -- is written into the
    region in the normalised input space (0 is the dataset mean).  The encoder runs on every distinct template's ``R + 1`` images in
    chunks of at most ``batch_size``; labels pass through unchanged.

    Each caption meets only the variants of its own template: captions are grouped by template, and a template's ``R + 1`` variants
    are the pseudo-templates of ``score_pairs``' template-major passes of at most ``batch_size`` sequences (apart from the results,
    memory is that of one pass plus one template's variants).  The occluded per-token row of (caption, region) is that of the single
    sequence on the zeroed features / the occluded image, bit for bit: it does not depend on ``batch_size``, ``n``, the order of the
    captions or the variants that share its pass.  ``base`` is ``score_pairs(...).logprob[i, template_index[i]]`` bit for bit.
    Arguments are validated before the encoder runs."""
    template_index, lengths = _check_explain_args(model, template_images, template_index, captions, lengths, batch_size, pad_index, False)
    fill = _check_occlusion_args(model, template_images, level, grid, fill, return_tokens)
    enc, dec = model.encoder, model.decoder
    n, l = captions.shape
    distinct, group = torch.unique(template_index.cpu(), return_inverse=True)
    with torch.no_grad():
        if level == "patch":
            pick = distinct.to(template_images.device)
            feats_all, spatial_all = enc(template_images[pick], labels[pick.to(labels.device)]) if labels is not None else enc(template_images[pick])
            s = spatial_all.shape[1]
            if s < 2:
                raise ValueError(f'level="patch" needs at least 2 patches, the encoder gave {s}')
            n_regions, dev = s, feats_all.device
            # variant 0 hides nothing, variant 1 + s hides row s
            hide = torch.cat([torch.zeros((1, s), dtype=torch.uint8, device=dev), torch.eye(s, dtype=torch.uint8, device=dev)])
            copy_keys = scoring._COPY_VARIANT_KEYS
            if copy_keys:
                # a template with at most one unmasked key has a variant without any: uniform attention over masked keys shows their K|V
                unmasked = s - hip.enc_key_mask(spatial_all.contiguous().view(-1, spatial_all.shape[-1])).view(-1, s).sum(1)
                copy_keys = int(unmasked.min()) >= 2
        else:
            n_regions, dev = grid[0] * grid[1], None
        base = drop = tokens = None
        for g in range(distinct.shape[0]):
            rows = (group == g).nonzero().squeeze(1)
            caps, lens = captions[rows.to(captions.device)], lengths[rows.to(lengths.device)]
            if level == "patch":
                feats, spatial = feats_all[g:g + 1].expand(n_regions + 1, -1), spatial_all[g:g + 1]
                res = _score_feature_pairs(dec, feats, spatial, caps, lens, batch_size, pad_index, hide=hide, detail=True, copy_keys=copy_keys)
            else:
                t = int(distinct[g])
                images = occluded_images(template_images[t], grid, fill)
                parts = []
                for lo in range(0, images.shape[0], batch_size):
                    chunk = images[lo:lo + batch_size]
                    parts.append(enc(chunk, labels[t:t + 1].repeat(chunk.shape[0], 1)) if labels is not None else enc(chunk))
                if isinstance(parts[0], tuple):
                    feats, spatial = (torch.cat(ts, 0) for ts in zip(*parts))
                else:
                    feats, spatial = torch.cat(parts, 0), None
                res = _score_feature_pairs(dec, feats, spatial, caps, lens, batch_size, pad_index, detail=True)
            logprob, _, sums, token_rows = res
            if base is None:
                dev = logprob.device
                base = torch.empty((n,), dtype=torch.float32, device=dev)
                drop = torch.empty((n, n_regions), dtype=torch.float32, device=dev)
                tokens = torch.empty((n, l, n_regions), dtype=torch.float32, device=dev) if return_tokens else None
            rows = rows.to(dev)
            base[rows] = logprob[:, 0]
            drop[rows] = (sums[:, :1] - sums[:, 1:]).float()
            if return_tokens:                               # fp32 - fp32 in fp64 is exact: one rounding
                tokens[rows] = (token_rows[:, :1].double() - token_rows[:, 1:].double()).float().transpose(1, 2)
        return OcclusionScores(base, drop, tokens)
