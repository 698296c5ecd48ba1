"""Text occlusion of given captions: which words a caption's score rests on.

``occlusion_maps`` says which image regions the score depends on; nothing said it about the text -- which earlier words make the
punchline likely, which label word the caption leans on.  Three of the five kinds have no attention map, and none has one over its own
history.  Occlusion is the faithful answer here too: hide one word, score the same caption again, report the log-probability lost.
Both levels run on the teacher-forced pass ``explain_captions`` / ``score_pairs`` / ``occlusion_maps`` share (``scoring._pass_logprobs``):
no entry point, option or kernel of their own."""
from typing import NamedTuple, Optional

import torch

from ..data import SPECIAL_TOKENS
from ..models._f32x_guard import f32x_guarded
from ..models.encoders import _require_eval
from .scoring import _check_explain_args, _pass_logprobs, _score_feature_pairs


class TextOcclusionScores(NamedTuple):
    """What ``text_occlusion`` returns for ``n`` captions of ``L`` positions and ``R`` regions (``L - 1`` caption columns or ``l`` label
    columns).  Device tensors:

    ``base`` fp32 ``[n]``              caption ``i``'s log-probability with nothing hidden: the fp64 sum of its fp32 per-token row
                                       (``explain_captions``' ``logprobs[i]``), rounded once -- ``occlusion_maps``' ``base``;
    ``drop`` fp32 ``[n, R]``           ``base - occluded`` over the positions the hidden word can reach: the difference of the two fp64
                                       sums, rounded once.  Positive: the word supports what follows it.  Exactly 0 for a region that is
                                       not real (history level: a column at or behind the caption's ``<eos>``);
    ``token_drop`` fp32 ``[n, L, R]``  or None: the same per token, exactly 0 at pads and, history level, at every position ``p <= j``."""
    base: torch.Tensor
    drop: torch.Tensor
    token_drop: Optional[torch.Tensor] = None

    def map(self, fn):
        """``TextOcclusionScores`` of ``fn(field)`` for every field that is there (``clone``, ``cpu`` ...)."""
        return TextOcclusionScores(*(None if t is None else fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The captions of several results over the same regions, in order."""
        parts = list(parts)
        return TextOcclusionScores(*(None if ts[0] is None else torch.cat(ts, 0) for ts in zip(*parts)))


def _check_text_occlusion_args(model, captions, lengths, labels, pad_index, level, fill, return_tokens):
    """The rules of the arguments ``text_occlusion`` adds to ``explain_captions``' -> the fill token id."""
    if level not in ("history", "label"):
        raise ValueError(f"level must be 'history' or 'label', got {level!r}; image regions are occlusion_maps' levels ('patch', 'pixel')")
    if not isinstance(return_tokens, bool):
        raise TypeError(f"return_tokens must be a bool, not {type(return_tokens).__name__}")
    dec = model.decoder
    v = dec.classifier.out_features
    fill_id = pad_index if isinstance(fill, str) and fill == "pad" else fill
    if isinstance(fill_id, bool) or not isinstance(fill_id, int) or not 0 <= fill_id < v:
        raise ValueError(f'fill must be "pad" (the call\'s pad_index) or an int token id in [0, {v}) such as vocab.stoi["<unk>"], '
                         f"got {fill!r}")
    if level == "label":
        if not hasattr(model.encoder, "label_encoder"):
            raise TypeError(f'level="label": {type(model).__name__} takes no labels (only CaptioningLSTMWithLabels and '
                            'CaptioningTransformerWithLabels do); level="history" works for every kind')
        if labels is None:
            raise ValueError('level="label" needs labels int64 [T, l], one row per template; level="history" works without them')
        if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[1] < 1 or labels.dtype != torch.int64:
            raise ValueError('level="label": labels must be an int64 tensor [T, l] with l >= 1, one row per template')
        return fill_id
    if getattr(dec, "pad_index", 0) == 1:
        raise NotImplementedError('level="history" with pad_index == 1: that decoder\'s position 0 attends over every position, so hiding '
                                  'a later word changes earlier rows; level="label" and occlusion_maps(level="pixel") do not depend on it')
    if captions.shape[1] < 2:
        raise ValueError('level="history" needs captions of L >= 2 positions: with L = 1 a caption is only its <eos> and no word is in '
                         "front of it")
    if int(lengths.max()) > captions.shape[1]:                                  # (a region index past the last column otherwise)
        raise ValueError(f'level="history": lengths must be <= L = {captions.shape[1]}, the positions of captions (a caption\'s length '
                         f"counts its <eos>), got {int(lengths.max())}")
    return fill_id


def history_variants(captions, lengths, fill_id):
    """The sequences of ``level="history"`` for ``captions`` int64 ``[n, L]`` and ``lengths [n]``, caption-major: caption ``i``
    contributes its base sequence and then one variant per real region ``j = 0 .. lengths[i] - 2`` (the columns in front of its
    ``<eos>``) -- ``lengths[i]`` sequences, ``sum(lengths)`` in all -> ``(caption int64 [N], region int64 [N] (-1: the base), inputs
    int64 [N, L - 1])``.  A variant's inputs are ``captions[i, :-1]`` with column ``j`` replaced by ``fill_id``; the targets stay
    ``captions[i]``."""
    n = captions.shape[0]
    dev = captions.device
    lens = lengths.to(dev)
    caption = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    first = torch.cumsum(lens, 0) - lens                                        # where caption i's sequences start
    region = torch.arange(caption.shape[0], device=dev) - first[caption] - 1
    inputs = captions[caption, :-1].clone()
    rows = (region >= 0).nonzero().squeeze(1)
    inputs[rows, region[rows]] = fill_id
    return caption, region, inputs


def _encode_distinct(enc, template_images, labels, pick):
    """The encoder on the templates ``pick`` (distinct, sorted) -> ``(feats [G, D], spatial [G, S, D] or None)``."""
    images = template_images[pick.to(template_images.device)]
    feats = enc(images, labels[pick.to(labels.device)]) if labels is not None else enc(images)
    return feats if isinstance(feats, tuple) else (feats, None)


def _history_rows(model, template_images, template_index, captions, lengths, labels, batch_size, pad_index, fill_id):
    """The passes of ``level="history"`` -> ``(caption [N], region [N], rows fp32 [N, L])``: the per-token row of every sequence of
    ``history_variants`` against the ORIGINAL caption, exact zeros at its pads.  ``template_index`` / ``lengths``: as
    ``_check_explain_args`` returns them."""
    enc, dec = model.encoder, model.decoder
    distinct, group = torch.unique(template_index.cpu(), return_inverse=True)
    feats, spatial = _encode_distinct(enc, template_images, labels, distinct)
    dev = feats.device
    caps = captions.to(dev).contiguous()
    caption, region, inputs = history_variants(caps, lengths, fill_id)
    which = group.to(dev)[caption]                                              # the row of feats / spatial of every sequence
    rows = torch.empty((caption.shape[0], caps.shape[1]), dtype=torch.float32, device=dev)
    for lo in range(0, caption.shape[0], batch_size):
        hi = min(lo + batch_size, caption.shape[0])
        idx = which[lo:hi]
        tgt = caps[caption[lo:hi]]
        sp = None if spatial is None else spatial.index_select(0, idx)
        logp, _ = _pass_logprobs(dec, feats.index_select(0, idx), sp, tgt, inp=inputs[lo:hi].contiguous())
        rows[lo:hi] = logp.masked_fill(tgt == pad_index, 0.0)
    return caption, region, rows


def _history_level(model, template_images, template_index, captions, lengths, labels, batch_size, pad_index, fill_id, return_tokens):
    n, l = captions.shape
    caption, region, rows = _history_rows(model, template_images, template_index, captions, lengths, labels, batch_size, pad_index, fill_id)
    dev = rows.device
    is_base = region < 0
    base_rows = rows[is_base]                                                   # [n, L], caption order
    varied = torch.zeros((n, l - 1, l), dtype=torch.float32, device=dev)        # [n, R, L]; a region that is not real keeps zeros
    varied[caption[~is_base], region[~is_base]] = rows[~is_base]
    p = torch.arange(l, device=dev)
    j = torch.arange(l - 1, device=dev)
    lens = lengths.to(dev)
    # m[i, j, p]: region j is real for caption i (j <= lengths[i] - 2) and position p lies behind it, inside the caption
    m = (j[None, :, None] < p[None, None, :]) & (p[None, None, :] < lens[:, None, None]) & (j[None, :, None] <= lens[:, None, None] - 2)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    b = torch.where(m, base_rows[:, None, :], zero)
    v = torch.where(m, varied, zero)
    base = base_rows.sum(-1, dtype=torch.float64).float()
    drop = (b.sum(-1, dtype=torch.float64) - v.sum(-1, dtype=torch.float64)).float()
    tokens = None
    if return_tokens:                                                           # fp32 - fp32 in fp64 is exact: one rounding
        tokens = torch.where(m, (b.double() - v.double()).float(), zero).transpose(1, 2).contiguous()
    return TextOcclusionScores(base, drop, tokens)


def label_variants(label_row, fill_id):
    """``label_row`` int64 ``[l]`` -> ``[l + 1, l]``: the row itself, then one copy per column ``k`` with that column replaced by
    ``fill_id``."""
    l = label_row.shape[0]
    out = label_row.unsqueeze(0).repeat(l + 1, 1)
    k = torch.arange(l, device=label_row.device)
    out[1 + k, k] = fill_id
    return out


@f32x_guarded
def _combine_guarded(enc, image_emb, variants):
    """The encoder's own combine step under the range guard its ``forward`` runs it under."""
    return enc._combine(image_emb, variants)


def _label_level(model, template_images, template_index, captions, lengths, labels, batch_size, pad_index, fill_id, return_tokens):
    enc, dec = model.encoder, model.decoder
    n, l = captions.shape
    n_regions = labels.shape[1]
    distinct, group = torch.unique(template_index.cpu(), return_inverse=True)
    _require_eval(enc, enc.dropout.p)                                           # (the encoder's forward, whose steps run apart here)
    enc.label_encoder.check(labels)                                             # host sync in front of the trunk's launches
    out = enc.image_encoder(template_images[distinct.to(template_images.device)])      # the trunk: once per distinct template
    image_emb, spatial_all = out if isinstance(out, tuple) else (out, None)
    dev = image_emb.device
    base = drop = tokens = None
    for g in range(distinct.shape[0]):
        rows = (group == g).nonzero().squeeze(1)
        caps, lens = captions[rows.to(captions.device)], lengths[rows.to(lengths.device)]
        variants = label_variants(labels[int(distinct[g])].to(dev), fill_id)
        feats = _combine_guarded(enc, image_emb[g:g + 1].expand(n_regions + 1, -1), variants)
        spatial = None if spatial_all is None else spatial_all[g:g + 1].expand(n_regions + 1, -1, -1).contiguous()
        logprob, _, sums, token_rows = _score_feature_pairs(dec, feats, spatial, caps, lens, batch_size, pad_index, detail=True)
        if base is None:
            base = torch.empty((n,), dtype=torch.float32, device=dev)
            drop = torch.empty((n, n_regions), dtype=torch.float32, device=dev)
            tokens = torch.empty((n, l, n_regions), dtype=torch.float32, device=dev) if return_tokens else None
        rows = rows.to(dev)
        base[rows] = logprob[:, 0]
        drop[rows] = (sums[:, :1] - sums[:, 1:]).float()
        if return_tokens:                                                       # fp32 - fp32 in fp64 is exact: one rounding
            tokens[rows] = (token_rows[:, :1].double() - token_rows[:, 1:].double()).float().transpose(1, 2)
    return TextOcclusionScores(base, drop, tokens)


def text_occlusion(model, template_images, template_index, captions, lengths, labels=None, batch_size=256, pad_index=0,
                   level="history", fill="pad", return_tokens=False):
    """How much of each caption's log-probability rests on each word: hide the word, score the same caption again, report what was
    lost -> ``TextOcclusionScores`` (``base [n]``, ``drop [n, R]``, ``token_drop [n, L, R]`` with ``return_tokens=True``).  Inputs and
    position convention are ``explain_captions``': output position ``p`` predicts ``captions[:, p]``, position 0 is the image slot, so
    caption column ``j`` is the decoder INPUT of position ``j + 1``.  ``occlusion_to_texts`` gives the readable form.

    ``fill``: what stands in for the hidden word -- ``"pad"`` (the call's ``pad_index``) or an int token id in ``[0, V)``, e.g.
    ``vocab.stoi['<unk>']`` = 1.  For the Transformer kinds a pad is a masked key, so ``"pad"`` is a clean removal: no later position
    attends to the slot.  For the LSTM kinds nothing is masked and the pad embedding is an untrained vector (the reference packs its
    sequences, so training never feeds it one): ``<unk>`` is the in-distribution choice there.

    ``level="history"`` (all five kinds; ``NotImplementedError`` for a ``pad_index == 1`` decoder, whose position 0 attends over every
    position; ``ValueError`` for ``L < 2`` or a length above ``L``): ``R = L - 1``, region ``j`` is caption column ``j`` as a decoder input.  It is real for
    caption ``i`` iff ``j <= lengths[i] - 2``, a token in front of the caption's ``<eos>``.  Variant ``(i, j)`` feeds the decoder
    ``captions[i, :-1]`` with column ``j`` replaced by the fill id; the TARGETS stay the original caption.  With ``b`` the base row,
    ``v`` the variant's fp32 per-token row and ``m[p] = 1`` for ``j < p < lengths[i]``: ``token_drop[i, p, j] = float32(float64(b[p])
    - float64(v[p]))`` where ``m[p]``, exactly 0.0 elsewhere -- positions ``p <= j`` cannot depend on a later input and are zero by
    definition, not by subtraction --, and ``drop[i, j] = float32(sum64(b * m) - sum64(v * m))``, exactly 0.0 for a region that is not
    real.  Only real variants are scored: the ``n`` base sequences and the ``sum(lengths - 1)`` variants are laid out caption-major
    (``history_variants``) and cut into passes of at most ``batch_size`` sequences, features gathered per sequence as
    ``explain_captions`` does; the encoder runs once per distinct template.

    ``level="label"`` (the two ``WithLabels`` kinds; ``TypeError`` otherwise, ``ValueError`` without ``labels``): ``R = l``, the label
    columns; variant ``k`` is the template's label row with column ``k`` replaced by the fill id.  The ResNet trunk runs once per
    distinct template; its start embedding goes through the encoder's own combine step for the ``l + 1`` label variants, spatial
    features are shared unchanged.  The variants are pseudo-templates of ``score_pairs``' template-major passes, as
    ``occlusion_maps(level="pixel")`` uses them; ``drop`` and ``token_drop`` are ``OcclusionScores``' definitions over all positions.
    The result is that of the full encoder run on the image repeated ``l + 1`` times with the variant labels, bit for bit.

    A variant's row is that of the single sequence, bit for bit: it does not depend on ``batch_size``, ``n``, the order of the captions
    or the sequences that share its pass.  ``base`` is ``score_pairs(...).logprob[i, template_index[i]]`` bit for bit.  Arguments are
    validated before the encoder runs."""
    template_index, lengths = _check_explain_args(model, template_images, template_index, captions, lengths, batch_size, pad_index, False)
    fill_id = _check_text_occlusion_args(model, captions, lengths, labels, pad_index, level, fill, return_tokens)
    run = _history_level if level == "history" else _label_level
    with torch.no_grad():
        return run(model, template_images, template_index, captions, lengths, labels, batch_size, pad_index, fill_id, return_tokens)


def occlusion_to_texts(tokens, scores, vocab):
    """The readable form of ``text_occlusion``'s ``drop``, the counterpart of ``token_scores``: for every caption a list of
    ``(token text, drop)``.  ``tokens`` int ``[n, >= R]``: the captions themselves (history level: the list covers a caption's real
    regions, its tokens up to but excluding ``<eos>``) or each caption's template label row, ``labels[template_index]`` (label level:
    every label column).  ``scores``: the ``TextOcclusionScores`` or its ``drop [n, R]``."""
    drop = scores.drop if isinstance(scores, TextOcclusionScores) else scores
    toks, drop = tokens.detach().cpu().tolist(), drop.detach().cpu().tolist()
    eos = vocab.stoi[SPECIAL_TOKENS['EOS']]
    out = []
    for row, vals in zip(toks, drop):
        items = []
        for tok, v in zip(row, vals):
            if tok == eos:
                break
            items.append((vocab.itos[tok], v))
        out.append(items)
    return out
