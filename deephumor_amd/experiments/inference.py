"""Text <-> token helpers either side of the caption path.

Host-side string work with the behaviour of ``deephumor/experiments/inference.py:11-89``: the prompt prefix goes in
as token ids (``text_to_seq``), the generated ids come out as text (``seq_to_text``) and are cut into the meme's
top/bottom blocks (``split_caption``)."""
import re

import torch

from ..data import SPECIAL_TOKENS

# a space followed by a run of punctuation: the space is dropped when a block is cleaned (inference.py:8)
_SPACE_BEFORE_PUNCT = re.compile(r"( )([!#$%&\()*+,\-.\/:;<=>?@\\^{|}~]+)")
_SPECIAL = re.compile(r"<\w+>")


def text_to_seq(text, vocab, tokenizer):
    """``str`` -> int64 ``[1, seq_len]``: lower-case, tokenize, out-of-vocabulary tokens become ``<unk>``."""
    unk = vocab.stoi[SPECIAL_TOKENS['UNK']]
    ids = [vocab.stoi.get(tok, unk) for tok in tokenizer.tokenize(text.lower())]
    return torch.tensor(ids).unsqueeze(0)


def bad_words_to_ids(words, vocab, tokenizer):
    """Banned words or phrases as strings -> the id lists ``generate_batch(..., bad_words_ids=)`` takes.  Every string goes through
    ``text_to_seq`` (same lower-casing, same tokenizer); no ``<eos>`` is added.  A string with a token outside the vocabulary maps
    to ``<unk>`` there; it is skipped, with ONE warning for all of them, because ``<unk>`` is never drawn and such a phrase could
    never be completed.  An empty string is skipped too.

    What a match means depends on the tokenizer: with the word tokenizer a phrase matches whole tokens; with the CHARACTER
    tokenizer a phrase is a run of characters and matches as a SUBSTRING -- banning "ass" also bans "class"."""
    import warnings
    unk = vocab.stoi[SPECIAL_TOKENS['UNK']]
    out, skipped = [], []
    for word in words:
        ids = text_to_seq(word, vocab, tokenizer)[0].tolist() if word else []
        if not ids:
            continue
        if unk in ids:
            skipped.append(word)
            continue
        out.append([int(t) for t in ids])
    if skipped:
        warnings.warn(f"bad_words_to_ids: {len(skipped)} of {len(list(words))} strings hold a token outside the vocabulary (<unk> is "
                      f"never drawn, nothing to ban) and are skipped: {skipped[:8]!r}", stacklevel=2)
    return out


def sequence_bias_from_words(word_bias, vocab, tokenizer):
    """Words or phrases with a bias each, ``{"cat": 4.0, "damn": -3.0}`` or a list of ``(string, bias)`` pairs -> the list of
    ``(token ids, bias)`` pairs ``generate_batch(..., sequence_bias=)`` takes, in the order given.  Every string goes through
    ``text_to_seq`` (same lower-casing, same tokenizer, as ``bad_words_to_ids``); no ``<eos>`` is added.  A string with a token
    outside the vocabulary maps to ``<unk>`` there; it is skipped, with ONE warning for all of them, because ``<unk>`` is never drawn
    and such a phrase could never be completed.  An empty string is skipped too.  The biases are passed on as they are
    (``beam.check_sequence_bias`` checks them with the call).

    What a MULTI-TOKEN phrase means: the bias lands on the phrase's LAST token, and only once the other tokens are in place --
    ``"hot dog": 5.0`` makes "dog" likelier behind "hot" and leaves "hot" alone (bias "hot" as well to steer a caption to the whole
    phrase).  With the CHARACTER tokenizer a word is a run of characters, so it is such a phrase, and it matches as a SUBSTRING:
    a bias on "cat" raises "t" behind "ca", inside "scatter" too."""
    import warnings
    unk = vocab.stoi[SPECIAL_TOKENS['UNK']]
    items = list(word_bias.items()) if hasattr(word_bias, "items") else list(word_bias)
    out, skipped = [], []
    for word, bias in items:
        ids = text_to_seq(word, vocab, tokenizer)[0].tolist() if word else []
        if not ids:
            continue
        if unk in ids:
            skipped.append(word)
            continue
        out.append((tuple(int(t) for t in ids), bias))
    if skipped:
        warnings.warn(f"sequence_bias_from_words: {len(skipped)} of {len(items)} strings hold a token outside the vocabulary (<unk> is "
                      f"never drawn, nothing to steer) and are skipped: {skipped[:8]!r}", stacklevel=2)
    return out


def prompts_to_batch(texts, vocab, tokenizer):
    """The host text step in front of ``generate_batch(..., caption=C, caption_lengths=L)``: one optional caption beginning per
    image -> ``(C int64 [N, P], L int64 [N])``.  Every text goes through ``text_to_seq``; a trailing ``<eos>`` is dropped, as the
    notebook's ``get_a_meme`` does with ``_preprocess_text(caption)[:-1]`` (deephumor_demo.ipynb: the prompt is a beginning, not
    a finished caption); ``None`` or ``''`` gives length 0 ("no prompt for this image"); rows are padded with ``<pad>`` to the
    longest prompt (``P`` may be 0)."""
    eos, pad = vocab.stoi[SPECIAL_TOKENS['EOS']], vocab.stoi[SPECIAL_TOKENS['PAD']]
    rows = []
    for text in texts:
        ids = text_to_seq(text, vocab, tokenizer)[0].tolist() if text else []
        if ids and ids[-1] == eos:
            ids = ids[:-1]
        rows.append(ids)
    lengths = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    width = max([len(r) for r in rows], default=0)
    caption = torch.full((len(rows), width), pad, dtype=torch.int64)
    for i, r in enumerate(rows):
        caption[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return caption, lengths


def seq_to_text(seq, vocab, delimiter=' '):
    """1-D token tensor -> text, cut before the first ``<eos>``."""
    ids = seq.detach().cpu().reshape(-1).tolist()
    eos = vocab.stoi[SPECIAL_TOKENS['EOS']]
    if eos in ids:
        ids = ids[:ids.index(eos)]
    return delimiter.join(vocab.itos[i] for i in ids)


def beams_to_texts(beams, vocab, delimiter=' '):
    """``BeamCaptions`` (``generate_batch(..., return_beams=True)``) -> for every image a list of ``(text, score)`` in slot order
    (best score first).  Every row is cut at its OWN length, then read by ``seq_to_text`` (which stops before ``<eos>``)."""
    toks, lens, scores = beams.tokens.cpu(), beams.lengths.cpu().tolist(), beams.scores.cpu().tolist()
    return [[(seq_to_text(toks[i, j, :lens[i][j]], vocab, delimiter), scores[i][j]) for j in range(toks.shape[1])]
            for i in range(toks.shape[0])]


def group_best(beams, num_beam_groups):
    """The best beam of every group of ``generate_batch(..., search="beam", num_beam_groups=G, diversity_penalty=lam,
    return_beams=True)``'s ``BeamCaptions``: the ``G`` DIFFERENT captions per image that diverse beam search is asked for.  Engine beam
    ``k`` belongs to group ``k // Bg``, ``Bg = B // G`` (``beams.beam_index``), and the slots are in score order, so a group's best
    beam is its first slot.  Returns a ``BeamCaptions`` with ``G`` slots per image, slot ``g`` group ``g``'s best -- ``tokens [N, G,
    T]``, ``lengths`` / ``scores`` / ``beam_index [N, G]``, ``drawn`` the group whose best is the plain call's caption,
    ``row_lengths`` as they were --, which ``beams_to_texts`` reads like any other (in GROUP order, not score order)."""
    from ..models.beam import BeamCaptions
    g = num_beam_groups
    n, b, t = beams.tokens.shape
    if isinstance(g, bool) or not isinstance(g, int) or g < 1 or b % g != 0:
        raise ValueError(f"num_beam_groups must be an int >= 1 that divides the {b} beams, got {g!r}")
    if bool((beams.beam_index < 0).any()):
        raise ValueError("group_best: a slot with beam_index -1 comes from an early_stopping pool and belongs to no group")
    dev = beams.tokens.device
    group = beams.beam_index // (b // g)                                         # [N, B]
    slots = torch.arange(b, device=dev)[None, None, :].expand(n, g, b)
    mine = group[:, None, :] == torch.arange(g, device=dev)[None, :, None]
    first = torch.where(mine, slots, torch.full((), b, device=dev)).min(-1).values  # [N, G]: every group holds Bg >= 1 beams
    take = lambda x: torch.gather(x, 1, first)
    tokens = torch.gather(beams.tokens, 1, first[:, :, None].expand(n, g, t))
    drawn = group[torch.arange(n, device=dev), beams.drawn]
    return BeamCaptions(tokens, take(beams.lengths), take(beams.scores), take(beams.beam_index), drawn, beams.row_lengths)


def rank_beams(model, inputs, beams, labels=None):
    """Ranks every image's candidates by MODEL probability: ``beams.scores`` cannot do that -- the search re-normalises them over
    the drawn candidates at every step (``log_softmax`` over each row's ``beam_size`` picks, reference beam.py:79), so they are not
    log-probabilities of the captions.  The ``N * B`` rows, each cut at its own length and padded with ``<pad>``, are scored
    teacher-forced by ``experiments.scoring.score_captions`` (``inputs``: the ``N`` images the beams were generated for, encoded
    once; ``template_index = repeat_interleave(arange(N), B)``; ``labels`` for the label models).
    Returns ``(order int64 [N, B], perplexity float32 [N, B])``: ``order[i]`` lists image ``i``'s slots by ascending perplexity
    (stable), ``perplexity[i, j]`` belongs to slot ``j``.
    This is a second decoder pass over all ``N * B`` captions and it scores the RAW model: every token of a row, prompt included,
    on the logits ``forward`` gives, at temperature 1.  ``beam_logprob_scores`` needs no pass -- it sums what
    ``return_logprobs=True`` recorded during the search -- and scores the rows the search saw: generated tokens only, at the call's
    temperature, behind ``logits_hook``, the history edits and the bans."""
    from .scoring import score_captions
    n, b, t = beams.tokens.shape
    pad = getattr(model.decoder, "pad_index", 0)
    dev = beams.tokens.device
    lens = beams.lengths.reshape(n * b)
    keep = torch.arange(t, device=dev)[None, :] < lens[:, None]
    rows = torch.where(keep, beams.tokens.reshape(n * b, t), torch.full((), pad, dtype=torch.int64, device=dev))
    index = torch.arange(n, device=dev).repeat_interleave(b)
    pp = score_captions(model, inputs, index, rows, lens, labels=labels, pad_index=pad).view(n, b)
    return torch.argsort(pp, dim=1, stable=True), pp


def beam_logprob_scores(beams, logprobs, length_normalize=False, first_pos=0):
    """Every candidate's model log-probability from ``generate_batch(..., return_beams=True, return_logprobs=True)``'s pair
    ``(beams, logprobs [N, B, T])``, without the second decoder pass of ``rank_beams``: fp32 ``[N, B]``, the sum of a beam's
    log-probabilities over its own columns (the columns below ``beams.lengths``; everything outside the generated ones is exactly 0),
    or with ``length_normalize`` their mean over the generated columns -- ``beams.lengths - first_pos``, ``first_pos`` the prefix
    length of the call (an int) or its ``caption_lengths`` (``[N]``).  ``argsort(..., descending=True)`` ranks the slots.  Under
    ``search="beam"`` the sums are ``beams.scores``.
    How it differs from ``rank_beams``: that one scores the raw model teacher-forced (``forward``'s logits at temperature 1, every
    token of the row); this one scores the EDITED rows the search drew from -- ``log_softmax(x / temperature)`` behind ``logits_hook``,
    ``no_repeat_ngram_size`` / ``repetition_penalty`` and ``min_len`` / ``bad_words_ids`` -- and only the generated tokens.  Without
    edits and at temperature 1 the two agree to the engine's logit parity."""
    n, b, t = logprobs.shape
    dev = logprobs.device
    lens = beams.lengths.to(dev)
    own = torch.arange(t, device=dev)[None, None, :] < lens[:, :, None]
    total = torch.where(own, logprobs.float(), torch.zeros((), device=dev)).sum(-1)
    if not length_normalize:
        return total
    first = torch.as_tensor(first_pos, device=dev).reshape(-1, 1)
    return total / (lens - first).clamp(min=1).float()


def attention_to_heatmaps(attention, size=(224, 224), grid=(7, 7)):
    """``generate_batch(..., return_attention=True)``'s maps as images: ``attention [..., S]`` (weights over the ``grid[0] * grid[1]``
    image patches in row-major order; keys beyond them -- the padded rows of a ``pad_index >= 2`` decoder -- are dropped) ->
    fp32 ``[..., H, W]`` by bilinear upsampling (``align_corners=False``: every patch spreads over its own ``H / 7 x W / 7`` cell and
    blends into its neighbours; for whole multiples of the grid the upsampled map has the patch map's mean).  A row that is all
    zero -- a column past the caption's length -- stays all zero.  Post-processing for display, on the tensor's own device.
    ``occlusion_maps``' ``drop [n, R]`` is such a tensor too (``R`` regions in row-major order): ``attention_to_heatmaps(drop,
    grid=(7, 7))`` for ``level="patch"`` at 224 x 224, ``grid=`` the call's own grid for ``level="pixel"`` -- the values are log-prob
    differences of either sign then, not weights, and are upsampled as they are."""
    gh, gw = grid
    if attention.shape[-1] < gh * gw:
        raise ValueError(f"attention has {attention.shape[-1]} keys, fewer than the {gh} x {gw} grid")
    lead = attention.shape[:-1]
    maps = attention[..., :gh * gw].float().reshape(-1, 1, gh, gw)
    out = torch.nn.functional.interpolate(maps, size=tuple(size), mode="bilinear", align_corners=False)
    return out.reshape(*lead, *size)


def _clean_block(block):
    block = _SPECIAL.sub('', block).strip(' \t\n\r\f\v')
    return _SPACE_BEFORE_PUNCT.sub(r'\2', block)


def split_caption(text, num_blocks=None):
    """Splits a caption at ``<sep>`` into cleaned blocks; pads with '' / truncates to ``num_blocks``."""
    blocks = [_clean_block(b) for b in text.split(SPECIAL_TOKENS['SEP'])]
    if num_blocks is None:
        return blocks
    return (blocks + [''] * max(0, num_blocks - len(blocks)))[:num_blocks]


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


_COEFF_CACHE = {}


def resize_coefficients(in_size, out_size):
    """Filter table of one axis of Pillow's antialiased BILINEAR resample (``precompute_coeffs`` + ``normalize_coeffs_8bpc``
    of Pillow's Resample.c): ``(bounds int32 [out, 2] = (first source index, count), weights int32 [out, ksize])`` with
    22-bit fixed-point weights.  Host-side double precision arithmetic, like Pillow's; a few KB per (in, out) pair."""
    import numpy as np
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale                                   # triangle filter of half-width 1, stretched when shrinking
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    weights = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        arg = (np.arange(n, dtype=np.float64) + lo - center + 0.5) / filterscale
        w = np.where(np.abs(arg) < 1.0, 1.0 - np.abs(arg), 0.0)
        if w.sum() != 0.0:
            w = w / w.sum()
        weights[xx, :n] = np.where(w < 0, -0.5 + w * (1 << 22), 0.5 + w * (1 << 22)).astype(np.int64)
        bounds[xx] = (lo, n)
    return bounds, weights


def _coeffs(in_size, out_size, dev):
    if in_size == out_size:
        return None
    key = (in_size, out_size, str(dev))
    if key not in _COEFF_CACHE:
        b, w = resize_coefficients(in_size, out_size)
        _COEFF_CACHE[key] = (torch.from_numpy(b).to(dev), torch.from_numpy(w).to(dev))
    return _COEFF_CACHE[key]


def resize_images(images_u8, size=(224, 224)):
    """Decoded RGB images uint8 ``[N, H, W, 3]`` on the GPU -> uint8 ``[N, size[0], size[1], 3]``: the notebook's
    ``transforms.Resize((224, 224))`` (deephumor_demo.ipynb:565; Pillow's antialiased bilinear resample) as device kernels,
    bit-identical to Pillow (``tests/golden/g9_resize.npz``)."""
    from .. import hip
    n, h, w, c = images_u8.shape
    return hip.resize_u8_hwc(images_u8.contiguous(), size[0], size[1], _coeffs(w, size[1], images_u8.device),
                             _coeffs(h, size[0], images_u8.device))


def preprocess_images(images_u8, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32):
    """The whole notebook transform (Resize -> ToTensor -> Normalize, deephumor_demo.ipynb:565-567) on device for a batch
    of equally sized decoded images uint8 ``[N, H, W, 3]``.  ``dtype=torch.float32``: the fp32 ``[N, 3, 224, 224]`` batch
    the reference's encoders take; ``torch.bfloat16`` / ``torch.float16``: the normalised batch already in the 16-bit
    channels-last ``[N, 224, 224, 8]`` layout the matrix-core stem convolution reads (normalise + pack fused, no fp32 tensor
    in front of conv1) -- ``ImageEncoder`` accepts it in place of the NCHW batch and gives identical features."""
    from .. import hip
    dev = images_u8.device
    x = resize_images(images_u8, size) if tuple(images_u8.shape[1:3]) != tuple(size) else images_u8.contiguous()
    m, s = torch.tensor(mean, dtype=torch.float32, device=dev), torch.tensor(std, dtype=torch.float32, device=dev)
    if dtype == torch.float32:
        return hip.normalize_u8_hwc(x, m, s)
    return hip.normalize_pack_u8(x, m, s, out_dtype=dtype)


def images_to_tensor(images_u8, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Decoded, already resized RGB images uint8 ``[N, H, W, 3]`` on the GPU -> the normalised fp32 ``[N, 3, H, W]``
    batch the encoders take: the notebook's ``ToTensor`` + ``Normalize`` (deephumor_demo.ipynb:565-567) as one
    device kernel."""
    from .. import hip
    dev = images_u8.device
    return hip.normalize_u8_hwc(images_u8.contiguous(), torch.tensor(mean, dtype=torch.float32, device=dev),
                                torch.tensor(std, dtype=torch.float32, device=dev))
