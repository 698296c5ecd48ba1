"""Teacher-forced scoring of (template, caption) pairs -- SURVEY.md section 8(f) rank 1.

The corpus has 300 template images and 900,000 captions (README.md:26,37): the ResNet-50 encoder output
depends on the template only, so it is computed ONCE per distinct template and gathered per caption;
the decoders then run their teacher-forced ``forward`` (same incremental engine as ``generate``) and the
perplexity kernels score every caption (call shape of trainer.py:63-81)."""
from typing import NamedTuple, Optional

import torch

from .. import hip
from ..data import SPECIAL_TOKENS
from ..models._f32x_guard import f32x_guarded
from ..models.beam import check_ids, check_return_attention
from .metrics import sequence_perplexity, sequence_perplexity_from_hidden


def score_captions(model, template_images, template_index, captions, lengths, labels=None, batch_size=256,
                   pad_index=0):
    """Per-caption perplexity ``[n]`` for ``captions`` int64 ``[n, L]`` (tokens + <eos>, padded with ``pad_index``,
    as ``MemeDataset``/``pad_collate`` produce them) of templates ``template_index`` int64 ``[n]`` into
    ``template_images`` ``[T, 3, H, W]``.  ``lengths`` ``[n]`` = non-pad tokens per caption (trainer.py:67).  Works for every captioning model of this package;
    label models additionally take ``labels`` int64 ``[T, l]`` (one label per template)."""
    enc = model.encoder
    with torch.no_grad():
        if labels is not None:
            feats = enc(template_images, labels)
        else:
            feats = enc(template_images)
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        out = []
        for lo in range(0, captions.shape[0], batch_size):
            hi = min(lo + batch_size, captions.shape[0])
            idx = template_index[lo:hi].to(feats.device)
            emb = feats.index_select(0, idx)
            tgt = captions[lo:hi]                       # tokens + <eos>, zero padded (datasets.py:72-79, no <bos>)
            inp = tgt[:, :-1]                           # trainer.py:69-73: model(images, captions[:, :-1], lengths)
            dec = model.decoder
            width = dec.classifier.in_features
            if feats.dtype in hip.HALF_DTYPES and width % 64 == 0 and width >= 128:       # dh_vocab_logprob's contract; else the logits route
                # bf16 path: hidden states -> fused classifier + log-softmax gather, the [rows, V] logits never exist
                if hasattr(dec, "lstm"):
                    hidden, _, _ = dec.hidden_states(emb, inp, None)
                else:
                    hidden = dec._forward(inp, None if spatial is None else spatial.index_select(0, idx), emb,
                                          num_positions=tgt.shape[1], return_hidden=True)
                plan = dec._get_plan()
                hidden = hidden[:, :tgt.shape[1]].contiguous()
                out.append(sequence_perplexity_from_hidden(hidden, plan["cls_w"], plan["cls_b"], tgt.contiguous(),
                                                           lengths[lo:hi], pad_index))
                continue
            if spatial is not None:
                logits = dec(inp, enc_out=spatial.index_select(0, idx), start_emb=emb, num_positions=tgt.shape[1])
            elif hasattr(dec, "lstm"):
                logits = dec(emb, inp, None)
            else:
                logits = dec(inp, start_emb=emb)
            # output position p (0 = image slot) predicts caption token p: pred[:, :max_len] (trainer.py:75)
            logits = logits[:, :tgt.shape[1]].contiguous()
            out.append(sequence_perplexity(logits, tgt.contiguous(), lengths[lo:hi], pad_index))
        return torch.cat(out)


class CaptionScores(NamedTuple):
    """What ``explain_captions`` returns for ``n`` captions of ``L`` positions.  Device tensors:

    ``logprobs`` fp32 ``[n, L]``      ``log_softmax(logits[i, p])[captions[i, p]]``, exactly 0.0 where ``captions[i, p]`` is the pad;
    ``perplexity`` fp32 ``[n]``       ``exp(-sum_p logprobs[i, p] / lengths[i])`` (``dh_seq_perplexity``), ``score_captions``' value;
    ``attention`` fp32 ``[n, L, S]``  or None: where position ``p`` looked -- the head-mean encoder-attention softmax of the last
                                      decoder layer over the ``S`` image patches; every real row sums to 1, pad rows are exactly 0."""
    logprobs: torch.Tensor
    perplexity: torch.Tensor
    attention: Optional[torch.Tensor] = None

    def map(self, fn):
        """``CaptionScores`` of ``fn(field)`` for every field that is there (``clone``, ``cpu`` ...)."""
        return CaptionScores(*(None if t is None else fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The captions of several results, in order."""
        parts = list(parts)
        return CaptionScores(*(None if ts[0] is None else torch.cat(ts, 0) for ts in zip(*parts)))


def _check_explain_args(model, template_images, template_index, captions, lengths, batch_size, pad_index, return_attention, pairs=False):
    """The argument rules of ``explain_captions``.  ``pairs`` (``score_pairs``): there is no ``template_index`` -- every caption meets
    every template -- and at least one template is asked for instead; -> ``(None, lengths)``."""
    check_return_attention(return_attention, model)
    if pairs and (not torch.is_tensor(template_images) or template_images.dim() < 1 or template_images.shape[0] < 1):
        raise ValueError("template_images must be a tensor [T, ...] with T >= 1 templates")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be an int >= 1, got {batch_size!r}")
    if isinstance(pad_index, bool) or not isinstance(pad_index, int):
        raise TypeError(f"pad_index must be an int, not {type(pad_index).__name__}")
    if not torch.is_tensor(captions) or captions.dim() != 2 or captions.dtype != torch.int64 or captions.shape[0] < 1 or captions.shape[1] < 1:
        raise ValueError("captions must be an int64 tensor [n, L] with n >= 1 and L >= 1 (tokens + <eos>, padded with pad_index)")
    n = captions.shape[0]
    lengths = torch.as_tensor(lengths)
    if tuple(lengths.shape) != (n,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
        raise ValueError(f"lengths must be an integer tensor of shape [{n}] (one per caption), got {tuple(lengths.shape)} {lengths.dtype}")
    if int(lengths.min()) < 1:
        raise ValueError("lengths must be >= 1 (a caption holds at least its <eos>)")
    if pairs:
        check_ids(captions, model.decoder.classifier.out_features)
        return None, lengths.long()
    template_index = torch.as_tensor(template_index)
    if tuple(template_index.shape) != (n,) or template_index.dtype.is_floating_point or template_index.dtype == torch.bool:
        raise ValueError(f"template_index must be an integer tensor of shape [{n}] (one per caption), got {tuple(template_index.shape)}")
    check_ids(template_index, template_images.shape[0])
    check_ids(captions, model.decoder.classifier.out_features)                # (nn.Embedding's IndexError)
    return template_index.long(), lengths.long()


def explain_captions(model, template_images, template_index, captions, lengths, labels=None, batch_size=256, pad_index=0,
                     return_attention=False):
    """``score_captions`` with the per-token values kept: for GIVEN captions (a corpus meme, a candidate being ranked) every token's
    model log-probability and, with ``return_attention=True``, the image map of every position -- what ``generate_batch(...,
    return_logprobs=True, return_attention=True)`` returns for the captions it writes.  Inputs and position convention are
    ``score_captions``': output position ``p`` predicts ``captions[:, p]``, position 0 is the image slot.  -> ``CaptionScores``.

    Routes of the log-probs, per batch of ``batch_size`` captions:
      16-bit model        ``score_captions``' launches (hidden states -> ``dh_vocab_logprob`` -> ``dh_seq_perplexity``): ``perplexity`` is
                          ``score_captions``' bit for bit;
      fp32, ``f32_split``  hidden states -> ``dh_vocab_logprob(DH_F32)`` on the plan's split classifier planes: no ``[rows, V]`` logits in
                          memory.  The stream's overflow word is read once per batch; a flagged batch (an activation outside the fp16
                          range) is repeated on the logits route with the option off, as ``f32x_guarded`` does;
      anything else       (option off, classifier width outside ``K % 64 == 0, K >= 128``, ``pad_index == 1``) the logits route:
                          ``forward`` then ``dh_token_logprob`` -- ``score_captions``' fp32 launches.
    A caption's values do not depend on ``batch_size`` or on the captions next to it.

    ``return_attention`` (a plain bool): only the kinds with encoder attention have maps (``TypeError`` otherwise, ``NotImplementedError``
    for a ``pad_index == 1`` decoder -- ``check_return_attention``).  ``S`` is the encoder's patch count, 49 at 224 x 224: the zero rows
    the reference pads the encoder output with are masked keys of weight exactly 0 and are not returned (a ``pad_index >= 2`` decoder
    masks nothing: once ``L`` exceeds the patch count its padded rows are real keys and ``S`` grows to ``L``).  Arguments are validated
    before the encoder runs."""
    template_index, lengths = _check_explain_args(model, template_images, template_index, captions, lengths, batch_size, pad_index,
                                                  return_attention)
    enc = model.encoder
    dec = model.decoder
    with torch.no_grad():
        feats = enc(template_images, labels) if labels is not None else enc(template_images)
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        dev = feats.device
        parts = []
        for lo in range(0, captions.shape[0], batch_size):
            hi = min(lo + batch_size, captions.shape[0])
            idx = template_index[lo:hi].to(dev)
            emb = feats.index_select(0, idx)
            sp = None if spatial is None else spatial.index_select(0, idx)
            tgt = captions[lo:hi].to(dev).contiguous()
            lens = lengths[lo:hi].to(dev)
            logp, attn = _pass_logprobs(dec, emb, sp, tgt, return_attention)
            pad = tgt == pad_index
            pp = hip.seq_perplexity(logp, tgt, lens, pad_index)
            if attn is not None:
                attn = attn[:, :tgt.shape[1]].masked_fill(pad[..., None], 0.0)
            parts.append(CaptionScores(logp.masked_fill(pad, 0.0), pp, attn))
        return CaptionScores.cat(parts)


def _pass_logits(dec, emb, sp, tgt, return_attention=False, inp=None, **kw):
    """The forward call of the logits route (``_pass_logprobs``, ``token_alternatives``): the decoder's own teacher-forced fp32 logits of
    the captions ``tgt`` int64 ``[bs, l]`` -> ``(logits [bs, l, V], attention [bs, >= l, S] or None)``.  Position ``p`` predicts
    ``tgt[:, p]``.  ``inp`` (``text_occlusion``): int64 ``[bs, l - 1]`` decoder inputs that differ from ``tgt[:, :-1]``.  ``kw``:
    ``_forward``'s ``enc_share`` / ``enc_hide``.  The rows are the classifier's own output, not a copy: their stride may exceed ``V``
    (``hip.linear`` pads large 16-bit logits rows to whole 64-column groups)."""
    if inp is None:
        inp = tgt[:, :-1]
    l = tgt.shape[1]
    attn = None
    if return_attention:
        logits, attn = f32x_guarded(lambda d: d._forward(inp, sp, emb, num_positions=l, return_attention=True, **kw))(dec)
    elif kw:
        logits = f32x_guarded(lambda d: d._forward(inp, sp, emb, num_positions=l, **kw))(dec)
    elif sp is not None:
        logits = dec(inp, enc_out=sp, start_emb=emb, num_positions=l)
    elif hasattr(dec, "lstm"):
        logits = dec(emb, inp, None)
    else:
        logits = dec(inp, start_emb=emb)
    return logits[:, :l], attn


def _pass_logprobs(dec, emb, sp, tgt, return_attention=False, share=1, hide=None, inp=None):
    """One decoder pass of ``explain_captions`` / ``score_pairs``, the one statement of their routes (``explain_captions``' docstring):
    start embeddings ``emb [bs, D]``, captions ``tgt`` int64 ``[bs, l]`` on the device -> ``(log-probs fp32 [bs, l], pads not yet
    zeroed; attention [bs, >= l, S] or None)``.  ``sp``: the spatial features of the two cross-attention kinds, ``[bs, S, D]`` -- or,
    with ``share > 1`` (``score_pairs``' template-major passes), ``[bs / share, S, D]``: image ``j`` serves sequences
    ``j * share .. (j + 1) * share - 1`` (``TransformerDecoder._forward``'s ``enc_share``).  ``hide`` (``occlusion_maps``): uint8
    ``[bs / share, S]`` -- ``sp`` then holds the base images whose variants the pass scores (``_forward``'s ``enc_hide``).  ``inp``
    (``text_occlusion``): int64 ``[bs, l - 1]`` -- what the decoder is fed when that is not ``tgt[:, :-1]``; the targets stay ``tgt``."""
    lstm = hasattr(dec, "lstm")
    dev = emb.device
    if inp is None:
        inp = tgt[:, :-1]
    bs, l = tgt.shape
    width = dec.classifier.in_features
    fused_ok = width % 64 == 0 and width >= 128                                  # dh_vocab_logprob's contract
    kw = dict(enc_share=share) if share > 1 else {}
    if hide is not None:
        kw["enc_hide"] = hide

    def hidden_route(split=False):
        attn = None
        if lstm:
            hidden, _, _ = dec.hidden_states(emb, inp, None)
        elif return_attention:
            hidden, attn = dec._forward(inp, sp, emb, num_positions=l, return_hidden=True, return_attention=True, **kw)
        else:
            hidden = dec._forward(inp, sp, emb, num_positions=l, return_hidden=True, **kw)
        plan = dec._get_plan()
        hidden = hidden[:, :l].contiguous()
        w_x = plan["cls_w_x"] if split else None
        logp = hip.vocab_logprob(hidden.reshape(bs * l, width), plan["cls_w"], plan["cls_b"], tgt.reshape(-1), w_x=w_x)
        return logp.view(bs, l), attn

    def logits_route():
        logits, attn = _pass_logits(dec, emb, sp, tgt, return_attention, inp=inp, **kw)
        logits = logits.contiguous()
        return hip.token_logprob(logits.reshape(bs * l, -1), tgt.reshape(-1)).view(bs, l), attn

    if emb.dtype in hip.HALF_DTYPES and fused_ok:
        return hidden_route()
    if (emb.dtype == torch.float32 and fused_ok and hip.option("f32_split") and getattr(dec, "pad_index", 0) != 1
            and not torch.cuda.is_current_stream_capturing() and "cls_w_x" in dec._get_plan()):
        logp, attn = hidden_route(split=True)
        with torch.cuda.device(dev):
            over = hip.f32x_take_overflow(dev)
        if over:                                                                 # an activation left the fp16 range: exact kernels
            with hip.option_scope(f32_split=0):
                logp, attn = logits_route()
        return logp, attn
    return logits_route()


class PairScores(NamedTuple):
    """What ``score_pairs`` returns for ``n`` captions and ``T`` templates.  Device tensors:

    ``logprob`` fp32 ``[n, T]``     ``log p(caption i | template t)``: the fp64 sum of the pair's per-token fp32 log-probs
                                    (``explain_captions``' ``logprobs`` row; pads contribute exactly 0), rounded once;
    ``perplexity`` fp32 ``[n, T]``  the pair's ``dh_seq_perplexity`` value, ``explain_captions``' bit for bit."""
    logprob: torch.Tensor
    perplexity: torch.Tensor

    def map(self, fn):
        """``PairScores`` of ``fn(field)`` (``clone``, ``cpu`` ...)."""
        return PairScores(*(fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The captions of several results over the same templates, in order."""
        return PairScores(*(torch.cat(ts, 0) for ts in zip(*list(parts))))


# Private switch between the two ways a cross-attention decoder gets a pass's template features (same bits either way):
# True   one K|V projection and one packed layout per template of the pass, shared by its captions (``_forward``'s ``enc_share``);
# False  the features gathered per pair, as ``explain_captions`` does.
# The route kept is the one ``tools/time_pairs.py`` measured faster (profiles/pairs/timing.txt); the tests reach the other through here.
_SHARE_TEMPLATE_KEYS = True


def score_pairs(model, template_images, captions, lengths, labels=None, batch_size=256, pad_index=0):
    """Every caption under every template: ``log p(caption i | template t)`` for ``captions`` int64 ``[n, L]`` and ``template_images``
    ``[T, 3, H, W]`` -> ``PairScores`` (``logprob``, ``perplexity``, fp32 ``[n, T]`` each).  Inputs and position convention are
    ``score_captions``' (``lengths [n]``, ``labels [T, l]`` for the label models; position ``p`` predicts ``captions[:, p]``, position 0
    is the image slot) without a ``template_index``.  ``rank_templates`` / ``rank_captions`` read the matrix.

    The encoder sees each template once.  The decoder runs in passes of at most ``batch_size`` (caption, template) sequences, laid out
    template-major -- sequence ``t' * n_c + c`` for the ``n_c`` captions and the templates of the pass --, so the rows of one template
    are contiguous and the two cross-attention kinds project and pack a template's keys once for all its captions.  Encoded features
    are gathered per pass: apart from the two ``[n, T]`` results, memory is that of one pass.  The routes of the log-probs are
    ``explain_captions``', per pass (one helper states them for both); a pair's two values are those of ``explain_captions`` on that
    single pair and do not depend on ``batch_size``, ``n``, ``T`` or the pairs that share its pass.  Arguments are validated before the
    encoder runs."""
    _, lengths = _check_explain_args(model, template_images, None, captions, lengths, batch_size, pad_index, False, pairs=True)
    enc = model.encoder
    dec = model.decoder
    with torch.no_grad():
        feats = enc(template_images, labels) if labels is not None else enc(template_images)
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        logprob, perplexity, _, _ = _score_feature_pairs(dec, feats, spatial, captions, lengths, batch_size, pad_index)
        return PairScores(logprob, perplexity)


# Private switch between the two ways ``occlusion_maps(level="patch")`` gives a pass the keys of a template's variants (same bits either
# way: a hidden row is a masked key of weight exactly 0):
# False  the variants' features with their rows zeroed, projected and packed per variant (``enc_share`` alone);
# True   one K|V projection and one packed layout for the template, copied on the device for the variants of the pass, the hidden rows
#        ORed onto the key mask (``_forward``'s ``enc_hide``).
# The route kept is the one ``tools/time_occlusion.py`` measured faster (profiles/occlusion/timing.txt: the copies and the mask algebra
# cost more than the 16 x smaller projection and pack save); the tests reach the other through here.
_COPY_VARIANT_KEYS = False


def _score_feature_pairs(dec, feats, spatial, captions, lengths, batch_size, pad_index, hide=None, detail=False, copy_keys=True):
    """``score_pairs`` behind the encoder: every caption of ``captions [n, L]`` under every row of the encoded features ``feats [T, D]``
    (``spatial [T, S, D]`` or None) in template-major passes of at most ``batch_size`` sequences -> ``(logprob fp32 [n, T], perplexity
    fp32 [n, T], sums, rows)``.  ``detail``: ``sums`` fp64 ``[n, T]``, the sums ``logprob`` rounds, and ``rows`` fp32 ``[n, T, L]``, the
    per-token log-probs with exact zeros at pads (None, None otherwise).
    ``hide`` (``occlusion_maps``, cross-attention kinds): uint8 ``[T, S]`` and ``spatial [1, S, D]`` -- the ``T`` feature rows are
    variants of ONE image, variant ``t`` being its spatial features with the rows flagged in ``hide[t]`` set to exactly 0.
    ``copy_keys=False``: the caller knows a variant without an unmasked key (its softmax is uniform and shows the zeroed rows' K|V),
    which only the zeroed features themselves get right."""
    dev = feats.device
    (n, l), t_all = captions.shape, feats.shape[0]
    caps, lens = captions.to(dev).contiguous(), lengths.to(dev)
    logprob = torch.empty((n, t_all), dtype=torch.float32, device=dev)
    perplexity = torch.empty((n, t_all), dtype=torch.float32, device=dev)
    sums = torch.empty((n, t_all), dtype=torch.float64, device=dev) if detail else None
    rows_out = torch.empty((n, t_all, l), dtype=torch.float32, device=dev) if detail else None
    for lo in range(0, n, batch_size):
        hi = min(lo + batch_size, n)
        nc = hi - lo
        per = min(max(1, batch_size // nc), t_all)                               # templates of a pass
        # template-major: sequence t' * nc + c.  The captions' side of a pass is the same for every pass of the chunk (a shorter
        # last pass takes a prefix of it)
        tgt_all, lens_all = caps[lo:hi].repeat(per, 1), lens[lo:hi].repeat(per)
        pad_all = tgt_all == pad_index
        for t0 in range(0, t_all, per):
            t1 = min(t0 + per, t_all)
            rows = (t1 - t0) * nc
            tgt = tgt_all[:rows]
            idx = torch.arange(t0, t1, device=dev).repeat_interleave(nc)
            emb = feats.index_select(0, idx)
            share = nc if _SHARE_TEMPLATE_KEYS and spatial is not None else 1
            if hide is not None:
                if _COPY_VARIANT_KEYS and copy_keys:
                    sp, flags = spatial, hide[t0:t1] if share > 1 else hide.index_select(0, idx)
                else:
                    sp, flags = spatial.expand(t1 - t0, -1, -1).masked_fill(hide[t0:t1].bool().unsqueeze(-1), 0.0), None
                    sp = sp if share > 1 else sp.repeat_interleave(nc, 0)
                logp, _ = _pass_logprobs(dec, emb, sp, tgt, share=share, hide=flags)
            else:
                sp = None if spatial is None else spatial[t0:t1] if share > 1 else spatial.index_select(0, idx)
                logp, _ = _pass_logprobs(dec, emb, sp, tgt, share=share)
            pp = hip.seq_perplexity(logp, tgt, lens_all[:rows], pad_index)
            zeroed = logp.masked_fill(pad_all[:rows], 0.0)
            total = zeroed.sum(-1, dtype=torch.float64)
            logprob[lo:hi, t0:t1] = total.float().view(t1 - t0, nc).t()
            perplexity[lo:hi, t0:t1] = pp.view(t1 - t0, nc).t()
            if detail:
                sums[lo:hi, t0:t1] = total.view(t1 - t0, nc).t()
                rows_out[lo:hi, t0:t1] = zeroed.view(t1 - t0, nc, l).transpose(0, 1)
    return logprob, perplexity, sums, rows_out


def token_scores(captions, scores, vocab):
    """The readable form of ``explain_captions``' log-probs, as ``beams_to_texts`` is for beams: for every caption a list of
    ``(token text, log-prob)`` up to and including its ``<eos>`` (the whole row without one; the pad never appears -- a row ends at its
    first pad).  ``scores``: the ``CaptionScores`` or its ``logprobs [n, L]``."""
    lp = scores.logprobs if isinstance(scores, CaptionScores) else scores
    toks, lp = captions.detach().cpu().tolist(), lp.detach().cpu().tolist()
    eos, pad = vocab.stoi[SPECIAL_TOKENS['EOS']], vocab.stoi[SPECIAL_TOKENS['PAD']]
    out = []
    for row, vals in zip(toks, lp):
        items = []
        for tok, v in zip(row, vals):
            if tok == pad:
                break
            items.append((vocab.itos[tok], v))
            if tok == eos:
                break
        out.append(items)
    return out
