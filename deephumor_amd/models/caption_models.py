"""Image captioning models: encoder + decoder compositions on the gfx950 kernels.

Drop-in for ``deephumor.models.caption_models`` (reference caption_models.py:9-461): same class
names, constructor arguments, ``forward`` / ``generate`` / ``save`` / ``from_pretrained`` and
checkpoint format ``{'model': state_dict, 'hp': dict}``.  New: ``generate_batch`` (N images at a
time; the reference handles exactly one) and ``CaptioningTransformerWithLabels`` (BASELINE
config 5).
"""
import torch
from torch import nn

from .. import hip
from ._f32x_guard import f32x_guarded
from .beam import (BeamCaptions, BeamOverflow, BeamSearchHelper, DecodeSettings, check_ids, check_prompts, compile_length_weights, held_length_weights, prompts_need_philox,
                   resolve_seed, warn_overflow_retry)
from .encoders import ImageEncoder, ImageLabelEncoder, SpatialImageLabelEncoder, _Planned
from .rnn_models import LSTMDecoder
from .transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder


class _CaptioningBase(nn.Module):
    _GEN_KEYS = ("caption", "max_len", "temperature", "beam_size", "top_k", "eos_index")

    def __init_subclass__(cls, **kw):
        """Every model's ``forward`` / ``generate_batch`` is the OUTERMOST range-guarded call of the split-operand fp32 path
        (``_f32x_guard.f32x_guarded``: one host read of the stream's overflow word per call, with option ``f32_split`` only)."""
        super().__init_subclass__(**kw)
        for name in ("forward", "generate_batch"):
            if name in cls.__dict__:
                setattr(cls, name, f32x_guarded(cls.__dict__[name]))

    def save(self, ckpt_path):
        """Saves the model's state and hyperparameters (reference caption_models.py:76-81)."""
        torch.save({'model': self.state_dict(), 'hp': self._hp}, ckpt_path)

    @classmethod
    def from_pretrained(cls, ckpt_path):
        """Loads and builds the model from a checkpoint file (reference caption_models.py:83-98)."""
        ckpt = torch.load(ckpt_path, map_location='cpu')
        model = cls(**ckpt['hp'])
        model.load_state_dict(ckpt['model'])
        return model

    _one = staticmethod(_IncrementalDecoder._one)       # ``generate``'s result from ``generate_batch``'s for one image

    # ``generate_batch`` = ``decode(encode(...))``.  The two halves are exposed separately so that a serving loop can run
    # the encoder of batch i+1 on one HIP stream while batch i decodes on another (deephumor_amd/pipeline.py): the decode
    # positions are chains of small latency-bound launches that leave most CUs idle, the encoder is throughput-bound.
    def encode(self, *inputs):
        """Image (+ label) encoder -> tuple of feature tensors consumed by ``decode``."""
        raise NotImplementedError

    def decode(self, encoded, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50, eos_index=3, *,
               caption_lengths=None, **kw):
        """Batched beam-search decoding of ``encode``'s output -> ``(tokens [N, max_len], lengths [N])``, or with
        ``return_beams=True`` every beam of every image as a ``beam.BeamCaptions`` (``LSTMDecoder.generate_batch``).
        ``top_p``, ``no_repeat_ngram_size`` / ``repetition_penalty``, ``min_len`` / ``bad_words_ids`` (in ``kw``): see there.
        ``search="beam"`` (in ``kw``; default ``"sample"``, the call without it): the deterministic search -- the ``beam_size`` most
        likely continuations, the same caption on every call, ``BeamCaptions.scores`` that are model log-probabilities (see there).
        ``caption_lengths`` (keyword only, int64 / int32 ``[N]``): a prompt of its own length per image -- row ``i`` is
        teacher-forced with ``caption[i, :caption_lengths[i]]`` (0: none; the rest of the row is ignored) and equals the dense
        single-image call with that prompt and ``img0 + i`` (``LSTMDecoder.generate_batch``).
        ``return_attention=True`` (in ``kw``, a plain bool; ``CaptioningTransformer`` / ``CaptioningTransformerWithLabels`` only): one
        more result, an fp32 device tensor that says where the model looked for every token -- ``(tokens, lengths, attention
        [N, T, S])``, or ``(BeamCaptions, attention [N, B, T, S])`` with ``return_beams=True`` in ``BeamCaptions`` slot order; ``T`` the
        width of ``tokens``, ``S`` the number of encoder keys (49; ``max(49, max_len + 1)`` with ``pad_index >= 2``, whose padded
        rows are keys).  ``attention[i, (slot,) c]`` is the mean over heads of the LAST decoder layer's encoder-attention softmax
        (reference transformers.py:106-115) at decode position ``c`` -- the position whose logits token column ``c`` was drawn from
        (or teacher-forced past, for prompt columns) -- taken on the row that computed that position of this beam's history.  Rows
        ``c <`` the beam's own length (``BeamCaptions.lengths``; the drawn beam's for the plain call) are filled and sum to 1; every
        other element is exactly 0.  A masked key has weight exactly 0 unless every key is masked (uniform ``1 / S``).  It changes
        no token; the other kinds raise ``TypeError``, ``pad_index == 1`` ``NotImplementedError`` (``beam.check_return_attention``).
        ``return_logprobs=True`` (in ``kw``, a plain bool; every kind): one more result, last in the tuple (behind ``attention``), an
        fp32 device tensor that says how likely the model found every token it wrote -- ``(tokens, lengths, logprobs [N, T])``, or
        ``(BeamCaptions, logprobs [N, B, T])`` with ``return_beams=True``; ``log_softmax(logits / temperature)`` at the token, on the
        row it was taken from, behind the history edits and the bans and in front of the top-k / nucleus / ``<unk>`` filtering; filled
        from the first generated column up to the beam's own length, exactly 0 elsewhere (``LSTMDecoder.generate_batch`` has the full
        contract).  It changes no token; ``pad_index == 1`` raises ``NotImplementedError`` (``beam.check_return_logprobs``).
        ``length_penalty`` (in ``kw``, with ``search="beam"``; default 0.0, the call without it): the search ranks its candidates by the
        length-normalised ``score * L ** -length_penalty`` inside the pruning, ``L`` the generated length; ``BeamCaptions.scores`` are
        those keys (``LSTMDecoder.generate_batch`` has the full contract).
        ``early_stopping`` (in ``kw``, with ``search="beam"``; ``None``, the default, is the call without it): ``True`` / ``False`` keep a
        finished-hypothesis pool per image -- an ``<eos>`` candidate goes there and takes no beam slot -- and stop an image when the pool
        is full (``True``) or when no live beam can still enter it (``False``); the result's slots are the pool's, each with its own
        length; refused with ``return_attention`` / ``return_logprobs`` (``LSTMDecoder.generate_batch`` has the full contract).
        ``num_beam_groups`` / ``diversity_penalty`` (in ``kw``, with ``search="beam"``; 1 / 0.0, the defaults, are the call without them):
        diverse beam search -- the beams are ``num_beam_groups`` groups that choose one after the other at every position, a group's
        candidates losing ``diversity_penalty`` for every earlier group that took the same token there; scores stay model
        log-probabilities, ``beam_index // (beam_size // num_beam_groups)`` is a beam's group and ``experiments.group_best`` returns
        each group's best beam; refused with ``early_stopping`` (``LSTMDecoder.generate_batch`` has the full contract).
        ``sequence_bias`` (in ``kw``; ``None``, the default, is the call without it): a mapping ``{tuple of token ids: bias}`` or a list
        of ``(phrase, bias)`` pairs -- the bias is added to the logit of a phrase's last id wherever the phrase's other ids end the
        row's history, a single id everywhere: positive steers towards a token, negative away from it without forbidding it;
        ``experiments.sequence_bias_from_words`` makes one from strings; ``pad_index == 1`` raises ``NotImplementedError``
        (``LSTMDecoder.generate_batch`` has the full contract)."""
        if caption_lengths is not None:
            kw["caption_lengths"] = caption_lengths
        return self.decoder.generate_batch(*encoded, caption=caption, max_len=max_len, temperature=temperature,
                                           beam_size=beam_size, top_k=top_k, eos_index=eos_index, **kw)

    def _check_prompts(self, caption, caption_lengths, max_len, kw):
        """A prompted batch is validated BEFORE the encoder runs (``beam.check_prompts`` / ``prompt_session_inputs``: shapes, ranges,
        the options it cannot be combined with); ``defer_check`` callers (graph capture, the pipeline) with device-resident lengths
        have done so themselves.  So are the decode settings in ``kw`` (``beam.DecodeSettings``), for every batch."""
        settings = DecodeSettings.from_kw(kw, max_len, self._hp["num_tokens"], self)
        settings.call_kw(kw)                      # (a setting that is off is the call without the keyword -- also for the decoders that do not know it)
        if caption_lengths is None:
            return None
        if getattr(self.decoder, "pad_index", 0) == 1:
            raise NotImplementedError("caption_lengths with pad_index == 1: that decoder re-runs the whole sequence per token on the "
                                      "module path, which has no per-image prompt phase")
        if settings.search != "beam":     # (search="beam" draws nothing: rng / noise_source are accepted and unused)
            prompts_need_philox(kw.get("rng"), kw.get("noise_source"))
        lens = torch.as_tensor(caption_lengths)
        if not (lens.is_cuda and (kw.get("defer_check") or torch.cuda.is_current_stream_capturing())):
            return check_prompts(caption, lens, max_len, self._hp["num_tokens"])      # on the host from here on: the decoder's own
        return lens                                                                      # check reads no length back again

    def _plan_signature(self):
        """Identity of everything a captured graph holds raw pointers to or derives constants from: storage pointer and
        in-place version counter of every parameter and buffer of the model."""
        ts = list(self.parameters()) + list(self.buffers())
        return tuple(t.data_ptr() for t in ts), tuple(t._version for t in ts), hip.options_epoch

    MAX_GRAPHS = 4      # captured graphs kept per model (one per (input shapes, decode settings))

    @staticmethod
    def _graph_state(graph, static, scap, seed_t, out, sig, plans, slens, length_penalty=0.0, device="cuda", early_stopping=None,
                     num_beam_groups=1):
        """What ``generate_batch_graphed`` caches per captured graph: the graph, its static inputs, its outputs, the plan signature and
        everything the captured nodes point at that nothing else owns -- the weight plans and, last, the ``length_penalty`` weight
        tables the capture's sessions launched with (``beam.held_length_weights``; ``()`` without a penalty, the tables of ones under
        ``early_stopping`` or ``num_beam_groups > 1``)."""
        return (graph, static, scap, seed_t, out, sig, plans, slens,
                held_length_weights(length_penalty, device, early_stopping, num_beam_groups))

    def generate_batch_graphed(self, *inputs, seed=None, caption=None, caption_lengths=None, **kw):
        """``generate_batch`` replayed from a captured hipGraph (torch.cuda.CUDAGraph on ROCm).

        The whole pass -- encoder, every decode position (a chain of ~70 dependent launches per position for
        the Transformer), beam steps, final draw -- is captured once per (input shapes, decode settings) and then
        replayed with one host call; inputs are copied into the graph's static buffers and the seed is passed
        through a device-resident word the beam kernels XOR into their Philox key, so replays with different
        seeds give the captions eager mode gives.  Worth 2-4 % at 256 images (the chain is GPU-latency-bound,
        not host-bound); the graph keeps its activations / KV cache allocated.

        A captured graph holds raw pointers to the weights and to the tensors the plans derive from them (fused QKV
        matrices, folded BatchNorm vectors, repacked convolution weights): it is valid only for the weight versions it
        was captured with.  Every cached graph therefore records the models' plan signature and keeps the plans
        themselves alive; ``load_state_dict`` / ``.to()`` / in-place weight updates change the signature and the
        graph is re-captured instead of replayed against stale or freed memory.

        ``caption_lengths`` (a prompt of its own length per image, see ``decode``): the lengths live in a device tensor of the graph
        that is overwritten before every replay, like ``caption``, and are validated on the host first (``beam.check_prompts``).  NO
        function of the lengths enters the graph cache key -- only the fact that lengths were passed, next to ``caption``'s shape:
        the captured chain treats every position ``0 .. min(P, max_len - 2)`` as mixed (all ``N * beam`` rows, the prompted beam
        step), so one graph serves every set of lengths of that shape and returns what eager returns for them."""
        # Every decode setting rides in ``kw`` and so is part of the cache key below: the graph of each one lives beside the plain one of
        # the same shapes (other select / finalize nodes, or a node more per position), and a replay returns clones of every field.
        # ``call_kw``: a setting that is off is the call without the keyword -- the plain graph, not a second one.  What a session
        # would upload is uploaded HERE, in front of any capture (no host-to-device copy happens inside one): the two lists, whose
        # hashable compiled forms replace the raw nestings in ``kw`` -- in the key, and so kept alive for as long as the graph is
        # cached --, and the weight table the selects that rank by key read (of ones without a penalty), which the sessions then find
        # in ``compile_length_weights``' cache and the graph's state holds (``_graph_state``)
        settings = DecodeSettings.from_kw(kw, kw.get("max_len", 25), self._hp["num_tokens"], self)
        settings.call_kw(kw)
        compiled = settings.compiled(inputs[0].device)
        for name in ("bad_words_ids", "sequence_bias"):
            if name in kw:
                kw[name] = getattr(compiled, name)
        if settings.length_penalty != 0.0 or settings.early_stopping is not None or settings.num_beam_groups > 1:
            compile_length_weights(settings.length_penalty, kw.get("max_len", 25), inputs[0].device)
        if kw.get("rng") == "torch" and settings.search != "beam":      # host-generated noise (parity mode): nothing to replay
            return self.generate_batch(*inputs, caption=caption, seed=seed, caption_lengths=caption_lengths, **kw)
        if caption_lengths is not None:
            caption_lengths = self._check_prompts(caption, torch.as_tensor(caption_lengths).cpu(), kw.get("max_len", 25), kw)
            caption_lengths = caption_lengths.to(device=inputs[0].device, dtype=torch.int32)
            caption = caption.to(inputs[0].device)
        seed = 0 if settings.search == "beam" else resolve_seed(seed)     # (nothing is drawn there: the default generator is not read)
        # ids are looked up without bounds tests and nothing can be read back inside a capture: the caption prefix and integer inputs
        # (labels) are range-checked here, in front of the capture / replay (beam.check_ids: nn.Embedding's IndexError)
        dec = getattr(self, "decoder", None)
        emb = getattr(dec, "embedding", None) or getattr(dec, "tok_embedding", None)
        if emb is not None and caption_lengths is None:       # (a prompted batch: _check_prompts above looked at the used ids)
            check_ids(caption, emb.num_embeddings, capturing_ok=False)
        lab = getattr(getattr(self, "encoder", None), "label_encoder", None)
        if lab is not None:
            for t in inputs:
                if not t.is_floating_point() and t.dtype != torch.uint8:
                    check_ids(t, lab.embedding.num_embeddings, capturing_ok=False)
        key = (tuple((tuple(t.shape), t.dtype) for t in inputs), None if caption is None else tuple(caption.shape),
               tuple(sorted(kw.items())), next(self.parameters()).dtype, caption_lengths is not None)
        lens_kw = {} if caption_lengths is None else {"caption_lengths": caption_lengths}
        cache = self.__dict__.setdefault("_graphs", {})
        eager_keys = self.__dict__.setdefault("_graph_overflowed", {})       # key -> plan signature it overflowed with
        sig = self._plan_signature()
        if key in eager_keys and eager_keys[key] != sig:
            del eager_keys[key]           # other weights since: the graphed path gets another chance
        if key in eager_keys:             # this configuration overflowed the pre-filtered samplers before (flat logits): straight to
            return self.generate_batch(*inputs, caption=caption, seed=seed, exact=True, **lens_kw, **kw)     # the general sampler, eagerly
        state = cache.get(key)
        if state is not None and state[5] != sig:
            cache.clear()                                 # weights changed: every captured graph points at dead tensors
            state = None
        if state is None:
            static = [t.clone() for t in inputs]
            scap = None if caption is None else caption.clone()
            slens = None if caption_lengths is None else caption_lengths.clone()
            seed_t = torch.zeros(1, dtype=torch.int64, device=inputs[0].device)

            slens_kw = {} if slens is None else {"caption_lengths": slens}

            def run():
                return self.generate_batch(*static, caption=scap, seed=0, seed_tensor=seed_t, defer_check=True, **slens_kw, **kw)

            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side), torch.no_grad():
                run()                                     # builds the weight plans, grows the allocator
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # thread_local: HIP calls of OTHER threads must not invalidate the capture -- with a process group alive, c10d's watchdog thread
            # polls hipEventQuery every few hundred ms, and in the default (global) mode one such call inside the capture window fails
            # the capture ("operation not permitted when stream is capturing": 1 run in 25 of `bench.py --rccl-single`, round 5)
            with torch.no_grad(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = run()
            sig = self._plan_signature()                  # (the warm-up built the plans)
            plans = [m._get_plan() for m in self.modules() if isinstance(m, _Planned)]     # outlive the graph
            while len(cache) >= self.MAX_GRAPHS:          # every graph keeps its activations / KV cache allocated: oldest out
                cache.pop(next(iter(cache)))
            state = cache[key] = self._graph_state(graph, static, scap, seed_t, out, sig, plans, slens,
                                                   length_penalty=settings.length_penalty, device=inputs[0].device,
                                                   early_stopping=settings.early_stopping, num_beam_groups=settings.num_beam_groups)
        else:
            cache[key] = cache.pop(key)                   # most recently used last
        graph, static, scap, seed_t, out = state[:5]
        err = out[-1]
        for dst, src in zip(static, inputs):
            dst.copy_(src)
        if scap is not None:
            scap.copy_(caption)
        if state[7] is not None:
            state[7].copy_(caption_lengths)
        seed_t.fill_(int(seed))
        graph.replay()
        if next(self.parameters()).dtype == torch.float32 and hip.option("f32_split") and hip.f32x_take_overflow(inputs[0].device):
            # an activation left the fp16 range of the split-operand path inside the replayed graph: this batch eagerly (the guarded
            # generate_batch repeats itself on the exact-fp32 kernels)
            return self.generate_batch(*inputs, caption=caption, seed=seed, **lens_kw, **kw)
        try:
            BeamSearchHelper.raise_for(int(err.item()))
        except BeamOverflow:              # flat logits: the captured chain cannot switch samplers -- this batch (and, from now on, this
            warn_overflow_retry()         # configuration) eagerly through the general sampler
            eager_keys[key] = self._plan_signature()
            return self.generate_batch(*inputs, caption=caption, seed=seed, exact=True, **lens_kw, **kw)
        if isinstance(out[0], BeamCaptions):          # (BeamCaptions, [attention,] [logprobs,] error word): clones of every field
            beams = out[0].map(torch.Tensor.clone)
            return (beams, *(t.clone() for t in out[1:-1])) if len(out) > 2 else beams
        return tuple(t.clone() for t in out[:-1])     # (tokens, lengths, [attention,] [logprobs,] error word)


class CaptioningLSTM(_CaptioningBase):
    """LSTM-based image captioning model (reference caption_models.py:9-98)."""

    def __init__(self, num_tokens, emb_dim=256, hidden_size=512, num_layers=2,
                 enc_dropout=0.3, dec_dropout=0.1):
        super().__init__()
        self.encoder = ImageEncoder(emb_dim=emb_dim, dropout=enc_dropout)
        self.decoder = LSTMDecoder(num_tokens=num_tokens, emb_dim=emb_dim, hidden_size=hidden_size,
                                   num_layers=num_layers, dropout=dec_dropout)
        self._hp = {'num_tokens': num_tokens, 'emb_dim': emb_dim, 'hidden_size': hidden_size,
                    'num_layers': num_layers, 'enc_dropout': enc_dropout, 'dec_dropout': dec_dropout}

    def forward(self, images, captions, lengths=None):
        return self.decoder(self.encoder(images), captions, lengths)

    def encode(self, images):
        return (self.encoder(images),)

    def generate_batch(self, images, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, *, caption_lengths=None, **kw):
        caption_lengths = self._check_prompts(caption, caption_lengths, max_len, kw)
        return self.decode(self.encode(images), caption, max_len, temperature, beam_size, top_k, eos_index, caption_lengths=caption_lengths, **kw)

    def generate(self, image, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        return self.decoder.single_output(self.generate_batch(image, caption, max_len, temperature, beam_size, top_k, eos_index, **kw),
                                          caption, max_len, beam_size)


class CaptioningLSTMWithLabels(_CaptioningBase):
    """LSTM captioning model conditioned on image + text label (reference caption_models.py:101-195).
    The label encoder and the decoder share ONE embedding (caption_models.py:125)."""

    def __init__(self, num_tokens, emb_dim=256, hidden_size=512, num_layers=2,
                 enc_dropout=0.3, dec_dropout=0.1):
        super().__init__()
        self.encoder = ImageLabelEncoder(num_tokens=num_tokens, emb_dim=emb_dim, dropout=enc_dropout)
        self.decoder = LSTMDecoder(num_tokens=num_tokens, emb_dim=emb_dim, hidden_size=hidden_size,
                                   num_layers=num_layers, dropout=dec_dropout,
                                   embedding=self.encoder.label_encoder.embedding)
        self._hp = {'num_tokens': num_tokens, 'emb_dim': emb_dim, 'hidden_size': hidden_size,
                    'num_layers': num_layers, 'enc_dropout': enc_dropout, 'dec_dropout': dec_dropout}

    def forward(self, images, captions, lengths, labels):
        return self.decoder(self.encoder(images=images, labels=labels), captions, lengths)

    def encode(self, images, labels):
        return (self.encoder(images, labels),)

    def generate_batch(self, images, labels, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, *, caption_lengths=None, **kw):
        caption_lengths = self._check_prompts(caption, caption_lengths, max_len, kw)
        return self.decode(self.encode(images, labels), caption, max_len, temperature, beam_size, top_k, eos_index, caption_lengths=caption_lengths, **kw)

    def generate(self, image, label, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        return self.decoder.single_output(self.generate_batch(image, label, caption, max_len, temperature, beam_size, top_k,
                                                              eos_index, **kw), caption, max_len, beam_size)


class _TransformerHP:
    def _set_hp(self, num_tokens, hid_dim, n_layers, n_heads, pf_dim, enc_dropout, dec_dropout, pad_index, max_len):
        self._hp = {'num_tokens': num_tokens, 'hid_dim': hid_dim, 'n_layers': n_layers, 'n_heads': n_heads,
                    'pf_dim': pf_dim, 'enc_dropout': enc_dropout, 'dec_dropout': dec_dropout,
                    'pad_index': pad_index, 'max_len': max_len}


class CaptioningTransformerBase(_CaptioningBase, _TransformerHP):
    """Transformer captioning model without encoder attention (reference caption_models.py:198-327)."""

    def __init__(self, num_tokens, hid_dim=512, n_layers=6, n_heads=8, pf_dim=2048,
                 enc_dropout=0.3, dec_dropout=0.1, pad_index=0, max_len=128):
        super().__init__()
        self.encoder = ImageEncoder(emb_dim=hid_dim, dropout=enc_dropout, spatial_features=False)
        self.decoder = SelfAttentionTransformerDecoder(num_tokens=num_tokens, hid_dim=hid_dim, n_layers=n_layers,
                                                       n_heads=n_heads, pf_dim=pf_dim, dropout=dec_dropout,
                                                       pad_index=pad_index, max_len=max_len)
        self._set_hp(num_tokens, hid_dim, n_layers, n_heads, pf_dim, enc_dropout, dec_dropout, pad_index, max_len)

    def forward(self, images, captions, lengths=None):
        return self.decoder(captions, start_emb=self.encoder(images))

    def encode(self, images):
        return (self.encoder(images),)

    def generate_batch(self, images, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, *, caption_lengths=None, **kw):
        caption_lengths = self._check_prompts(caption, caption_lengths, max_len, kw)
        return self.decode(self.encode(images), caption, max_len, temperature, beam_size, top_k, eos_index, caption_lengths=caption_lengths, **kw)

    def generate(self, image, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        return self._one(self.generate_batch(image, caption, max_len, temperature, beam_size, top_k, eos_index, **kw))


class CaptioningTransformer(_CaptioningBase, _TransformerHP):
    """Transformer captioning model attending over the 7x7 spatial image features
    (reference caption_models.py:330-461)."""

    def __init__(self, num_tokens, hid_dim=512, n_layers=6, n_heads=8, pf_dim=2048,
                 enc_dropout=0.3, dec_dropout=0.1, pad_index=0, max_len=128):
        super().__init__()
        self.encoder = ImageEncoder(emb_dim=hid_dim, dropout=enc_dropout, spatial_features=True)
        self.decoder = TransformerDecoder(num_tokens=num_tokens, hid_dim=hid_dim, n_layers=n_layers,
                                          n_heads=n_heads, pf_dim=pf_dim, dropout=dec_dropout,
                                          pad_index=pad_index, max_len=max_len)
        self._set_hp(num_tokens, hid_dim, n_layers, n_heads, pf_dim, enc_dropout, dec_dropout, pad_index, max_len)

    def forward(self, images, captions, lengths=None):
        image_emb, image_spatial_emb = self.encoder(images)
        return self.decoder(captions, enc_out=image_spatial_emb, start_emb=image_emb)

    def encode(self, images):
        return tuple(self.encoder(images))                  # (image_emb, image_spatial_emb)

    def generate_batch(self, images, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, *, caption_lengths=None, **kw):
        caption_lengths = self._check_prompts(caption, caption_lengths, max_len, kw)
        return self.decode(self.encode(images), caption, max_len, temperature, beam_size, top_k, eos_index, caption_lengths=caption_lengths, **kw)

    def generate(self, image, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        return self._one(self.generate_batch(image, caption, max_len, temperature, beam_size, top_k, eos_index, **kw))


class CaptioningTransformerWithLabels(_CaptioningBase, _TransformerHP):
    """BASELINE config 5: ImageLabelEncoder (with spatial features) + CaptioningTransformer decoder.
    No reference class exists; composition defined in SURVEY.md 8(a) row A4 from reference parts."""

    def __init__(self, num_tokens, hid_dim=512, n_layers=6, n_heads=8, pf_dim=2048,
                 enc_dropout=0.3, dec_dropout=0.1, pad_index=0, max_len=128):
        super().__init__()
        self.encoder = SpatialImageLabelEncoder(num_tokens=num_tokens, emb_dim=hid_dim, dropout=enc_dropout)
        self.decoder = TransformerDecoder(num_tokens=num_tokens, hid_dim=hid_dim, n_layers=n_layers,
                                          n_heads=n_heads, pf_dim=pf_dim, dropout=dec_dropout,
                                          pad_index=pad_index, max_len=max_len)
        self._set_hp(num_tokens, hid_dim, n_layers, n_heads, pf_dim, enc_dropout, dec_dropout, pad_index, max_len)

    def forward(self, images, captions, lengths, labels):
        start, spatial = self.encoder(images, labels)
        return self.decoder(captions, enc_out=spatial, start_emb=start)

    def encode(self, images, labels):
        return tuple(self.encoder(images, labels))          # (start_emb, image_spatial_emb)

    def generate_batch(self, images, labels, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, *, caption_lengths=None, **kw):
        caption_lengths = self._check_prompts(caption, caption_lengths, max_len, kw)
        return self.decode(self.encode(images, labels), caption, max_len, temperature, beam_size, top_k, eos_index, caption_lengths=caption_lengths, **kw)

    def generate(self, image, label, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        return self._one(self.generate_batch(image, label, caption, max_len, temperature, beam_size, top_k,
                                              eos_index, **kw))
