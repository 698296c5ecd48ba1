"""LSTM caption decoder on the gfx950 kernels.

Drop-in for ``deephumor.models.rnn_models.LSTMDecoder`` (reference rnn_models.py:8-143): same
constructor, ``forward(image_emb, captions, lengths)`` and ``generate(image_emb, caption, ...)``;
``generate_batch`` is the new batched entry point (the reference is strictly one image per call,
SURVEY.md section 2b).  One time step of one layer is ONE launch on the bf16 path (``dh_lstm_layer_fused``: the
[x | h_prev[beam parent]] operand gathered by the loader, gate GEMM on the matrix cores, cell update in the epilogue,
state ping-pong); on the fp32 parity path ``dh_lstm_prepare`` (state/embedding gather incl. beam reorder) + per layer
``dh_linear`` ([x|h] gate GEMM) + ``dh_lstm_cell``.  Both are sequenced by the native ``dh_lstm_decode_step``.
"""
import os

import torch
from torch import nn

from .. import hip
from ._f32x_guard import f32x_guarded
from .beam import BeamCaptions, DecodeSession, DecodeSettings, call_logits_hook, check_ids, check_lengths, classifier_must_be_finite, decode_with_overflow_retry, make_noise_source, run_interleaved, session_inputs
from .encoders import _Planned


class LSTMDecoder(_Planned, nn.Module):
    """LSTM-based decoder (reference rnn_models.py:8-26)."""

    def __init__(self, num_tokens, emb_dim=256, hidden_size=512,
                 num_layers=3, dropout=0.1, embedding=None):
        super().__init__()
        self.num_tokens = num_tokens
        self.embedding = embedding if embedding is not None else nn.Embedding(num_tokens, emb_dim)
        self.lstm = nn.LSTM(emb_dim, hidden_size, num_layers, batch_first=True,
                            dropout=(0 if num_layers == 1 else dropout))
        self.classifier = nn.Linear(hidden_size, num_tokens)

    # -- derived constants: [W_ih | W_hh] per layer and the summed bias -------------------------
    def _build_plan(self):
        layers = []
        # fp32 weights with option "f32_split": the gate products and the classifier as three fp16 MFMAs on split operands
        # (csrc/gemm_f32x.hip; dh_split_f32x planes of the weights, made here once per weight version)
        split = (self.classifier.weight.dtype == torch.float32 and self.classifier.weight.is_cuda and bool(hip.option("f32_split"))
                 and all(hip.f32_split_ok(p) for p in self.parameters() if p.dim() > 1))
        for l in range(self.lstm.num_layers):
            w = torch.cat([getattr(self.lstm, f"weight_ih_l{l}").detach(),
                           getattr(self.lstm, f"weight_hh_l{l}").detach()], dim=1).contiguous()
            b = (getattr(self.lstm, f"bias_ih_l{l}").detach().float()
                 + getattr(self.lstm, f"bias_hh_l{l}").detach().float()).contiguous()
            if w.dtype in hip.HALF_DTYPES:
                # gate-interleaved copy for the fused step kernel: row 4u+g = gate g (i, f, g, o) of hidden unit u
                hh = self.lstm.hidden_size
                w_il = w.view(4, hh, -1).permute(1, 0, 2).reshape(4 * hh, -1).contiguous()
                b_il = b.view(4, hh).t().reshape(-1).contiguous()
                # ... and that copy in MFMA fragment order for the register-stationary step (decode shapes)
                w_pk = hip.pack_mfma_fragments(w_il) if hip.lstm_layer_wreg_supported(w.shape[1] - hh, hh) else None
            else:
                w_il = b_il = w_pk = None
            w_x = hip.split_f32x(w) if split else None
            # ... and the split planes in MFMA fragment order: the gate product of a decode step with the weights stationary in registers
            w_xp = hip.pack_f32x_fragments(w_x) if (split and hip.option("decode_wreg")) else None
            layers.append((w, b, w_il, b_il, w_pk, w_x, w_xp))
        plan = dict(layers=layers, emb=self.embedding.weight.detach(),
                    cls_w=self.classifier.weight.detach(), cls_b=self.classifier.bias.detach().float().contiguous(),
                    dtype=self.classifier.weight.dtype)
        if split:
            plan["cls_w_x"] = hip.split_f32x(plan["cls_w"].contiguous())
            # the classifier on a split top-layer state (csrc/gemm_f32xp.hip) fills the beam sampler's group maxima like the 16-bit paths
            plan["f32_planes"] = bool(hip.option("f32_planes")) and self.lstm.hidden_size % 32 == 0
        if plan["dtype"] in hip.HALF_DTYPES and plan["cls_w"].is_cuda and plan["cls_w"].shape[1] == 512 and hip.option("vocab_wreg"):
            # the beam-search classifier with the weights streamed from L2 into registers (csrc/vocab_wreg.hip): padded, fragment-packed copy
            plan["cls_w_pk"], plan["cls_b_pad"] = hip.pack_vocab_weights(plan["cls_w"], plan["cls_b"])
        return plan

    def _check_mode(self):
        if self.training and self.lstm.dropout > 0:
            raise RuntimeError("deephumor_amd implements the inference path; call model.eval()")

    class _State:
        """Recurrent state of n_img*beam logical rows + per-step scratch (cached per row count), described to
        the native step driver (``dh_lstm_decode_step``) through plain C structs."""

        def __init__(self, dec, plan, n_img, beam, dev):
            self.nl, self.hh, self.e = dec.lstm.num_layers, dec.lstm.hidden_size, dec.lstm.input_size
            self.dev, self.dtype = dev, plan["dtype"]
            self.rows_total = r = n_img * beam
            # never read before it is written: the first step runs with started == 0 (zero state by flag)
            self.h = torch.empty((self.nl, r, self.hh), device=dev, dtype=self.dtype)
            self.c = torch.empty((self.nl, r, self.hh), device=dev)             # cell state always fp32
            self.started = 0                                                    # 0: zero state, then 1, 2, 1, 2, ...
            self._scratch = {}
            self.planes = bool(plan.get("f32_planes"))
            self.c_layers = (hip.LstmLayer * self.nl)()
            for i, (w, b, w_il, b_il, w_pk, w_x, w_xp) in enumerate(plan["layers"]):
                if w_x is not None:
                    self.c_layers[i].w_x = w_x.data_ptr()
                if w_xp is not None:
                    self.c_layers[i].w_xp = w_xp.data_ptr()
                self.c_layers[i].w, self.c_layers[i].b = w.data_ptr(), b.data_ptr()
                if w_il is not None:
                    self.c_layers[i].w_il, self.c_layers[i].b_il = w_il.data_ptr(), b_il.data_ptr()
                if w_pk is not None:
                    self.c_layers[i].w_pk = w_pk.data_ptr()
            m = self.c_model = hip.LstmModel()
            m.n_layers, m.E, m.Hh, m.V = self.nl, self.e, self.hh, dec.num_tokens
            m.dtype = {torch.float32: hip.F32, torch.bfloat16: hip.BF16, torch.float16: hip.F16}[self.dtype]
            m.layers = self.c_layers
            m.emb, m.cls_w, m.cls_b = plan["emb"].data_ptr(), plan["cls_w"].data_ptr(), plan["cls_b"].data_ptr()
            if "cls_w_pk" in plan:
                m.cls_w_pk, m.cls_b_pad = plan["cls_w_pk"].data_ptr(), plan["cls_b_pad"].data_ptr()
            if "cls_w_x" in plan:
                m.cls_w_x = plan["cls_w_x"].data_ptr()
            m.h, m.c = self.h.data_ptr(), self.c.data_ptr()
            if self.dtype in hip.HALF_DTYPES:     # fused step kernel: other workgroups still gather the old state rows
                self.h_alt, self.c_alt = torch.empty_like(self.h), torch.empty_like(self.c)
                m.h_alt, m.c_alt = self.h_alt.data_ptr(), self.c_alt.data_ptr()

        def scratch(self, rows):
            if rows not in self._scratch:
                nl, hh, e, dev, dt = self.nl, self.hh, self.e, self.dev, self.dtype
                bufs = dict(
                    xcat0=torch.empty((rows, e + hh), device=dev, dtype=dt),
                    xcatl=torch.empty((max(nl - 1, 1), rows, 2 * hh), device=dev, dtype=dt),
                    c_cur=torch.empty((nl, rows, hh), device=dev),
                    gates=torch.empty((rows, 4 * hh), device=dev),              # gate pre-activations fp32
                    hout=torch.empty((rows, hh), device=dev, dtype=dt))
                if self.planes:                        # fp32, split operands: the top layer's state as fp16 planes for the classifier
                    bufs["topp"] = torch.empty((2, rows, hh), device=dev, dtype=torch.float16)
                    bufs["xcat0p"] = torch.empty((2, rows, e + hh), device=dev, dtype=torch.float16)       # ... and of the gate GEMMs' operands
                    bufs["xcatlp"] = torch.empty((max(nl - 1, 1), 2, rows, 2 * hh), device=dev, dtype=torch.float16)
                c = hip.LstmScratch()
                for k, v in bufs.items():
                    setattr(c, k, v.data_ptr())
                bufs["c"] = c
                self._scratch[rows] = bufs
            return self._scratch[rows]

    def _step(self, plan, st, rows, rpi, mult, rows_total, img_emb=None, tokens=None, tok_pos=0, hparent=None,
              hout=None, logits=None, group_max=None):
        """One LSTM time step for ``rows`` compact rows (+ classifier if ``logits``): one native call."""
        sc = st.scratch(rows)
        hip.lstm_decode_step(st.c_model, sc["c"], img_emb, tokens, tok_pos, hparent, st.started, rows, rpi, mult,
                             rows_total, h_out=hout, logits=logits, group_max=group_max)
        st.started = 2 if st.started == 1 else 1
        return hout if hout is not None else sc["hout"]

    @f32x_guarded
    def forward(self, image_emb, captions, lengths=None):
        """Teacher-forced logits ``[bs, max(lengths), num_tokens]`` (reference rnn_models.py:28-46).
        Rows past ``lengths[i]`` are the packed-sequence zeros, i.e. the classifier bias."""
        hs, bs, steps_out = self.hidden_states(image_emb, captions, lengths)
        plan = self._get_plan()
        out = hip.linear(hs.view(bs * steps_out, -1), plan["cls_w"], plan["cls_b"], out_dtype=torch.float32, tag="vocab", w_x=plan.get("cls_w_x"))
        return out.view(bs, steps_out, -1)

    def hidden_states(self, image_emb, captions, lengths=None):
        """The top layer's hidden states ``[bs, max(lengths), hidden]`` in front of the classifier (zero past
        ``lengths[i]``, as ``pad_packed_sequence`` leaves them) -> ``(hs, bs, steps)``."""
        self._check_mode()
        plan = self._get_plan()
        bs, steps = captions.shape[0], captions.shape[1] + 1
        dev = image_emb.device
        if lengths is None:
            lengths = torch.full((bs,), steps, dtype=torch.long)
        lengths = torch.as_tensor(lengths).cpu()
        check_lengths(lengths, steps)                     # (pack_padded_sequence's errors)
        check_ids(captions, self.embedding.num_embeddings)
        steps_out = int(lengths.max())
        hh = self.lstm.hidden_size
        tokens = captions.to(torch.int32).contiguous()
        st = self._State(self, plan, bs, 1, dev)
        hs = torch.zeros((bs, steps_out, hh), device=dev, dtype=plan["dtype"])
        for t in range(steps_out):
            self._step(plan, st, bs, 1, 1, bs, img_emb=image_emb if t == 0 else None,
                       tokens=None if t == 0 else tokens, tok_pos=t - 1, hout=hs[:, t, :])
        valid = (torch.arange(steps_out)[None, :] < lengths[:, None]).to(dev)
        hs.mul_(valid[..., None])          # pad_packed_sequence zero rows (mask, not arithmetic on valid rows)
        return hs, bs, steps_out

    @f32x_guarded
    def generate_batch(self, image_emb, caption=None, max_len=25, temperature=1.0, beam_size=10, top_k=50,
                       eos_index=3, seed=None, img0=0, noise_source=None, logits_hook=None, streams=1, seed_tensor=None,
                       defer_check=False, early_stop_every=0, exact=False, rng=None, *, caption_lengths=None, return_beams=False, top_p=1.0,
                       no_repeat_ngram_size=0, repetition_penalty=1.0, **kw):
        """Batched beam-search sampling for ``image_emb [N, 1, E]`` or ``[N, E]``.

        Returns ``(tokens int64 [N, max_len] zero-padded, lengths int64 [N])``; row ``i`` equals what the reference's ``generate``
        returns for image ``i`` under the same random draws (rnn_models.py:48-143, incl. the hidden-state indexing at :135-137).

        The engine arguments.  ``streams`` > 1 decodes that many image sub-batches concurrently on separate HIP streams (same
        captions).  ``early_stop_every=k`` (> 0) checks every k steps whether every image has finished (the reference's
        ``all_ended()`` break, rnn_models.py:131) -- one host sync per check, same captions.  ``exact=True`` draws every row through
        the general sampler from the start (what a batch is repeated with automatically when flat logits overflow the pre-filtered
        samplers, see ``BeamOverflow``).  ``rng="torch"``: the draws consume torch CPU generators in the reference's order
        (``beam.TorchRngNoise``) -- on the fp32 path ``torch.manual_seed(s); decoder.generate(emb, rng="torch")`` returns the
        reference's sampled caption; in a batch image ``i`` replays ``torch.manual_seed(seed + img0 + i)``.  ``caption_lengths`` (int64
        / int32 ``[N]``, host or device): a prompt of its own length per image -- row ``i`` is teacher-forced with ``caption[i,
        :caption_lengths[i]]`` (0: none; the rest of the row is ignored) and equals row 0 of the dense call ``generate_batch(image_emb[i:i+1],
        caption=caption[i:i+1, :caption_lengths[i]], img0=img0 + i, ...)``; Philox noise only (``beam.prompt_session_inputs``).

        The decode settings, keyword only: the four named above and, in ``kw``, the rest of ``beam.DecodeSettings.names()`` -- any other
        keyword is a ``TypeError``.  Each is validated by its ``beam.check_*`` function before anything runs, and each one's default is
        the call without the keyword: same launches, same bits.  ``BeamSearchHelper`` has the full contract of every one:

        ``return_beams=True``          every beam the search ends with, a ``beam.BeamCaptions`` whose ``best()`` is the plain pair;
        ``top_p``                      nucleus filtering beside ``top_k`` (a number in ``(0, 1]``);
        ``no_repeat_ngram_size`` / ``repetition_penalty``   no n-gram twice in a row's history / CTRL's penalty on its tokens;
        ``min_len`` / ``bad_words_ids``  no ``<eos>`` before ``min_len`` / no last id of a listed phrase behind its other ids;
        ``sequence_bias``              ``{phrase: bias}``, added to the logit of a phrase's last id behind its other ids;
        ``search="beam"``              the deterministic search: the ``beam_size`` most likely continuations, no noise, scores that
                                       are cumulative model log-probabilities;
        ``length_penalty``             (``search="beam"``) candidates ranked by ``score * L ** -length_penalty``;
        ``early_stopping``             (``search="beam"``; ``True`` / ``False``) finished hypotheses go to a pool of ``beam_size``;
        ``num_beam_groups`` / ``diversity_penalty``   (``search="beam"``) diverse groups of beams;
        ``return_logprobs=True``       one more result, last: the model log-probability of every token written, ``[N, T]`` or
                                       ``[N, B, T]`` behind a ``BeamCaptions``."""
        return self._decode_session(image_emb, caption, max_len, temperature, beam_size, top_k, eos_index, seed, img0, noise_source,
                                    logits_hook, streams, seed_tensor, defer_check, early_stop_every, exact, rng, caption_lengths,
                                    return_beams=return_beams, top_p=top_p, no_repeat_ngram_size=no_repeat_ngram_size,
                                    repetition_penalty=repetition_penalty, **kw)

    def _decode_session(self, image_emb, caption, max_len, temperature, beam_size, top_k, eos_index, seed, img0, noise_source,
                        logits_hook, streams, seed_tensor, defer_check, early_stop_every, exact, rng, caption_lengths, **kw):
        """The implementation of ``generate_batch``: the engine arguments by name, the decode settings in ``kw``."""
        settings = DecodeSettings.from_call(kw, beam_size, max_len, self)
        return_beams = settings.return_beams
        self._check_mode()
        plan = self._get_plan()
        classifier_must_be_finite(plan)
        settings = settings.compiled(image_emb.device)                 # the two lists uploaded once (compiled ones: as they are)
        prompts, rng, noise_source, rng_seed, seed, rng_state0 = session_inputs(
            settings, caption, caption_lengths, max_len, self.embedding.num_embeddings, image_emb.device, seed, rng, noise_source, defer_check)
        image_emb = image_emb.reshape(image_emb.shape[0], -1).to(plan["dtype"]).contiguous()

        def new_helper(lo, hi, exact, **kw):
            return settings.new_helper(temperature=temperature, beam_size=beam_size, top_k=top_k, eos_index=eos_index,
                                       device=image_emb.device, n_img=hi - lo, seed=seed, img0=img0 + lo, seed_tensor=seed_tensor,
                                       exact=exact, **kw)

        def prompted_session(lo, hi, exact):
            """``session`` for a batch with ``caption_lengths``.  Slot ``s`` consumes the image (s = 0) or token ``s - 1`` and
            predicts token ``s``; image ``i`` makes its first draw at ``s = first_pos[i]``.  Slots below the shortest prompt run
            as the dense prefix does (one compact row per image); from there to the longest prompt all ``n * beam`` rows run and
            the prompted beam step sorts the images by phase (the rows of a still-forced image recompute copies of its base row,
            which ``hparent`` keeps them reading from); past the longest prompt it is the dense loop."""
            n, b = hi - lo, beam_size
            r = n * b
            ses = DecodeSession(new_helper(lo, hi, exact, max_len=max_len), plan, self.num_tokens, early_stop_every)
            ses.set_prompts(prompts, lo, hi)
            helper, logits, gmax = ses.helper, ses.logits, ses.group_max
            st = self._State(self, plan, n, b, image_emb.device)
            emb = image_emb[lo:hi]
            for s in range(ses.pmin):
                self._step(plan, st, n, 1, b, r, img_emb=emb if s == 0 else None, tokens=None if s == 0 else helper.tokens, tok_pos=s - 1)
            for s in range(ses.pmin, max_len):
                self._step(plan, st, r, b, 1, r, img_emb=emb if s == 0 else None, tokens=None if s == 0 else helper.tokens,
                           tok_pos=s - 1, hparent=helper.hparent, logits=logits, group_max=gmax)
                if logits_hook is not None:
                    call_logits_hook(logits_hook, s, logits, helper)
                if s <= ses.pmax:
                    helper.step_prompted(logits, write_pos=s, t=0, step_index=s, first_sets_ended=True, group_max=gmax)
                else:
                    helper.step(logits, first=False, write_pos=s, t=0, step_index=s, group_max=gmax)
                yield
                if ses.all_done(s):
                    break
            return helper.finalize(len_bias_done=1, full_len=max_len, defer_check=defer_check, beams=return_beams)

        def session(lo, hi, exact):
            if prompts is not None:
                return (yield from prompted_session(lo, hi, exact))
            n, b = hi - lo, beam_size
            r = n * b
            # a prefix of max_len or more tokens: the reference still makes its first draw and returns prefix + 1 tokens -- it never
            # truncates to max_len (rnn_models.py:97-101: the loop simply does not run); the token buffers are that wide then
            eff_len = max(max_len, (0 if caption is None else caption.shape[1]) + 1)
            noise = make_noise_source(rng, rng_seed, noise_source, lo, hi, img0, rng_state0)
            ses = DecodeSession(new_helper(lo, hi, exact, max_len=eff_len, noise_source=noise), plan, self.num_tokens, early_stop_every)
            pos = ses.set_prefix(caption, lo, hi)
            helper, logits, gmax = ses.helper, ses.logits, ses.group_max
            st = self._State(self, plan, n, b, image_emb.device)
            gm = None if gmax is None else gmax[:n]
            # image slot, then the teacher-forced prefix: one row per image living at logical row img*beam
            lg = logits[:n]
            self._step(plan, st, n, 1, b, r, img_emb=image_emb[lo:hi], logits=lg if pos == 0 else None,
                       group_max=gm if pos == 0 else None)
            for j in range(pos):
                last = j == pos - 1
                self._step(plan, st, n, 1, b, r, tokens=helper.tokens, tok_pos=j, logits=lg if last else None,
                           group_max=gm if last else None)
            if logits_hook is not None:
                call_logits_hook(logits_hook, pos, lg, helper)
            helper.step(lg, first=True, write_pos=pos, t=0, step_index=pos, first_sets_ended=True, group_max=gm)
            yield
            for i in range(pos + 1, max_len):
                self._step(plan, st, r, b, 1, r, tokens=helper.tokens, tok_pos=i - 1, hparent=helper.hparent,
                           logits=logits, group_max=gmax)
                if logits_hook is not None:
                    call_logits_hook(logits_hook, i, logits, helper)
                helper.step(logits, first=False, write_pos=i, t=0, step_index=i, group_max=gmax)
                yield
                if ses.all_done(i):
                    break
            # (no decode step when the prefix fills max_len - 1: the reference then returns beam 0 -- see finalize)
            return helper.finalize(len_bias_done=1, full_len=eff_len, defer_check=defer_check, first_beam=pos + 1 >= max_len,
                                   beams=return_beams, pos=pos)

        def run(exact):
            return run_interleaved(lambda lo, hi: session(lo, hi, exact), image_emb.shape[0], streams)
        return decode_with_overflow_retry(run, exact).public(return_beams)

    def generate(self, image_emb, caption=None, max_len=25,
                 temperature=1.0, beam_size=10, top_k=50, eos_index=3, **kw):
        """Single-image API of the reference (rnn_models.py:48-49): ``image_emb [1, 1, E]`` ->
        1-D int64 token tensor; with ``return_beams=True`` the image's ``BeamCaptions`` (``N = 1``, nothing squeezed).  ``top_p``,
        ``no_repeat_ngram_size``, ``repetition_penalty`` and every other decode setting (in ``kw``): see ``generate_batch``."""
        res = self.generate_batch(image_emb, caption=caption, max_len=max_len, temperature=temperature,
                                  beam_size=beam_size, top_k=top_k, eos_index=eos_index, **kw)
        return self.single_output(res, caption, max_len, beam_size)

    @staticmethod
    def single_output(res, caption, max_len, beam_size):
        """Row 0 of ``generate_batch``'s result in the shape the reference's single-image ``generate`` returns; a ``BeamCaptions``
        (``return_beams=True``) as it is, and so ``(BeamCaptions, logprobs [1, B, T])``.  ``return_logprobs=True`` without it: the pair
        ``(caption, logprobs [len])``."""
        if isinstance(res, BeamCaptions) or isinstance(res[0], BeamCaptions):
            return res
        if len(res) == 3:
            return LSTMDecoder.single_output(res[:2], caption, max_len, beam_size), res[2][0, :int(res[1][0])]
        toks, lens = res
        seq = toks[0, :int(lens[0])]
        if (0 if caption is None else caption.shape[1]) + 1 >= max_len:
            # no decode step ran: the reference indexes ``sample_seq`` with the [beam, 1] result of its final draw on the
            # [beam, 1] scores of the first step (rnn_models.py:140-141) and returns ``beam_size`` copies of beam 0's row
            seq = seq.unsqueeze(0).repeat(beam_size, 1)
        return seq.squeeze()
