"""``experiments.explain_captions`` without a GPU: the fp64 restatement of ``explain_ref`` against golden G25 (the real reference's
per-token log-probs and attention maps), the ``CaptionScores`` record, the argument checks (which run before the encoder), the
readable form ``token_scores`` and the fp32 argument contract of ``dh_vocab_logprob``.

Restatement against G25.  G25 holds fp64 log-softmax values of the reference's fp32 logits; the restatement runs the oracle's
fp32 encoder and then the decoder in fp64 (cross-attention kinds) or the oracle's fp32 decoder.  Two fp32 evaluations of logits
of magnitude <= 32 differ by a few ulps of 3.8e-6 per accumulation; the bound is 1e-4 for the log-probs and 1e-6 for the maps
(weights <= 0.07, energies of O(1): an fp32 softmax is within 1e-7 relative of fp64)."""
import ctypes

import numpy as np
import pytest
import torch

import attention_maps_ref as AR
import explain_ref as E
from helpers import synth_images
from oracle import ref_path as R

LOGP_RESTATEMENT_ATOL = 1e-4
MAPS_RESTATEMENT_ATOL = 1e-6


def build(kind):
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_state_dict
    model = getattr(M, kind)(**E.HP[kind]).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=E.SEED))
    return model


# ---- restatement against G25 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_restatement_matches_g25(kind):
    g = E.golden(kind)
    cap, lengths, index, labels = E.captions()
    assert int(g["seed"]) == E.SEED and np.array_equal(g["captions"], cap.numpy()) and np.array_equal(g["lengths"], lengths.numpy())
    assert np.array_equal(g["template_index"], index.numpy()) and np.array_equal(g["labels"], labels.numpy())
    assert bool((cap[torch.arange(7), lengths - 1] == E.EOS).all()) and int(lengths.min()) == 1 and int(lengths.max()) == E.L
    sd = {k: v.detach() for k, v in build(kind).state_dict().items()}
    hp = dict(pad_index=E.PAD, n_heads=E.HP[kind].get("n_heads", 0))
    with torch.no_grad():
        start, enc_out = R._encode(kind, sd, synth_images(E.N_TEMPLATES, seed=0), labels)
        if kind in E.CROSS_KINDS:
            maps, logits = AR.teacher_forced_maps(sd, start[index], enc_out[index], cap[:, :-1], E.PAD, hp["n_heads"], with_logits=True)
            want = E.caption_maps(torch.from_numpy(g["attention"]), cap)
            got = E.caption_maps(maps, cap)
            assert got.shape == (7, E.L, E.N_KEYS) and float((got - want).abs().max()) <= MAPS_RESTATEMENT_ATOL
            assert float((got[cap != E.PAD].sum(-1) - 1).abs().max()) < 1e-12 and bool((got[cap == E.PAD] == 0).all())
        elif "LSTM" in kind:
            logits = R.lstm_decoder_forward(sd, "decoder", start[index], cap[:, :-1], None)
        else:
            logits = R.transformer_forward(sd, "decoder", cap[:, :-1], None, start[index], E.PAD, hp["n_heads"])
    lp = E.token_logprobs(logits, cap)
    want = torch.from_numpy(g["logprobs"]).masked_fill(cap == E.PAD, 0.0)
    assert float((lp - want).abs().max()) <= LOGP_RESTATEMENT_ATOL
    pp = E.perplexity(lp, cap, lengths)
    assert torch.allclose(pp, torch.stack([(-lp[i, :n].sum() / n).exp() for i, n in enumerate(lengths.tolist())]), rtol=1e-12)


def test_head_mean_softmax_restates_the_masked_fill():
    g = torch.Generator().manual_seed(5)
    energy = torch.randn(2, 3, 4, 6, generator=g)
    masked = torch.zeros(2, 1, 1, 6, dtype=torch.bool)
    masked[0, ..., 4:] = True
    masked[1] = True                                                                 # every key masked: uniform, as masked_fill gives
    w = E.head_mean_softmax(energy, masked)
    assert w.shape == (2, 4, 6) and bool((w[0, :, 4:] == 0).all()) and torch.allclose(w.sum(-1), torch.ones(2, 4, dtype=torch.float64))
    assert torch.allclose(w[1], torch.full((4, 6), 1 / 6, dtype=torch.float64))
    assert torch.allclose(w[0, :, :4], torch.softmax(energy[0, :, :, :4].double(), -1).mean(0))


# ---- CaptionScores -----------------------------------------------------------------------------------------------------------------
def test_caption_scores_record():
    from deephumor_amd.experiments import CaptionScores
    a = CaptionScores(torch.zeros(2, 3), torch.ones(2), torch.full((2, 3, 49), 0.5))
    b = CaptionScores(torch.ones(1, 3), torch.zeros(1))
    assert a._fields == ("logprobs", "perplexity", "attention") and b.attention is None
    lp, pp, att = a
    assert lp is a.logprobs and pp is a.perplexity and att is a.attention
    d = a.map(lambda t: t.double())
    assert isinstance(d, CaptionScores) and all(t.dtype == torch.float64 for t in d)
    assert b.map(lambda t: t + 1).attention is None and float(b.map(lambda t: t + 1).perplexity) == 1.0
    c = CaptionScores.cat([a, a.map(lambda t: t + 1)])
    assert c.logprobs.shape == (4, 3) and c.perplexity.tolist() == [1, 1, 2, 2] and c.attention.shape == (4, 3, 49)
    assert CaptionScores.cat([b, b]).attention is None and CaptionScores.cat([b, b]).logprobs.shape == (2, 3)


# ---- validation, before the encoder runs -------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_encoder_runs(monkeypatch):
    from deephumor_amd.experiments import explain_captions
    cap, lengths, index, labels = E.captions()
    images = torch.zeros(E.N_TEMPLATES, 3, 8, 8)

    def boom(*a, **kw):
        raise AssertionError("the encoder ran")
    for kind in ("CaptioningTransformer", "CaptioningLSTM", "CaptioningTransformerBase"):
        model = build(kind)
        monkeypatch.setattr(model.encoder, "forward", boom)
        call = lambda **kw: explain_captions(model, kw.pop("images", images), kw.pop("index", index), kw.pop("cap", cap),      # noqa: E731
                                             kw.pop("lengths", lengths), **kw)
        with pytest.raises(TypeError, match="return_attention must be a bool, not int"):
            call(return_attention=1)
        bad = cap.clone()
        bad[1, 2] = E.V
        with pytest.raises(IndexError, match="index out of range in self"):
            call(cap=bad)
        bad[1, 2] = -1
        with pytest.raises(IndexError, match="index out of range in self"):
            call(cap=bad)
        with pytest.raises(IndexError, match="index out of range in self"):
            call(index=torch.tensor([0, 1, 2, 3, 0, 1, 1]))
        with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[7\]"):
            call(lengths=lengths[:6])
        with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[7\]"):
            call(lengths=lengths.float())
        with pytest.raises(ValueError, match="lengths must be >= 1"):
            call(lengths=lengths - 1)
        with pytest.raises(ValueError, match=r"template_index must be an integer tensor of shape \[7\]"):
            call(index=index[:3])
        with pytest.raises(ValueError, match="captions must be an int64 tensor"):
            call(cap=cap.int())
        with pytest.raises(ValueError, match="captions must be an int64 tensor"):
            call(cap=cap[0])
        with pytest.raises(ValueError, match="batch_size must be an int >= 1"):
            call(batch_size=0)
        if kind == "CaptioningTransformer":
            with pytest.raises(AssertionError, match="the encoder ran"):             # valid arguments reach it
                call(return_attention=True)
        else:
            with pytest.raises(TypeError, match=f"return_attention: {kind} has no encoder attention"):
                call(return_attention=True)
    import deephumor_amd.models as M
    model = M.CaptioningTransformer(**dict(E.HP["CaptioningTransformer"], pad_index=1)).eval()
    monkeypatch.setattr(model.encoder, "forward", boom)
    with pytest.raises(NotImplementedError, match="return_attention with pad_index == 1"):
        explain_captions(model, images, index, cap, lengths, return_attention=True)


# ---- token_scores -------------------------------------------------------------------------------------------------------------------
def test_token_scores_on_both_tokenizers():
    from deephumor_amd.data import SPECIAL_TOKENS, CharTokenizer, Vocab, WordPunctTokenizer
    from deephumor_amd.experiments import CaptionScores, text_to_seq, token_scores
    for tok, text, want in ((WordPunctTokenizer(), "one does not simply", ["one", "does", "not", "simply"]),
                            (CharTokenizer(), "why not", list("why not"))):
        vocab = Vocab(tok.tokenize("one does not simply walk why"))
        eos = vocab.stoi[SPECIAL_TOKENS["EOS"]]
        ids = text_to_seq(text, vocab, tok)[0].tolist()
        width = len(ids) + 3
        cap = torch.zeros((2, width), dtype=torch.int64)
        cap[0, :len(ids)] = torch.tensor(ids)
        cap[0, len(ids)] = eos
        cap[1, 0] = eos                                                               # a caption that is only <eos>
        lp = -torch.arange(2 * width, dtype=torch.float32).view(2, width)
        out = token_scores(cap, CaptionScores(lp, torch.ones(2)), vocab)
        assert [t for t, _ in out[0]] == want + ["<eos>"] and [v for _, v in out[0]] == lp[0, :len(ids) + 1].tolist()
        assert out[1] == [("<eos>", float(lp[1, 0]))]
        assert token_scores(cap, lp, vocab) == out                                    # the bare tensor is taken too
        full = torch.tensor([ids[:3]])                                                # no <eos>, no pad: the whole row
        assert [t for t, _ in token_scores(full, torch.zeros(1, 3), vocab)[0]] == want[:3]


def test_heatmaps_take_the_teacher_forced_tensor():
    from deephumor_amd.experiments import attention_to_heatmaps
    att = torch.zeros(7, E.L, 49)
    att[:, :3] = 1.0 / 49
    maps = attention_to_heatmaps(att, size=(14, 21))
    assert maps.shape == (7, E.L, 14, 21) and bool((maps[:, 3:] == 0).all())
    assert torch.allclose(maps[:, :3], torch.full((7, 3, 14, 21), 1.0 / 49))


# ---- dh_vocab_logprob(DH_F32): the argument checks ----------------------------------------------------------------------------------
def test_fp32_vocab_logprob_argument_contract():
    """Checked before any launch (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    from deephumor_amd import hip
    fn = hip.load().dh_vocab_logprob
    names = ["A", "lda", "W", "ldw", "bias", "targets", "logp", "group_max", "group_sum", "target_logit", "gm_ld", "M", "V", "K", "dtype",
             "stream"]
    #       A   lda  W   ldw  bias targets logp gmax gsum tgt gm_ld M  V    K    dtype   stream
    good = [64, 136, 64, 128, 64, 64, 64, 64, 64, 64, 16, 5, 1000, 128, hip.F32, None]

    def call(**over):
        a = list(good)
        for k, val in over.items():
            a[names.index(k)] = val
        return fn(*a)
    for over in (dict(A=None), dict(W=None), dict(targets=None), dict(logp=None), dict(group_max=None), dict(group_sum=None),
                 dict(target_logit=None), dict(gm_ld=15), dict(gm_ld=0), dict(M=0), dict(V=0), dict(K=0), dict(K=96, ldw=96, lda=96),
                 dict(K=160, ldw=160, lda=160), dict(lda=124), dict(lda=130), dict(ldw=96), dict(ldw=136), dict(A=68), dict(W=72)):
        assert call(**over) == 1, over
    assert ctypes.sizeof(ctypes.c_void_p) == 8
