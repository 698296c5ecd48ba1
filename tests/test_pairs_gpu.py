"""``experiments.score_pairs`` and the one-launch teacher-forced cross-attention on a real MI355X.

The shapes are the smallest where it can go wrong: ``explain_ref``'s tiny models, 4 templates (the fourth a second copy of the first),
the 7 captions of lengths 1 .. 9 with L = 9 (28 pairs: ``batch_size`` 5 cuts a pass inside the caption list, 1 gives a pass per pair,
256 one pass with 4 templates of 7 captions -- 63 query rows per template on the shared path, 3 full row blocks of 16 and one of 15).

What is equality here is asked as equality: a pair's ``perplexity`` against ``explain_captions`` on that single pair, every invariance,
the shared template keys against the gathered ones, a row of a long cross-attention call against the same row in a short one.
``logprob`` is the fp64 sum of the pair's fp32 log-probs rounded once; the test sums ``explain_captions``' row the same way and allows
1 fp32 ulp.  Kernel tolerances against fp64 are those of tests/test_prefill_gpu.py (``atol = 2e-5`` in fp32; 16-bit: its measured ulp
gates, 1.25 x 0.5001 / 0.5027 for the row kernels, 1.25 x 30.21 / 31.56 for the matrix-core form whose softmax weights are rounded to
the operand type).  Golden G26 gates are 4 x the worst value seen on an MI355X (``pairs_ref.WORST_*``, profiles/pairs/errors.txt).

What the launch spy can see: ``hip._launch`` records calls of the C entry points.  ``dh_attn_cross_prefill`` / ``_packed`` were one
CALL per layer before and after; the ``ceil(n_pos / 16)`` kernel launches the parent made were a host loop INSIDE the entry point,
which no Python-side recorder sees.  The spy therefore pins the calls (one per layer, with the image and row counts of the shared
path); that one call is one kernel launch is by construction (csrc/attention.hip has no loop left) and is what the equality of a
16-position call with the same rows inside a 63-position call exercises: those rows are row blocks 1 .. 3 of a single grid."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import explain_ref as E  # noqa: E402
import pairs_ref as P  # noqa: E402
from attn_ref import BF16, F16, F32, Gate as _Gate, attn_ref, rnd  # noqa: E402
from helpers import synth_images  # noqa: E402

# dtype settings: (id, dtype, options)
SETTINGS = (("f32_split", F32, dict(f32_split=1)), ("f32_exact", F32, dict(f32_split=0)), ("f16", F16, {}), ("bf16", BF16, {}))
SET_IDS = [s[0] for s in SETTINGS]
ULP_GATE = {"cross_prefill": {BF16: 1.25 * 0.5001, F16: 1.25 * 0.5027}, "cross_prefill_packed": {BF16: 1.25 * 30.21, F16: 1.25 * 31.56}}


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


_MODELS = {}


def build(kind, dt=F32):
    if (kind, dt) not in _MODELS:
        import deephumor_amd.models as M
        from deephumor_amd.synth import synth_state_dict
        model = getattr(M, kind)(**E.HP[kind]).eval()
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=E.SEED))
        _MODELS[(kind, dt)] = model.to(dt).cuda()
    return _MODELS[(kind, dt)]


@pytest.fixture(scope="module", autouse=True)
def drop_models():
    yield
    _MODELS.clear()


@pytest.fixture(scope="module")
def data():
    """(images [4, 3, 224, 224], captions [7, 9], lengths [7], labels [4, 3]) on the GPU."""
    return tuple(t.cuda() for t in P.inputs(synth_images(E.N_TEMPLATES, seed=0)))


def pairs(model, kind, data, dt, images=None, cap=None, lengths=None, labels=None, **kw):
    from deephumor_amd.experiments import score_pairs
    images = data[0] if images is None else images
    labels = data[3] if labels is None else labels
    return score_pairs(model, images.to(dt), data[1] if cap is None else cap, data[2] if lengths is None else lengths,
                       labels=labels if "WithLabels" in kind else None, **kw)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


class Spy:
    """The ``hip._launch`` recorder of tests/test_early_stopping_gpu.py: (name, args) of every native call."""

    def __init__(self, hip, monkeypatch):
        self.calls = []
        real = hip._launch

        def launch(name, *a, **k):
            self.calls.append((name, a))
            return real(name, *a, **k)
        monkeypatch.setattr(hip, "_launch", launch)

    def named(self, *names):
        return [a for n, a in self.calls if n in names]

    def clear(self):
        del self.calls[:]


# ---- 1. equality with the per-pair call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_every_pair_is_the_single_pair_call(hip, data, kind, setting):
    from deephumor_amd.experiments import explain_captions, rank_templates
    _, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, labels = data
    lab = labels if "WithLabels" in kind else None
    with hip.option_scope(**opts):
        got = pairs(model, kind, data, dt)
        assert got.logprob.shape == got.perplexity.shape == (7, 4) and got.logprob.dtype == got.perplexity.dtype == torch.float32
        worst_ulp = 0.0
        for t in range(4):
            for i in range(7):
                one = explain_captions(model, images.to(dt), torch.tensor([t], device="cuda"), cap[i:i + 1], lengths[i:i + 1], labels=lab)
                assert torch.equal(one.perplexity[0], got.perplexity[i, t]), (i, t, float(one.perplexity[0]), float(got.perplexity[i, t]))
                want = one.logprobs[0].double().sum()                                # pads are exactly 0 there
                worst_ulp = max(worst_ulp, P.ulps32(got.logprob[i, t].cpu().numpy(), want.cpu().numpy()))
    print(f"[pairs equality] {kind} {setting[0]}: logprob vs the summed single-pair row, worst {worst_ulp:.3f} fp32 ulp (bound 1)")
    assert worst_ulp <= 1.0
    assert bool((got.logprob < 0).all()) and bool(torch.isfinite(got.perplexity).all())
    assert torch.equal(got.logprob[:, 3], got.logprob[:, 0]) and torch.equal(got.perplexity[:, 3], got.perplexity[:, 0])   # the copy
    ranks = rank_templates(got, top=4)
    for row in ranks.index.tolist():
        assert row.index(0) + 1 == row.index(3)                                      # index 0 right before its copy, index 3


# ---- 2. invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_a_pair_does_not_depend_on_its_company(hip, data, kind, setting):
    _, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, labels = data
    with hip.option_scope(**opts):
        base = pairs(model, kind, data, dt)
        for bs in (1, 5):
            assert same(base, pairs(model, kind, data, dt, batch_size=bs)), bs       # (256 is the default: base)
        assert same(base, pairs(model, kind, data, dt, batch_size=256))
        rev = pairs(model, kind, data, dt, cap=cap.flip(0), lengths=lengths.flip(0))
        assert same(base, rev.map(lambda x: x.flip(0)))
        few = pairs(model, kind, data, dt, cap=cap[2:5], lengths=lengths[2:5])       # another n
        assert same(base.map(lambda x: x[2:5]), few)
        images5 = torch.cat([images, images[1:2].flip(-1)])                          # a fifth template appended
        labels5 = torch.cat([labels, labels[1:2]])
        more = pairs(model, kind, data, dt, images=images5, labels=labels5)
        assert more.logprob.shape == (7, 5) and same(base, more.map(lambda x: x[:, :4]))
        assert same(more, pairs(model, kind, data, dt, images=images5, labels=labels5, batch_size=5))


# ---- 3. shared template keys == gathered template keys ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.CROSS_KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_shared_template_keys_are_the_gathered_ones(hip, data, kind, setting, monkeypatch):
    """Both routes through the private switch ``scoring._SHARE_TEMPLATE_KEYS`` (no option: the option table keeps its 15 entries), and
    the spy's proof that each took its route: shared -> the K|V projection, the pack and the attention see 4 images of 7 x 9 rows;
    gathered -> 28 images of 9 rows."""
    from deephumor_amd.experiments import scoring
    _, dt, opts = setting
    model = build(kind, dt)
    n_layers = E.HP[kind]["n_layers"]
    spy = Spy(hip, monkeypatch)
    seen = {}
    with hip.option_scope(**opts):
        for shared in (True, False):
            monkeypatch.setattr(scoring, "_SHARE_TEMPLATE_KEYS", shared)
            spy.clear()
            seen[shared] = pairs(model, kind, data, dt)
            if dt == F32:
                att = [(a[5], a[6]) for a in spy.named("dh_attn_cross_prefill")]
                assert not spy.named("dh_attn_cross_pack", "dh_attn_cross_prefill_packed")
            else:
                att = [(a[6], a[7]) for a in spy.named("dh_attn_cross_prefill_packed")]
                assert [a[3] for a in spy.named("dh_attn_cross_pack")] == [4 if shared else 28] * n_layers
                assert not spy.named("dh_attn_cross_prefill")
            assert att == [(4, 7 * E.L) if shared else (28, E.L)] * n_layers, att     # one call per layer: (images, rows per image)
            small = pairs(model, kind, data, dt, batch_size=5)                       # passes of 5 captions x 1 template, then 2 x 2
            assert same(seen[shared], small)
    assert same(seen[True], seen[False])


# ---- 4. the one-launch teacher-forced cross-attention --------------------------------------------------------------------------------
def cross_ref(q, kv, keymask, n_img, n_pos, s, n_heads, scale):
    d = q.shape[1]
    dh = d // n_heads
    qq = q.double().view(n_img, n_pos, n_heads, dh).transpose(1, 2)
    k = kv[:, :d].double().reshape(n_img, s, n_heads, dh).transpose(1, 2)
    v = kv[:, d:].double().reshape(n_img, s, n_heads, dh).transpose(1, 2)
    out = attn_ref(qq, k, v, keymask.view(n_img, 1, 1, s).bool(), scale)
    return out.transpose(1, 2).reshape(n_img * n_pos, d)


def cross_case(dt, n_img, n_pos, s, d):
    """q as a column slice of a wider matrix (ldq = d + 128), kv [n_img * s, 2d], one masked key in image 0 and every key of image 1
    masked (uniform attention) -- the case of tests/test_prefill_gpu.py."""
    wide = rnd(n_img * n_pos, d + 128, seed=n_pos + s).to(dt)
    kv = rnd(n_img * s, 2 * d, seed=3 * s + n_img).to(dt)
    mask = torch.zeros(n_img * s, dtype=torch.uint8)
    mask[min(3, s - 1)] = 1
    if n_img > 1:
        mask[s:2 * s] = 1
    return wide, kv, mask


N_POS = (1, 15, 16, 17, 33, 7 * 9)
# (d, heads, keys): head dim 64 with S <= 64 (the LDS kernel: the caption models' shape), S > 64 (the bandwidth-shaped kernel), head dim
# 32 (the same, other lane layout), head dim 24 (the general kernel)
ROW_KERNEL_SHAPES = ((128, 2, 49), (128, 2, 70), (64, 2, 20), (48, 2, 10))


def check_rows_inside_a_longer_call(call, q, got, n_img, n_pos, d):
    """``call(q rows, n_pos) -> out``: image ``i``'s rows 16 .. 31 as a 16-position call of their own, and a few single rows as
    1-position calls, against the same rows of the long call -- bit for bit."""
    full = got.view(n_img, n_pos, d)
    qv = q.view(n_img, n_pos, -1)
    if n_pos >= 32:
        part = call(qv[:, 16:32].reshape(n_img * 16, -1), 16).view(n_img, 16, d)
        assert torch.equal(part, full[:, 16:32])
    for r in sorted({0, n_pos // 2, n_pos - 1}):
        one = call(qv[:, r:r + 1].reshape(n_img, -1), 1).view(n_img, 1, d)
        assert torch.equal(one, full[:, r:r + 1]), r


@pytest.mark.parametrize("dt", (F32, F16, BF16), ids=("f32", "f16", "bf16"))
def test_cross_prefill_is_one_launch_for_every_position(hip, dt):
    gate = _Gate("cross_prefill", dt, ULP_GATE)
    for d, h, s in ROW_KERNEL_SHAPES:
        for n_img in (1, 3):
            for n_pos in N_POS:
                wide, kv, mask = cross_case(dt, n_img, n_pos, s, d)
                kvg, maskg = kv.cuda(), mask.cuda()
                q = wide.cuda()[:, 64:64 + d].contiguous()
                qs = wide.cuda()[:, 64:64 + d]                                       # ldq > d
                call = lambda rows, np_: hip.attn_cross_prefill(rows, kvg, maskg, n_img, np_, s, d, h, 8.0)      # noqa: E731
                got = call(qs, n_pos)
                assert torch.equal(got, call(q, n_pos))
                gate.add(got, cross_ref(wide[:, 64:64 + d], kv, mask, n_img, n_pos, s, h, 8.0), dict(d=d, n_img=n_img, s=s, n_pos=n_pos))
                check_rows_inside_a_longer_call(call, q, got, n_img, n_pos, d)
    gate.check()


@pytest.mark.parametrize("dt", (F16, BF16), ids=("f16", "bf16"))
def test_cross_prefill_packed_is_one_launch_for_every_position(hip, dt):
    gate = _Gate("cross_prefill_packed", dt, ULP_GATE)
    d, h = 128, 2
    for s in (7, 49, 64):
        for n_img in (1, 3):
            for n_pos in N_POS:
                wide, kv, mask = cross_case(dt, n_img, n_pos, s, d)
                maskg = mask.cuda()
                q = wide.cuda()[:, 64:64 + d].contiguous()
                qs = wide.cuda()[:, 64:64 + d]
                want = cross_ref(wide[:, 64:64 + d], kv, mask, n_img, n_pos, s, h, 8.0)
                for dperm in (False, True):
                    kp, vt = hip.attn_cross_pack(kv.cuda(), n_img, s, d, h, dperm=dperm)
                    call = lambda rows, np_: hip.attn_cross_prefill_packed(rows, kp, vt, maskg, n_img, np_, s, d, h, 8.0, dperm=dperm)   # noqa: E731
                    got = call(qs, n_pos)
                    assert torch.equal(got, call(q, n_pos))
                    gate.add(got, want, dict(n_img=n_img, s=s, n_pos=n_pos, dperm=dperm))
                    check_rows_inside_a_longer_call(call, q, got, n_img, n_pos, d)
    gate.check()


@pytest.mark.parametrize("dt", (F32, BF16), ids=("f32", "bf16"))
def test_forward_calls_the_cross_attention_once_per_layer(hip, data, dt, monkeypatch):
    """``forward`` at 25 positions (two chunks of 16 before): one call per layer over all 25 -- see the module docstring for what a
    Python-side recorder can and cannot see of the launches behind it."""
    kind = "CaptioningTransformer"
    model = build(kind, dt)
    images = data[0][:3].to(dt)
    g = torch.Generator().manual_seed(3)
    cap = torch.randint(6, E.V, (3, 24), generator=g).cuda()
    spy = Spy(hip, monkeypatch)
    with torch.no_grad():
        feats, spatial = model.encoder(images)
        spy.clear()
        model.decoder(cap, enc_out=spatial, start_emb=feats, num_positions=25)
    name = "dh_attn_cross_prefill" if dt == F32 else "dh_attn_cross_prefill_packed"
    at = (5, 6) if dt == F32 else (6, 7)
    assert [(a[at[0]], a[at[1]]) for a in spy.named(name)] == [(3, 25)] * E.HP[kind]["n_layers"]


# ---- 5. structure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformerBase", "CaptioningTransformer"))
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_structure(hip, data, kind, setting, monkeypatch):
    _, dt, opts = setting
    model = build(kind, dt)
    spy = Spy(hip, monkeypatch)
    enc_real = model.encoder.forward
    batches = []

    def counted(images, *a, **kw):
        batches.append(images.shape[0])
        return enc_real(images, *a, **kw)
    monkeypatch.setattr(model.encoder, "forward", counted)
    with hip.option_scope(**opts):
        pairs(model, kind, data, dt, batch_size=5)
    assert batches == [4]                                                            # once, over the T images
    n_passes = 4 + 2                                                                 # 5 captions x 1 template (4 passes), 2 captions x 2 templates (2)
    fused, logits = spy.named("dh_vocab_logprob"), spy.named("dh_token_logprob")
    if setting[0] == "f32_exact":
        assert len(logits) == n_passes and not fused
    else:
        assert len(fused) == n_passes and not logits
    assert len(spy.named("dh_seq_perplexity")) == n_passes


# ---- 6. overflow --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningLSTM"))
def test_a_flagged_pass_is_repeated_on_the_logits_route(hip, data, kind, monkeypatch):
    """As tests/test_explain_gpu.py::test_range_guard: one hidden activation of 7e4 sets the stream's sticky word on the fused fp32 route;
    every flagged pass is repeated with the option off, so the result is the option-off result bit for bit and the word reads 0."""
    model = build(kind)
    enc_real = model.encoder.forward

    def exact_encoder(*a, **kw):              # the same encoder bits in both calls: the comparison is about the decoder's routes
        with hip.option_scope(f32_split=0):
            return enc_real(*a, **kw)
    monkeypatch.setattr(model.encoder, "forward", exact_encoder)
    with hip.option_scope(f32_split=0):
        want = pairs(model, kind, data, F32, batch_size=14)
    dec = model.decoder
    name = "hidden_states" if hasattr(dec, "lstm") else "_forward"
    real = getattr(dec, name)
    planted = []

    def plant(*a, **kw):
        out = real(*a, **kw)
        if hip.option("f32_split") and (name == "hidden_states" or kw.get("return_hidden")):      # the fused route only, not its repeat
            (out[0] if isinstance(out, tuple) else out)[1, 2, 5] = 7e4
            planted.append(1)
        return out
    monkeypatch.setattr(dec, name, plant)
    spy = Spy(hip, monkeypatch)
    assert not hip.f32x_take_overflow()
    with hip.option_scope(f32_split=1):
        got = pairs(model, kind, data, F32, batch_size=14)
        assert not hip.f32x_take_overflow()
    assert len(planted) == 2 and len(spy.named("dh_vocab_logprob")) == 2 and len(spy.named("dh_token_logprob")) == 2
    assert same(got, want) and bool(torch.isfinite(got.logprob).all())


# ---- 7. golden G26 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_golden_g26(hip, data, kind, setting):
    """Against the real reference's fp64 values.  fp32: the README's 1e-3 bar for log-probs AND 4 x the worst seen per kind; a pair sums
    at most 9 tokens, each within G25's 8.8e-6.  16-bit: 4 x the worst seen (the weights themselves are rounded: the binding check of those
    types is the bit equality of test_every_pair_is_the_single_pair_call)."""
    tag, dt, opts = setting
    g = P.golden(kind)
    with hip.option_scope(**opts):
        got = pairs(build(kind, dt), kind, data, dt)
    err = float(np.abs(got.logprob.double().cpu().numpy() - g["logprob"]).max())
    rel = float(np.abs(got.perplexity.double().cpu().numpy() / g["perplexity"] - 1).max())
    key = (kind, "f32" if dt == F32 else tag)
    print(f"[pairs g26] {kind} {tag}: logprob {err:.3e} (worst seen {P.WORST_LOGPROB.get(key)}), "
          f"perplexity {rel:.3e} relative (worst seen {P.WORST_PERPLEXITY_REL.get(key)})")
    if dt == F32:
        assert err <= 1e-3
    assert err <= P.gate(P.WORST_LOGPROB[key]) and rel <= P.gate(P.WORST_PERPLEXITY_REL[key])
