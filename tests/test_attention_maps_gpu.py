"""``generate_batch(..., return_attention=True)`` on a real MI355X.

Kernel level: ``dh_attn_cross_weights`` against the fp64 head-mean softmax of ``attn_ref.CrossCase`` in all three types (the
arithmetic is fp32 on exactly representable inputs, so the project's fp32 attention gate ``attn_ref.F32_ATOL`` holds for every
type), its logical-row mapping, and ``dh_beam_gather_attention`` bit for bit against torch indexing.

Model level, both cross-attention kinds, on the SHARPENED weights of ``attention_maps_ref`` (last layer's ``enc_attn.fc_q`` x 8: on
the synthetic weights as they are the maps are nearly flat and a map taken from the wrong row or position would pass): the prompt
columns against golden G23 (the real reference), every generated column of every beam -- through the beam shuffles -- against the
fp64 restatement ``teacher_forced_maps`` on that beam's own tokens, bitwise self-consistency of everything the keyword composes
with, graph replay, the default's launch sequence, the refusals.

Gates (``GATE``).  Measured on an MI355X, not set in advance: 4 x (fp32) / 2 x (16-bit) the worst error printed by the tests
below over both kinds, see DESIGN.md section 5.  There is ONE fp32 gate, the one measured against G23; the generated columns
and the ``f32_split`` case are held to it as well:

  fp32, prompt columns vs G23            worst 1.013e-06 -> the fp32 gate 4.05e-06
  fp32, generated columns vs fp64        worst 4.634e-07    against the fp32 gate   (with option f32_split: 1.867e-06, likewise)
  fp16 vs fp64 on the rounded weights    worst 3.211e-04 -> gate 6.42e-04
  bf16 vs fp64 on the rounded weights    worst 2.877e-03 -> no gate of that kind, see below

A 16-bit gate must stay <= 4e-3, a quarter of the 1.6e-2 by which the maps of sibling beams differ on these weights.  fp16 does,
six times over.  bf16 does not: 2 x 2.877e-03 = 5.75e-03 (CaptioningTransformer 2.368e-03, WithLabels 2.877e-03, against fp64 on
the bf16-rounded weights and the model's own encoder output).  That is the type, not the kernel -- dh_attn_cross_weights is within
2e-5 of fp64 on bf16 operands (first test below), and fp16, with 3 more mantissa bits, is 9 x closer: q and K reach the kernel
rounded to 8 bits, and at gain 8 an energy error of 2^-9 relative moves a weight of 0.18 by ~2e-3.  So bf16 has no gate of the
issue's kind; it takes part in every bitwise check below (plain == drawn slot, batch == halves == streams, prompts ==
singles, zeros past the length, rows summing to 1).  Those alone would not see a query handed to the tap in another layout, or
every beam reading one and the same wrong row, so bf16 also runs the generated-columns test against ``BF16_COARSE`` = 8e-3:
NOT the issue's gate and not derived from the measurement, but half the 1.6e-2 by which the maps of sibling beams differ --
the test requires that separation (>= 2 x the bound) of the seed it uses, so a map from another row or position is at least
the bound away from the right one.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
import attention_maps_ref as R  # noqa: E402
from attn_ref import BF16, DT_IDS, DTYPES, F16, F32  # noqa: E402
from helpers import captions_and_lengths, synthetic_sd, synth_images  # noqa: E402

# worst error seen on an MI355X (both kinds) -> gate = 4 x (fp32) / 2 x (16-bit); the tests print what they see
WORST = {F32: 1.013e-06, F16: 3.211e-04}            # fp32: prompt columns vs G23
BF16_COARSE = 8e-3                                  # half the sibling separation of 1.6e-2; see the module docstring
GATE = {F32: 4.0 * WORST[F32], F16: 2.0 * WORST[F16], BF16: BF16_COARSE}
GATE["g23"] = GATE["f32x"] = GATE[F32]              # one fp32 gate
APART = {F32: 4.0, "f32x": 4.0, F16: 4.0, BF16: 2.0}   # sibling maps must be this many gates apart on the reference side
assert GATE[F16] <= 4e-3 and GATE[F32] <= 1e-4
GEN_KW = dict(max_len=14, beam_size=5, top_k=20, temperature=1.1)
S_SET, RPI_SET, DH_SET = (1, 7, 49, 64, 65, 100), (1, 5, 16, 17), ((512, 8), (128, 8), (512, 4))


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


# ---- 1. dh_attn_cross_weights -----------------------------------------------------------------------------------------------------
def want_weights(c):
    """fp64 head mean of the softmax of the case's energies [rows, S]."""
    q, k, _, masked = c.operands()
    energy = (torch.einsum("bhtd,bhsd->bhts", q.double(), k.double()) / c.scale).masked_fill(masked, -1e8)
    return torch.softmax(energy, -1).mean(1).reshape(c.rows, c.s)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_cross_weights_against_fp64(hip, dt):
    """Every S x rows per image x (D, H), q contiguous and as a column block of a [rows, 3D] buffer (same bits), NaN-prefilled
    output with sentinel rows behind it."""
    n = 0
    for d, h in DH_SET:
        for s in S_SET:
            for rpi in RPI_SET:
                c = A.CrossCase(dt, rpi, s, d, h, float(d // h) ** 0.5)
                want = want_weights(c)
                kv, mask, wide = c.kv.cuda(), c.mask.cuda(), c.wide.cuda()
                outs = []
                for q in (wide[:, d:2 * d], wide[:, d:2 * d].contiguous()):
                    out = torch.full((c.rows + A.EXTRA_ROWS, s), float("nan"), device="cuda")
                    hip.attn_cross_weights(q, kv, mask, out, 3, rpi, 1, s, d, h, c.scale)
                    assert bool(out[c.rows:].isnan().all()), c.what()
                    outs.append(out[:c.rows].cpu())
                assert outs[0].stride(0) == s and torch.equal(outs[0], outs[1]), c.what()
                got = outs[0].view(3, rpi, s)
                np.testing.assert_allclose(got.double().numpy(), want.view(3, rpi, s).numpy(), atol=A.F32_ATOL, rtol=0, err_msg=str(c.what()))
                if s > 1:
                    assert bool((got[0, :, min(3, s - 1)] == 0.0).all()), c.what()          # the masked key beside live ones
                    assert bool((got[2, :, :s - 1] == 0.0).all()), c.what()
                assert bool((got[2, :, s - 1] == 1.0).all()), c.what()                       # the only live key
                assert float((got[1] - 1.0 / s).abs().max()) <= A.F32_ATOL, c.what()          # every key masked: uniform
                n += 1
    assert n == len(DH_SET) * len(S_SET) * len(RPI_SET)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_cross_weights_row_mapping(hip, dt):
    """One compact row per image, ``row_mult = 4`` (the prefix phase of a beam-4 batch): logical rows 0, 4, 8 and nothing else."""
    c = A.CrossCase(dt, 1, 49, 512, 8, 8.0)
    out = torch.full((12 + A.EXTRA_ROWS, 49), float("nan"), device="cuda")
    hip.attn_cross_weights(c.wide.cuda()[:, 512:1024], c.kv.cuda(), c.mask.cuda(), out, 3, 1, 4, 49, 512, 8, 8.0)
    out = out.cpu()
    written = ~out.isnan().any(1)
    assert written.nonzero().flatten().tolist() == [0, 4, 8] and bool(out[~written].isnan().all())
    np.testing.assert_allclose(out[written].double().numpy(), want_weights(c).numpy(), atol=A.F32_ATOL, rtol=0)


# ---- 2. dh_beam_gather_attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 49])
def test_gather_is_bit_exact(hip, s):
    n, beam, t, n_pos = 3, 4, 6, 7
    rows = n * beam
    g = torch.Generator().manual_seed(40 + s)
    attn_w = torch.randn(n_pos, rows, s, generator=g)
    src = A.SelfCase(F32, n, beam, 1, 64, 8, 0, n_pos - 1, 0, 8.0).src                    # [rows, n_pos + 2]: random within each image
    assert src.shape == (rows, n_pos + 2) and bool(((src // beam) == (torch.arange(rows)[:, None] // beam)).all())
    index = torch.stack([torch.randperm(beam, generator=g) for _ in range(n)]).int()
    lengths = torch.randint(0, t + 1, (n, beam), generator=g, dtype=torch.int32)
    lengths[0, 0], lengths[0, 1] = 0, t
    out = torch.full((n * beam * t * s + 64,), float("nan"), device="cuda")
    view = out[:n * beam * t * s].view(n, beam, t, s)
    hip.beam_gather_attention(attn_w.cuda(), src.cuda(), index.cuda(), lengths.cuda(), view)
    want = torch.zeros(n, beam, t, s)
    for i in range(n):
        for j in range(beam):
            r = i * beam + int(index[i, j])
            for c in range(int(lengths[i, j])):
                want[i, j, c] = attn_w[c, int(src[r, c])]
    assert torch.equal(view.cpu(), want) and bool(out[n * beam * t * s:].isnan().all())


# ---- 3. models ----------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def build(kind, dt=F32, sharp=True, **hp_over):
    """The kind on the (sharpened) synthetic weights in ``dt`` on the GPU, built once -> (model, hp)."""
    key = (kind, dt, sharp, tuple(sorted(hp_over.items())))
    if key not in _MODELS:
        import deephumor_amd.models as M
        sd, hp = synthetic_sd(kind)
        hp = dict(hp, **hp_over)
        model = getattr(M, kind)(**hp).eval()
        model.load_state_dict(R.sharpened(sd) if sharp else sd)
        _MODELS[key] = (model.to(dt).cuda(), hp)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def drop_models():
    yield
    _MODELS.clear()


@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0).cuda()


def model_args(kind, images, lo=0, hi=4):
    labels = captions_and_lengths()[2].cuda()
    return (images[lo:hi], labels[lo:hi]) if "WithLabels" in kind else (images[lo:hi],)


def gen(model, args, **kw):
    with torch.no_grad():
        return model.generate_batch(*args, **kw)


def test_prompt_columns_match_the_reference(hip, images):
    """fp32, G23's prompt: columns 0 .. 5 of EVERY beam of images 0 and 1 are G23's positions 0 .. 5 (the beams share them)."""
    worst = 0.0
    for kind, name in ((R.KINDS[0], "sharp"), (R.KINDS[1], "sharp"), (R.KINDS[0], "plain")):
        g = R.golden(kind)
        model, _ = build(kind, sharp=name == "sharp")
        beams, att = gen(model, model_args(kind, images, 0, 2), caption=torch.from_numpy(g["prompt"]).cuda(), max_len=8, beam_size=3,
                         top_k=20, seed=3, return_beams=True, return_attention=True)
        assert att.shape == (2, 3, 8, 49) and att.dtype == torch.float32 and bool((beams.lengths >= 6).all())
        err = float((att[:, :, :6].cpu().double() - torch.from_numpy(g[name]).double()[:, None]).abs().max())
        print(f"[attention g23] {kind} {name}: {err:.3e}")
        worst = max(worst, err)
    print(f"[attention g23] worst {worst:.3e} (gate {GATE['g23']:.3e})")
    assert worst <= GATE["g23"]


def forked(tokens, pos=0):
    """Some image has two beams with the same first generated token that differ later."""
    for row in tokens.tolist():
        for a in range(len(row)):
            for b in range(a):
                if row[a][pos] == row[b][pos] and row[a] != row[b]:
                    return True
    return False


def reference_maps(model, hp, kind, images, tokens):
    """fp64 maps [N, B, T, 49] of every beam's own tokens on the model's (possibly 16-bit-rounded) weights and its own encode."""
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        start, enc = (t.float().cpu() for t in model.encode(*model_args(kind, images)))
        return torch.stack([R.teacher_forced_maps(sd, start[i:i + 1].expand(tokens.shape[1], -1), enc[i:i + 1].expand(tokens.shape[1], -1, -1),
                                                  tokens[i, :, :-1], hp["pad_index"], hp["n_heads"])[..., :R.N_KEYS] for i in range(tokens.shape[0])])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which", [F32, "f32x", F16, BF16], ids=["f32", "f32_split", "f16", "bf16_coarse"])
def test_generated_columns_through_the_beam_shuffles(hip, images, kind, which):
    """Every beam of every image: ``attention[i, j, :lengths[i, j]]`` is the restatement on that beam's own tokens.  Not vacuous:
    some image holds a fork (a row whose early positions another row computed), and on the reference side two beams of an image
    with different histories at a column have maps there >= 4 x the gate apart (bf16: 2 x its coarse bound = the 1.6e-2)."""
    dt = F32 if which == "f32x" else which
    model, hp = build(kind, dt)
    opts = dict(f32_split=1) if which == "f32x" else {}
    for seed in range(77, 85):                        # (the seed walks on until the conditions hold)
        with hip.option_scope(**opts):
            beams, att = gen(model, model_args(kind, images), seed=seed, return_beams=True, return_attention=True, **GEN_KW)
        tokens, lengths = beams.tokens.cpu(), beams.lengths.cpu()
        want = reference_maps(model, hp, kind, images, tokens)
        apart = float("inf")
        for i in range(4):
            for a in range(5):
                for b in range(a):
                    for c in range(1, int(min(lengths[i, a], lengths[i, b]))):
                        if tokens[i, a, :c].tolist() != tokens[i, b, :c].tolist():
                            apart = min(apart, float((want[i, a, c] - want[i, b, c]).abs().max()))
        if forked(tokens) and apart >= APART[which] * GATE[which]:
            break
    else:
        pytest.fail(f"no seed in 77 .. 84 gives a fork and maps {APART[which] * GATE[which]:.1e} apart (last: {apart:.3e})")
    assert att.shape == (4, 5, 14, 49) and int(lengths.min()) >= 1
    got = att.cpu().double()
    filled = torch.arange(14)[None, None, :] < lengths[:, :, None]
    err = float((got - want)[filled].abs().max())
    print(f"[attention generated] {kind} {which}: seed {seed}, worst {err:.3e} (gate {GATE[which]:.3e}), sibling maps >= {apart:.3e} apart")
    assert bool((got[~filled] == 0).all())
    assert err <= GATE[which]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_bitwise_self_consistency(hip, images, kind, dt):
    model, _ = build(kind, dt)
    args = model_args(kind, images)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.1, seed=5)
    toks, lens, att = gen(model, args, return_attention=True, **kw)
    assert same((toks, lens), gen(model, args, **kw)) and att.shape == (4, 10, 49) and att.dtype == torch.float32 and att.is_cuda
    beams, att4 = gen(model, args, return_beams=True, return_attention=True, **kw)
    assert same(beams, gen(model, args, return_beams=True, **kw)) and att4.shape == (4, 3, 10, 49)
    assert torch.equal(att, att4[torch.arange(4), beams.drawn])                              # the plain call = the drawn slot
    filled = torch.arange(10, device="cuda")[None, None, :] < beams.lengths[:, :, None]
    assert bool((att4[~filled] == 0).all()) and bool((att4[filled] >= 0).all())
    assert float((att4[filled].sum(-1) - 1).abs().max()) <= 1e-5
    # batch == halves == streams == early stop
    lo = gen(model, model_args(kind, images, 0, 2), return_beams=True, return_attention=True, **kw)
    hi = gen(model, model_args(kind, images, 2, 4), return_beams=True, return_attention=True, img0=2, **kw)
    assert torch.equal(torch.cat([lo[1], hi[1]]), att4) and same(type(beams).cat([lo[0], hi[0]]), beams)
    for extra in (dict(streams=2), dict(early_stop_every=2), dict(streams=2, early_stop_every=2)):
        b2, a2 = gen(model, args, return_beams=True, return_attention=True, **kw, **extra)
        assert same(b2, beams) and torch.equal(a2, att4), extra
        assert same(gen(model, args, return_attention=True, **kw, **extra), (toks, lens, att)), extra
    # generate = row 0
    with torch.no_grad():
        cap, a1 = model.generate(*model_args(kind, images, 0, 1), return_attention=True, **kw)
        b1, ab1 = model.generate(*model_args(kind, images, 0, 1), return_attention=True, return_beams=True, **kw)
    n0 = int(lens[0])
    assert torch.equal(cap, toks[0, :n0]) and a1.shape == (n0, 49) and torch.equal(a1, att[0, :n0])
    assert torch.equal(ab1, att4[:1]) and same(b1, beams.map(lambda t: t[:1]))
    # a prompted batch = the four dense single-image calls
    cap = captions_and_lengths()[0][:4, :5].cuda()
    plens = [0, 2, 5, 3]
    pt, pl, pa = gen(model, args, caption=cap, caption_lengths=torch.tensor(plens), return_attention=True, **kw)
    assert same((pt, pl), gen(model, args, caption=cap, caption_lengths=torch.tensor(plens), **kw))
    for i, n in enumerate(plens):
        st, sl, sa = gen(model, model_args(kind, images, i, i + 1), caption=cap[i:i + 1, :n] if n else None, img0=i, return_attention=True, **kw)
        assert torch.equal(st[0], pt[i]) and torch.equal(sl[0], pl[i]) and torch.equal(sa[0], pa[i]), (i, n)
    # the other generators and the general sampler carry it too
    for extra in (dict(rng="torch"), dict(exact=True), dict(top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.2, min_len=3)):
        t3 = gen(model, args, return_attention=True, **kw, **extra)
        assert same(t3[:2], gen(model, args, **kw, **extra)) and t3[2].shape == (4, 10, 49), extra


@pytest.mark.parametrize("kind", R.KINDS)
def test_graph_replay(hip, images, kind):
    model, _ = build(kind, BF16)
    args = model_args(kind, images)
    kw = dict(max_len=8, beam_size=3, top_k=20)
    first = None
    for seed in (3, 4):
        with torch.no_grad():
            got = model.generate_batch_graphed(*args, seed=seed, return_attention=True, **kw)
            plain = model.generate_batch_graphed(*args, seed=seed, **kw)
            beams, batt = model.generate_batch_graphed(*args, seed=seed, return_attention=True, return_beams=True, **kw)
        want = gen(model, args, seed=seed, return_attention=True, **kw)
        assert len(got) == 3 and same(got, want) and len(plain) == 2 and same(plain, want[:2])
        assert torch.equal(batt[torch.arange(4), beams.drawn], want[2])
        if first is None:
            first = (got, tuple(t.clone() for t in got))
    assert same(*first) and not torch.equal(first[0][2], got[2])                             # the second replay left the first result alone
    assert len(model._graphs) == 3
    with torch.no_grad():                     # return_attention=False is the plain call: the plain graph, not a fourth one
        off = model.generate_batch_graphed(*args, seed=4, return_attention=False, **kw)
    assert same(off, plain) and len(model._graphs) == 3


@pytest.mark.parametrize("kind", R.KINDS)
def test_default_is_the_call_without_the_keyword(hip, images, kind, monkeypatch):
    """Equal outputs and the same launches, counted at ``hip._launch``; on, the position driver with the tap, the n-best final
    draw and one gather take the place of their plain forms -- nothing else."""
    model, _ = build(kind, BF16)
    args = model_args(kind, images)
    kw = dict(max_len=8, beam_size=3, top_k=10, seed=1)
    names = []
    real = hip._launch

    def counting(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", counting)

    def run(**extra):
        del names[:]
        return gen(model, args, **kw, **extra), list(names)
    run()
    for streams in (1, 2):
        plain, p_names = run(streams=streams)
        off, off_names = run(streams=streams, return_attention=False)
        assert same(plain, off) and off_names == p_names
        on, on_names = run(streams=streams, return_attention=True)
        assert same(on[:2], plain)
        swap = {"dh_transformer_decode_position": "dh_transformer_decode_position_attn", "dh_beam_finalize": "dh_beam_finalize_beams"}
        want = []
        for n in p_names:
            want.append(swap.get(n, n))
            if n == "dh_beam_finalize":
                want.append("dh_beam_gather_attention")
        assert on_names == want and on_names.count("dh_beam_gather_attention") == streams
        assert p_names.count("dh_transformer_decode_position") == 9 * streams


def test_refusals(hip, images):
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline
    kind = R.KINDS[0]
    model, _ = build(kind, F32)
    args = model_args(kind, images)
    one, _ = build(kind, F32, pad_index=1)
    for call in (one.generate_batch, one.generate, one.generate_batch_graphed):
        with pytest.raises(NotImplementedError, match="pad_index == 1"):
            call(*model_args(kind, images, 0, 1), max_len=6, beam_size=2, top_k=5, return_attention=True)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="pad_index == 1"):
            one.decode(one.encode(*args), max_len=6, beam_size=2, top_k=5, return_attention=True)
        with pytest.raises(TypeError, match="must be a bool"):
            model.decode(model.encode(*args), max_len=6, beam_size=2, top_k=5, return_attention=1)
    with pytest.raises(NotImplementedError, match="^return_attention: "):
        CaptionPipeline(model, max_len=6, beam_size=2, top_k=5, return_attention=True)
    with pytest.raises(TypeError, match="must be a bool"):
        CaptionPipeline(model, max_len=6, beam_size=2, top_k=5, return_attention=1)
    assert "return_attention" not in CaptionPipeline(model, max_len=6, beam_size=2, top_k=5, return_attention=False).gen_kw
    with pytest.raises(NotImplementedError, match="^return_attention: "):
        dist.generate_sharded(lambda lo, hi: gen(model, model_args(kind, images, lo, hi), max_len=6, beam_size=2, top_k=5, seed=1, img0=lo,
                                                 return_attention=True), 4)
    base, _ = build("CaptioningTransformerBase", F32, sharp=False)
    with pytest.raises(TypeError, match="no encoder attention"):
        base.decode(base.encode(images), max_len=6, beam_size=2, top_k=5, return_attention=True)


def test_padded_keys_of_pad_index_2(hip, images):
    """``pad_index >= 2``: nothing is masked and once ``max_len + 1`` exceeds 49 the padded zero rows are real keys --
    ``S = max_len + 1`` -- whose weights the restatement gives too."""
    kind = R.KINDS[0]
    model, hp = build(kind, F32, pad_index=2)
    beams, att = gen(model, model_args(kind, images, 0, 2), max_len=52, beam_size=2, top_k=20, seed=2, return_beams=True, return_attention=True)
    assert att.shape == (2, 2, 52, 53)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        start, enc = (t.float().cpu() for t in model.encode(*model_args(kind, images, 0, 2)))
        # (all 52 columns teacher-forced: 53 positions, the engine's key count; position c sees tokens[:c] only)
        want = R.teacher_forced_maps(sd, start[:1].expand(2, -1), enc[:1].expand(2, -1, -1), beams.tokens[0].cpu(), 2, hp["n_heads"])[:, :52]
    assert want.shape == (2, 52, 53)
    filled = torch.arange(52)[None, :] < beams.lengths[0].cpu()[:, None]
    err = float((att[0].cpu().double() - want)[filled].abs().max())
    print(f"[attention pad_index 2] worst {err:.3e}")
    assert err <= GATE[F32] and float(want[..., 49:].sum(-1).min()) > 1e-3
