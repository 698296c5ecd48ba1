"""``experiments.occlusion_maps`` on a real MI355X.

The shapes are the smallest where it can go wrong: ``explain_ref``'s tiny models (V = 300), four templates (the fourth a second copy of
the first), three captions of 7 positions (lengths 7, 4, 2) under every template -- 12 rows, caption-major, so the captions of a template
are never neighbours and grouping by template has work to do.  Patch level: S = 49, 50 variants per template: ``batch_size`` 256 holds a
template's 3 x 50 sequences in one pass, 64 cuts the variants (21 per pass), 5 one variant of 3 captions per pass, 1 cuts the captions
too.  Pixel level: grids (1, 1), (2, 2) and (3, 2) -- the last divides neither 224 by 3 nor the passes evenly.

What is equality here is asked as equality: every occluded row against ``_pass_logprobs`` on that single sequence with hand-zeroed
features / hand-occluded images, every invariance, the two K|V routes, ``base`` against ``score_pairs``, ``score_pairs`` against a
copy of its body before the pass loop became a shared helper.

Against the fp32 restatement (``occlusion_ref``) and golden G27 (the real reference): fp32 within ``occlusion_ref.CEILING`` = L x 2e-3
and within 1.25 x the worst value seen on an MI355X (``occlusion_ref.WORST``); the 16-bit types print what they measure -- their weights
are rounded, their binding check is the bit equality above.  A sign or a best region is compared only after asserting that the
reference's own margin (``occlusion_ref.margin`` / ``top_gap``) exceeds twice the gate.

``token_drop`` against ``drop``: each of the L per-token differences is rounded to fp32 once (half an ulp of its size) and ``drop`` once:
the fp64 sum of ``token_drop`` is within ``sum_p ulp(token_drop[p]) / 2 + ulp(drop) / 2`` of ``drop``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import explain_ref as E  # noqa: E402
import occlusion_ref as O  # noqa: E402
from attn_ref import BF16, F16, F32  # noqa: E402
from helpers import synth_images  # noqa: E402

SETTINGS = (("f32_split", F32, dict(f32_split=1)), ("f32_exact", F32, dict(f32_split=0)), ("f16", F16, {}), ("bf16", BF16, {}))
SET_IDS = [s[0] for s in SETTINGS]
PATCH_SAMPLE = (0, 7, 24, 48)              # the regions whose single-sequence passes are run: corners of the index range and two inside


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


_MODELS = {}
_RESTATED = {}


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
    _RESTATED.clear()


@pytest.fixture(scope="module")
def data():
    """(images [4, 3, 224, 224], captions [12, 7], lengths [12], template_index [12], labels [4, 3]) on the GPU."""
    return tuple(t.cuda() for t in O.inputs(synth_images(E.N_TEMPLATES, seed=0)))


def lab(kind, labels):
    return labels if "WithLabels" in kind else None


def occl(model, kind, data, dt, rows=None, **kw):
    from deephumor_amd.experiments import occlusion_maps
    images, cap, lengths, index, labels = data
    if rows is not None:
        cap, lengths, index = cap[rows], lengths[rows], index[rows]
    return occlusion_maps(model, images.to(dt), index, cap, lengths, labels=lab(kind, labels), **kw)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def encode(model, kind, images, labels):
    with torch.no_grad():
        out = model.encoder(images, labels) if "WithLabels" in kind else model.encoder(images)
    return out if isinstance(out, tuple) else (out, None)


def single_row(model, feats, spatial, cap_row):
    """One sequence through the pass helper -> its fp32 row ``[L]`` with exact zeros at pads."""
    from deephumor_amd.experiments import scoring
    with torch.no_grad():
        logp, _ = scoring._pass_logprobs(model.decoder, feats, spatial, cap_row)
    return logp.masked_fill(cap_row == E.PAD, 0.0)[0]


def expect(base_row, row):
    """(base, drop, token_drop) of one (caption, region) from the two fp32 rows, by the definition: fp64 sums, one rounding."""
    b, r = base_row.double(), row.double()
    return b.sum().float(), (b.sum() - r.sum()).float(), (b - r).float()


def check_against_rows(got, i, r, base_row, row):
    base, drop, tokens = expect(base_row, row)
    assert torch.equal(got.base[i], base), (i, float(got.base[i]), float(base))
    assert torch.equal(got.drop[i, r], drop), (i, r, float(got.drop[i, r]), float(drop))
    assert torch.equal(got.token_drop[i, :, r], tokens), (i, r)


def check_shapes(got, n, regions, cap):
    assert got.base.shape == (n,) and got.drop.shape == (n, regions) and got.token_drop.shape == (n, O.L, regions)
    assert got.base.dtype == got.drop.dtype == got.token_drop.dtype == torch.float32 and got.base.is_cuda
    assert bool((got.token_drop[cap == E.PAD] == 0).all()) and bool(torch.isfinite(got.drop).all()) and bool((got.base < 0).all())
    total, drop = got.token_drop.double().sum(1).cpu().numpy(), got.drop.cpu().numpy()
    bound = (np.spacing(np.abs(got.token_drop.cpu().numpy())).astype(np.float64).sum(1) + np.spacing(np.abs(drop)).astype(np.float64)) / 2
    assert bool((np.abs(total - drop.astype(np.float64)) <= bound).all())


def check_invariances(model, kind, data, dt, got, sizes, **kw):
    cap = data[1]
    for bs in sizes:
        assert same(got, occl(model, kind, data, dt, return_tokens=True, batch_size=bs, **kw)), bs
    perm = torch.tensor([7, 2, 11, 0, 5, 9, 4, 1, 10, 3, 8, 6], device="cuda")
    assert same(got.map(lambda x: x[perm]), occl(model, kind, data, dt, rows=perm, return_tokens=True, **kw))
    few = torch.tensor([9, 1], device="cuda")                                            # another n: two captions of template 1
    assert same(got.map(lambda x: x[few]), occl(model, kind, data, dt, rows=few, return_tokens=True, **kw))
    plain = occl(model, kind, data, dt, **kw)                                            # without the tokens: the same two fields
    assert plain.token_drop is None and torch.equal(plain.base, got.base) and torch.equal(plain.drop, got.drop)
    for x in (got.base, got.drop, got.token_drop):                                       # the copy of template 0: rows 4 c + 3 and 4 c
        assert torch.equal(x[3::4], x[0::4])
    assert cap.shape[0] == 12


def report(what, kind, tag, dt, got, want_base, want_drop, level):
    eb = float(np.abs(got.base.double().cpu().numpy() - np.asarray(want_base)).max())
    ed = float(np.abs(got.drop.double().cpu().numpy() - np.asarray(want_drop)).max())
    key = (kind, level, what)
    seen = O.WORST.get(key) if dt == F32 else O.WORST_16[(kind, level)][tag] if what == "g27" else "not kept"
    print(f"[occlusion {what}] {kind} {level} {tag}: base {eb:.3e}, drop {ed:.3e} (worst seen {seen})")
    if dt == F32:
        assert eb <= O.CEILING and ed <= O.CEILING
        assert eb <= O.gate(O.WORST[key][0]) and ed <= O.gate(O.WORST[key][1])
    return ed


class Spy:
    """The ``hip._launch`` recorder of tests/test_pairs_gpu.py: (name, args) of every native call."""

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


# ---- 1. patch level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.CROSS_KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_patch_level(hip, data, kind, setting):
    from deephumor_amd.experiments import explain_captions, score_pairs
    tag, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, index, labels = data
    with hip.option_scope(**opts):
        got = occl(model, kind, data, dt, return_tokens=True)
        check_shapes(got, 12, 49, cap)
        feats, spatial = encode(model, kind, images.to(dt), labels)
        for i in range(12):
            t = int(index[i])
            base_row = single_row(model, feats[t:t + 1], spatial[t:t + 1], cap[i:i + 1])
            for s in PATCH_SAMPLE:
                zeroed = spatial[t:t + 1].clone()
                zeroed[0, s] = 0
                check_against_rows(got, i, s, base_row, single_row(model, feats[t:t + 1], zeroed, cap[i:i + 1]))
        check_invariances(model, kind, data, dt, got, (1, 5, 64, 256))
        pairs = score_pairs(model, images.to(dt), cap, lengths, labels=lab(kind, labels))
        assert torch.equal(got.base, pairs.logprob[torch.arange(12), index.cpu()])
        rows = explain_captions(model, images.to(dt), index, cap, lengths, labels=lab(kind, labels)).logprobs
        assert torch.equal(got.base, rows.sum(-1, dtype=torch.float64).float())
    # the restatement: ref_path's decoder on the model's own (possibly rounded) weights and its own encoder output
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    base, drop, _ = O.patch_level(sd, E.HP[kind]["n_heads"], feats.float().cpu(), spatial.float().cpu(), cap.cpu(), index.cpu())
    report("restatement", kind, tag, dt, got, base.numpy(), drop.numpy(), "patch")
    g = O.golden(kind)
    ed = report("g27", kind, tag, dt, got, g["patch_base"], g["patch_drop"], "patch")
    if dt == F32:
        assert O.top_gap(g["patch_drop"]) > 2 * O.gate(O.WORST[(kind, "patch", "g27")][1]) >= 2 * ed      # the margin first, then the ranking
        assert np.array_equal(got.drop.argmax(1).cpu().numpy(), g["patch_drop"].argmax(1))


@pytest.mark.parametrize("kind", E.CROSS_KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_patch_routes_and_masked_patches(hip, data, kind, setting, monkeypatch):
    """Both K|V routes through the private switch ``scoring._COPY_VARIANT_KEYS`` give the same bits, and the spy's proof that each took
    its route in 16-bit: copied -> ``dh_attn_cross_pack`` sees ONE image per layer and pass; per variant -> the 50 variants of the pass.
    Then a zero planted in feature row 5 of every template (a key the model's own rule masks): its column of ``drop`` is exactly 0.0 on
    both routes.  Then template 1 with a zero in every row but row 2: hiding row 2 leaves no key, the softmax over masked keys is uniform
    and shows the zeroed row's K|V -- both routes give what the hand-zeroed features give."""
    from deephumor_amd.experiments import scoring
    tag, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, index, labels = data
    n_layers = E.HP[kind]["n_layers"]
    spy = Spy(hip, monkeypatch)
    enc_real = model.encoder.forward
    plant = {}

    def planted(*a, **kw):
        feats, spatial = enc_real(*a, **kw)
        spatial = spatial.clone()
        if plant.get("row5"):
            spatial[:, 5, 3] = 0
        if plant.get("one_key"):
            spatial[1, :2, 0] = 0
            spatial[1, 3:, 0] = 0
        return feats, spatial
    monkeypatch.setattr(model.encoder, "forward", planted)
    with hip.option_scope(**opts):
        for case in ("plain", "row5", "one_key"):
            plant.clear()
            plant[case] = True
            seen = {}
            for copied in (True, False):
                monkeypatch.setattr(scoring, "_COPY_VARIANT_KEYS", copied)
                spy.clear()
                seen[copied] = occl(model, kind, data, dt, return_tokens=True)
                packs = [a[3] for a in spy.named("dh_attn_cross_pack")]
                if dt != F32:
                    one = copied and case != "one_key"                                   # (a variant without a key: zeroed features on both)
                    assert packs == [1 if one else 50] * (n_layers * 4), (case, copied, packs)
                else:
                    assert not packs and len(spy.named("dh_attn_cross_prefill")) == n_layers * 4
                assert same(seen[copied], occl(model, kind, data, dt, return_tokens=True, batch_size=5))
            assert same(seen[True], seen[False]), case
            got = seen[True]
            if case == "plain":
                assert bool((got.drop != 0).any())
                continue
            feats, spatial = encode(model, kind, images.to(dt), labels)
            if case == "row5":
                assert bool((got.drop[:, 5] == 0.0).all()) and bool((got.token_drop[:, :, 5] == 0.0).all())
                assert bool((got.drop[:, :5] != 0).any()) and bool((got.drop[:, 6:] != 0).any())
                pick = [(i, s) for i in (0, 6) for s in (4, 5, 6)]
            else:
                on1 = index == 1
                others = torch.ones(49, dtype=torch.bool, device="cuda")
                others[2] = False
                assert bool((got.drop[on1][:, others] == 0.0).all()) and bool((got.drop[on1][:, 2] != 0.0).all())
                assert bool((got.drop[~on1] != 0).any())
                pick = [(i, s) for i in (1, 5, 9) for s in (2, 3)]
            for i, s in pick:
                t = int(index[i])
                zeroed = spatial[t:t + 1].clone()
                zeroed[0, s] = 0
                check_against_rows(got, i, s, single_row(model, feats[t:t + 1], spatial[t:t + 1], cap[i:i + 1]),
                                   single_row(model, feats[t:t + 1], zeroed, cap[i:i + 1]))


# ---- 2. pixel level -----------------------------------------------------------------------------------------------------------------
def restated_pixel(kind):
    """``occlusion_ref.pixel_level`` on the fp32 weights, grid (2, 2): once per kind."""
    if kind not in _RESTATED:
        images, cap, lengths, index, labels = O.inputs(synth_images(E.N_TEMPLATES, seed=0))
        sd = {k: v.detach().float().cpu() for k, v in build(kind).state_dict().items()}
        _RESTATED[kind] = O.pixel_level(kind, sd, E.HP[kind].get("n_heads", 0), images, labels, cap, index, O.GOLDEN_GRID, O.FILL)
    return _RESTATED[kind]


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_pixel_level(hip, data, kind, setting):
    from deephumor_amd.experiments import explain_captions, score_pairs
    tag, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, index, labels = data
    with hip.option_scope(**opts):
        by_grid = {}
        for grid in O.GRIDS:
            got = by_grid[grid] = occl(model, kind, data, dt, level="pixel", grid=grid, fill=O.FILL, return_tokens=True)
            check_shapes(got, 12, grid[0] * grid[1], cap)
            boxes = O.regions(224, 224, grid)
            for t in range(4):
                variants = torch.stack([images[t]] + [O.occlude(images[t], box, O.FILL) for box in boxes]).to(dt)
                feats, spatial = encode(model, kind, variants, labels[t:t + 1].repeat(len(variants), 1))
                for i in range(t, 12, 4):
                    rows = [single_row(model, feats[v:v + 1], None if spatial is None else spatial[v:v + 1], cap[i:i + 1])
                            for v in range(len(variants))]
                    for r in range(len(boxes)):
                        check_against_rows(got, i, r, rows[0], rows[1 + r])
        check_invariances(model, kind, data, dt, by_grid[(2, 2)], (1, 5, 64, 256), level="pixel", grid=(2, 2), fill=O.FILL)
        assert same(by_grid[(3, 2)], occl(model, kind, data, dt, level="pixel", grid=(3, 2), fill=O.FILL, return_tokens=True, batch_size=5))
        # grid (1, 1): the one region is the whole image -- scoring the caption on an image made of the fill
        filled = torch.tensor(O.FILL, device="cuda").view(1, 3, 1, 1).expand(1, 3, 224, 224).to(dt).contiguous()
        zero = torch.zeros(12, dtype=torch.int64, device="cuda")
        for t in range(4):                                                               # (the label models: the template's own label)
            on_fill = explain_captions(model, filled, zero, cap, lengths, labels=lab(kind, labels[t:t + 1])).logprobs
            on_image = explain_captions(model, images[t:t + 1].to(dt), zero, cap, lengths, labels=lab(kind, labels[t:t + 1])).logprobs
            want = (on_image.sum(-1, dtype=torch.float64) - on_fill.sum(-1, dtype=torch.float64)).float()
            assert torch.equal(by_grid[(1, 1)].drop[t::4, 0], want[t::4]), t
        scalar = occl(model, kind, data, dt, level="pixel", grid=(1, 1), fill=0.25)      # one number: every channel
        assert same(scalar, occl(model, kind, data, dt, level="pixel", grid=(1, 1), fill=(0.25, 0.25, 0.25)))
        assert not torch.equal(scalar.drop, by_grid[(1, 1)].drop)
        pairs = score_pairs(model, images.to(dt), cap, lengths, labels=lab(kind, labels))
        for grid in O.GRIDS:
            assert torch.equal(by_grid[grid].base, pairs.logprob[torch.arange(12), index.cpu()]), grid
    got = by_grid[O.GOLDEN_GRID]
    base, drop, _ = restated_pixel(kind)
    report("restatement", kind, tag, dt, got, base.numpy(), drop.numpy(), "pixel")
    g = O.golden(kind)
    ed = report("g27", kind, tag, dt, got, g["pixel_base"], g["pixel_drop"], "pixel")
    if dt == F32:
        tol = O.gate(O.WORST[(kind, "pixel", "g27")][1])
        assert min(O.margin(g["pixel_drop"]), O.top_gap(g["pixel_drop"])) > 2 * tol >= 2 * ed      # the margins first
        assert np.array_equal(np.sign(got.drop.cpu().numpy()), np.sign(g["pixel_drop"]))
        assert np.array_equal(got.drop.argmax(1).cpu().numpy(), g["pixel_drop"].argmax(1))


# ---- 3. structure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningLSTM"))
def test_structure(hip, data, kind, monkeypatch):
    """The encoder sees every distinct template once (patch level) or its R + 1 images in chunks of ``batch_size`` (pixel level), and
    each caption meets only the variants of its own template: the passes hold 12 x (R + 1) sequences in all, not 12 x 4 x (R + 1)."""
    model = build(kind, BF16)
    spy = Spy(hip, monkeypatch)
    enc_real = model.encoder.forward
    batches = []

    def counted(images, *a, **kw):
        batches.append(images.shape[0])
        return enc_real(images, *a, **kw)
    monkeypatch.setattr(model.encoder, "forward", counted)
    rows = torch.tensor([0, 2, 4, 6, 10], device="cuda")                                 # templates 0 and 2 only: 3 + 2 captions
    if kind == "CaptioningTransformer":
        occl(model, kind, data, BF16, rows=rows)
        assert batches == [2]
        assert sum(a[11] for a in spy.named("dh_vocab_logprob")) == 5 * 50 * O.L         # rows of the classifier: sequences x positions
        del batches[:]
        spy.clear()
    occl(model, kind, data, BF16, rows=rows, level="pixel", grid=(3, 2), batch_size=4)
    assert batches == [4, 3, 4, 3]
    assert sum(a[11] for a in spy.named("dh_vocab_logprob")) == 5 * 7 * O.L


# ---- 4. unchanged values ------------------------------------------------------------------------------------------------------------
def score_pairs_before(model, template_images, captions, lengths, labels=None, batch_size=256, pad_index=0):
    """``score_pairs`` as it stood before its pass loop became ``scoring._score_feature_pairs`` -- the body, statement by statement."""
    from deephumor_amd import hip
    from deephumor_amd.experiments import scoring
    from deephumor_amd.experiments.scoring import PairScores, _pass_logprobs
    enc = model.encoder
    dec = model.decoder
    with torch.no_grad():
        feats = enc(template_images, labels) if labels is not None else enc(template_images)
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        dev = feats.device
        (n, l), t_all = captions.shape, feats.shape[0]
        caps, lens = captions.to(dev).contiguous(), lengths.to(dev)
        out = PairScores(torch.empty((n, t_all), dtype=torch.float32, device=dev), torch.empty((n, t_all), dtype=torch.float32, device=dev))
        for lo in range(0, n, batch_size):
            hi = min(lo + batch_size, n)
            nc = hi - lo
            per = min(max(1, batch_size // nc), t_all)
            tgt_all, lens_all = caps[lo:hi].repeat(per, 1), lens[lo:hi].repeat(per)
            pad_all = tgt_all == pad_index
            for t0 in range(0, t_all, per):
                t1 = min(t0 + per, t_all)
                rows = (t1 - t0) * nc
                tgt = tgt_all[:rows]
                idx = torch.arange(t0, t1, device=dev).repeat_interleave(nc)
                emb = feats.index_select(0, idx)
                share = nc if scoring._SHARE_TEMPLATE_KEYS and spatial is not None else 1
                sp = None if spatial is None else spatial[t0:t1] if share > 1 else spatial.index_select(0, idx)
                logp, _ = _pass_logprobs(dec, emb, sp, tgt, share=share)
                pp = hip.seq_perplexity(logp, tgt, lens_all[:rows], pad_index)
                total = logp.masked_fill(pad_all[:rows], 0.0).sum(-1, dtype=torch.float64).float()
                out.logprob[lo:hi, t0:t1] = total.view(t1 - t0, nc).t()
                out.perplexity[lo:hi, t0:t1] = pp.view(t1 - t0, nc).t()
        return out


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("setting", SETTINGS, ids=SET_IDS)
def test_score_pairs_and_explain_captions_kept_their_bits(hip, data, kind, setting):
    from deephumor_amd.experiments import explain_captions, score_captions, score_pairs
    tag, dt, opts = setting
    model = build(kind, dt)
    images, cap, lengths, index, labels = data
    with hip.option_scope(**opts):
        for bs in (256, 5):
            now = score_pairs(model, images.to(dt), cap[::4], lengths[::4], labels=lab(kind, labels), batch_size=bs)
            before = score_pairs_before(model, images.to(dt), cap[::4], lengths[::4], labels=lab(kind, labels), batch_size=bs)
            assert torch.equal(now.logprob, before.logprob) and torch.equal(now.perplexity, before.perplexity), bs
        explained = explain_captions(model, images.to(dt), index, cap, lengths, labels=lab(kind, labels))
        assert torch.equal(explained.perplexity, now.perplexity.reshape(-1))        # row 4 c + t is caption c under template t
        if dt != F32 or tag == "f32_exact":
            assert torch.equal(explained.perplexity, score_captions(model, images.to(dt), index, cap, lengths, labels=lab(kind, labels)))
