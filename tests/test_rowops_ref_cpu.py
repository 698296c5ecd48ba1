"""rowops_ref.py without a GPU: its references against torch in fp64 (F.layer_norm, F.max_pool2d, torch.log_softmax, permute and
the like), its case tables against the route sets that test_rowops_routes_gpu.py and test_pools_layout_gpu.py assert, and the
CPU fp32 yardsticks that their gates are built from, recomputed and compared with the tables entered there."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
import test_pools_layout_gpu as GP
import test_rowops_routes_gpu as GR
from rowops_ref import BF16, DTYPES, F16, F32, NAME

# A yardstick is the worst error of a CPU fp32 library routine over a table's cases.  Its last digits depend on the routine's
# vector width, so a recomputed value must lie within a factor 2 of the entered one; a table made from other cases, another
# reference or another scale of the operands is off by more than that somewhere.
STALE = 2.0


def fresh(table, now):
    assert set(table) == set(now), set(table) ^ set(now)
    bad = {k: (table[k], now[k]) for k in table if not (now[k] / STALE <= table[k] <= now[k] * STALE)}
    assert not bad, bad


# ---- routes ---------------------------------------------------------------------------------------------------------------------
def test_layernorm_route_rule_and_tables():
    assert [R.ln_route(d, F32) for d in (8, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [R.ln_route(d, BF16) for d in (8, 512, 520, 1024, 1032, 2048, 2056, 4096)] == [1, 1, 2, 2, 4, 4, 8, 8]
    for dt in DTYPES:
        nvs = {R.ln_route(d, dt) for d in range(8, R.LN_MAX_D + 1, 8)}
        assert nvs == set(R.LN_REACHABLE[dt])                                   # 16-bit rows never reach NV = 16
        per_pass = 64 * R.vec_elems(dt)
        for nv in R.LN_REACHABLE[dt]:
            widths = [d for d in R.LN_WIDTHS[dt] if R.ln_route(d, dt) == nv]
            top = min(nv * per_pass, R.LN_MAX_D)
            assert top in widths, (NAME[dt], nv)                                 # the route's upper boundary
            assert nv == 1 or (nv // 2) * per_pass + 8 in widths, (NAME[dt], nv)   # the first width past the route below
            assert any(R.ln_dead_lanes(d, dt) > 0 for d in widths), (NAME[dt], nv)   # a last pass with dead lanes
            assert any(R.ln_dead_lanes(d, dt) == 0 for d in widths), (NAME[dt], nv)
        assert {(-r) % 4 for r in R.LN_ROWS} == {0, 1, 3}                        # idle waves of the tail workgroup
        for cases in (R.ln_real_cases(dt), R.ln_spike_cases(dt), R.ln_const_cases(dt)):
            seen = {(c.nv, c.form) for c in cases}
            assert {nv for nv, _ in seen} == set(R.LN_REACHABLE[dt])
            assert {"y", "none"} <= {f for _, f in seen}
        assert {(c.rows, c.form) for c in R.ln_real_cases(dt)} == {(r, f) for r in R.LN_ROWS for f in R.LN_FORMS}
    assert {(k[1], k[2]) for k in GR.LN_YARD if k[0] == "real"} == {(NAME[dt], nv) for dt in DTYPES for nv in R.LN_REACHABLE[dt]}
    assert {(k[1], k[2]) for k in GR.LN_YARD if k[0] == "spike"} == {(NAME[dt], nv) for dt in DTYPES for nv in R.LN_REACHABLE[dt]}


def test_spike_positions_hit_the_last_live_pass():
    for dt in DTYPES:
        vn = R.vec_elems(dt)
        for d in R.LN_WIDTHS[dt]:
            pos, (p, d0) = R.ln_spike_positions(d, dt), R.ln_last_pass(d, dt)
            assert 0 in pos and d - 1 in pos and d0 in pos and d0 + vn - 1 in pos and d - vn in pos
            assert d0 < d <= d0 + 64 * vn and p < R.ln_route(d, dt)
            if R.ln_dead_lanes(d, dt) == 0:
                assert d0 + 63 * vn in pos and d0 + 64 * vn - 1 == d - 1
            x = next(iter(c for c in R.ln_spike_cases(dt) if c.d == d)).x
            assert x.shape[0] == len(pos) and bool((x != 0).sum(-1).eq(1).all()) and [int(r.nonzero()) for r in x] == pos


def test_wrap_tables_cover_every_capped_launcher():
    for name, (cap, case) in R.WRAP.items():
        items = R.work_items(name, case["shape"])
        assert cap < items < 1.1 * cap, (name, items, cap)
    assert not R.wraps("maxpool3x3s2", (3, 64, 15, 8)) and not R.wraps("normalize_pack_u8", (2, 17, 19, 3))
    for name, shape in R.MASK_WRAP.items():
        total = math.prod(shape) if name != "autoregressive_mask" else shape[0] * shape[1] ** 2
        assert R.MASK_WRAP_CAP < total < 1.1 * R.MASK_WRAP_CAP, (name, total)
    assert not any(R.mask_wraps(math.prod(s)) for s in R.MASK_SMALL)
    assert any(lq != lk for _, lq, lk in R.MASK_SMALL)


# ---- references against torch ---------------------------------------------------------------------------------------------------
def test_ln_ref_is_layer_norm_in_fp64():
    for dt in DTYPES:
        for c in list(R.ln_gated_cases(dt))[::17]:
            want = F.layer_norm(c.v().double(), (c.d,), c.gamma.double(), c.beta.double(), c.eps)
            assert float((c.want() - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), c.what()
            if c.y is not None:
                assert torch.equal(c.v(), (c.x.double() + c.y.double()).float()), c.what()      # the sum is ONE fp32 rounding
    for dt in DTYPES:
        for c in list(R.ln_const_cases(dt))[::5]:
            assert bool((c.v() == 3).all())
            assert float((c.want() - c.beta.double()).abs().max()) == 0.0, c.what()


def test_split_planes_recombine():
    w = torch.cat([R.randn(4000, seed=1) * 3, torch.tensor([0.0, -0.0, 1e-6, 65503.0, -1e-9])])
    hi, lo = R.split_planes(w)
    back = hi.double() + lo.double() / 2048
    assert float(((back - w.double()).abs() / w.double().abs().clamp(min=2.0 ** -14)).max()) <= 2.0 ** -21


def test_exact_references_are_the_torch_statements():
    tok, pos, start = R.randn(50, 64, seed=1), R.randn(8, 64, seed=2), R.randn(3, 64, seed=3)
    ids = torch.randint(0, 50, (18, 9), generator=R.gen(4), dtype=torch.int32)
    got = R.embed_ref(tok, pos, start, ids, 6, 2, 3, 4, 8.0)
    assert torch.equal(got, tok[ids[::3, 3].long()] / 8.0 + pos[4])
    assert torch.equal(R.embed_ref(tok, pos, None, ids, 6, 2, 3, 4, 8.0), tok[ids[::3, 4].long()] / 8.0 + pos[4])
    assert torch.equal(R.embed_ref(tok, pos, start, None, 6, 2, 3, 0, 8.0), start.repeat_interleave(2, 0) / 8.0 + pos[0])
    s = math.sqrt(520)                                       # a scale that is not an fp32 number: divided by fp32(scale)
    want = ((tok.double() / float(torch.tensor(s, dtype=F32))).float().double() + pos[1].double()).float()
    assert torch.equal(R.embed_ref(tok, pos, None, torch.arange(50, dtype=torch.int32)[:, None].repeat(1, 2), 50, 1, 1, 1, s), want)

    emb, labels = R.randn(20, 33, seed=5), torch.randint(0, 20, (7, 17), generator=R.gen(6))
    assert float((R.label_mean_ref(emb, labels).double() - emb.double()[labels].mean(1)).abs().max()) < 1e-6
    assert torch.equal(R.label_mean_ref(emb, labels[:, :1]), emb[labels[:, 0]])
    x = R.randn(3, 50, 16, seed=7)
    assert float((R.avgpool_seq_ref(x).double() - x.double().mean(1)).abs().max()) < 1e-6
    assert torch.equal(R.avgpool_seq_ref(x[:, :1]), x[:, 0])

    img = R.bytes_image(2, 17, 19, 3, seed=8)
    assert all(len(torch.unique(img[..., ch])) == 256 for ch in range(3))
    mean, std = R.NORM_MEAN[:3], R.NORM_STD[:3]
    tv = img.permute(0, 3, 1, 2).float().div(255).sub_(mean[None, :, None, None]).div_(std[None, :, None, None])   # ToTensor + Normalize
    assert torch.equal(R.normalize_ref(img, mean, std), tv)
    packed = R.pack_nhwc8_ref(tv, BF16)
    assert torch.equal(packed[..., :3], tv.permute(0, 2, 3, 1).to(BF16)) and bool((packed[..., 3:] == 0).all())
    assert torch.equal(R.nhwc_pad_ref(tv, 4)[..., :3], tv.permute(0, 2, 3, 1)) and bool((R.nhwc_pad_ref(tv, 4)[..., 3] == 0).all())
    neg = R.negative(2, 8, 7, 15, seed=9)
    assert bool((neg < 0).all()) and bool((F.max_pool2d(neg, 3, 2, 1) < 0).all())
    assert torch.equal(R.maxpool_ref(neg), F.max_pool2d(F.pad(neg, (1, 1, 1, 1), value=float("-inf")), 3, 2, 0))


def test_mask_rows_and_round16():
    for dt in DTYPES:
        for d in R.MASK_D:
            e, kinds = R.mask_rows(37, d, dt, 0)
            assert set(kinds) == set(R.MASK_KINDS) and R.key_mask_ref(e).tolist() == [bool(R.MASKED[k]) for k in kinds]
            i = kinds.index("subnormal")
            tiny = e[i].float().abs().min()
            assert 0 < float(tiny) < {F32: 1.2e-38, BF16: 1.2e-38, F16: 6.2e-5}[dt] and float(tiny) == float(R.smallest_subnormal(dt).float())
            assert bool(torch.isnan(e[kinds.index("nan")]).any()) and not bool((e[kinds.index("nan")] == 0).any())
            if d > 1:
                z = e[kinds.index("neg_zero")]
                assert int((z == 0).sum()) == 1 and bool(torch.signbit(z[z == 0].float()).all())
    assert float(R.smallest_subnormal(BF16).double()) == 2.0 ** -133 and float(R.smallest_subnormal(F16).double()) == 2.0 ** -24
    x = torch.tensor([0.0, -0.0, 1e-10, -1e-10, 1e-40, -1e-40, 1.0, -3e-8, 2.9e-8, 65504.0])
    for dt in (BF16, F16):
        h = R.round16_keep_nonzero_ref(x, dt)
        assert torch.equal((h == 0), (x == 0)) and torch.equal(torch.signbit(h.float()), torch.signbit(x))
        big = x.to(dt) != 0
        assert torch.equal(h[big], x.to(dt)[big])
        small = ~big & (x != 0)
        assert bool((h[small].float().abs() == R.smallest_subnormal(dt).float()).all())


def test_scoring_references():
    for v, kind, rows, x, t in R.logprob_cases():
        assert x.shape == (rows, v) and bool(((t >= 0) & (t < v)).all()) and bool(torch.isfinite(x.gather(-1, t[:, None])).all())
        want = F.log_softmax(x.double(), -1)[torch.arange(rows), t]
        assert torch.equal(R.logprob_ref(x, t), want)
        if kind == "neg_inf" and v > 1:
            assert bool(torch.isinf(x).any(-1).all())
        if kind == "max_last":
            assert bool((x.argmax(-1) == v - 1).all())
        if kind == "scaled" and v >= 255:
            gone = torch.exp(x - x.max(-1, keepdim=True).values) < 2.0 ** -25      # under half an ulp of the sum's leading 1
            assert float(gone.float().mean()) > 0.5 and bool((torch.exp(x - x.max(-1, keepdim=True).values) == 0).any())
    assert {(v, k) for v, k, *_ in R.logprob_cases()} == set(GR.LP_YARD) == {(v, k) for v in R.LP_V for k in R.LP_KINDS}
    assert {r for _, _, r, *_ in R.logprob_cases()} == {1, 5}
    for L in R.PP_L:
        logp, targets, lengths = R.perplexity_case(L)
        lv = logp.double() / lengths[:, None]
        lv[targets == R.PP_PAD] = 0.0                                          # metrics.perplexity, per sequence
        assert torch.equal(R.perplexity_ref(logp, targets, lengths), (-lv.sum(-1)).exp())
        count = (targets != R.PP_PAD).sum(-1)
        assert int(count[2]) == 1 and (L == 1 or int(lengths[1]) < int(count[1])) and int(count[0]) == L
    assert set(R.PP_L) == set(GR.PP_YARD) and set(R.ROWS_HW) == set(GP.ROWS_YARD)
    assert {(n * c) % 4 for n, c in R.ROWS_NC} == {0, 1, 2, 3}


# ---- the yardsticks behind the gates --------------------------------------------------------------------------------------------
def test_layernorm_yardsticks_are_current():
    now = R.ln_yardsticks()
    fresh(GR.LN_YARD, now)
    assert all(R.YARD_MULT * v <= R.PLAIN_ATOL for k, v in now.items() if k[0] == "plain")
    for dt in (BF16, F16):
        assert all(R.ulp16_gate(R.YARD_MULT * v, dt) <= 1.0 for k, v in now.items() if k[1] == NAME[dt])
    assert R.ulp16_gate(0.0, BF16) == 0.5 and R.ulp16_gate(2.0 ** -16, F16) == 1.5 and R.ulp16_gate(2.0 ** -13, BF16) == 1.5


def test_scoring_and_pool_yardsticks_are_current():
    now = R.logprob_yardsticks()
    assert {k for k, v in GR.LP_YARD.items() if v == 0} == {k for k, v in now.items() if v == 0}      # exact rows: V = 1, log(1)
    fresh({k: v for k, v in GR.LP_YARD.items() if v > 0}, {k: v for k, v in now.items() if v > 0})
    fresh(GR.PP_YARD, R.perplexity_yardsticks())
    fresh(GP.ROWS_YARD, R.avgpool_rows_yardsticks())


@pytest.mark.parametrize("x,want", [(1.0, 2.0 ** -24), (0.75, 2.0 ** -25), (-7.0, 2.0 ** -22), (0.0, 0.0)])
def test_half_ulp(x, want):
    assert R.half_ulp_f32(torch.tensor([x, x / 4])) == want
