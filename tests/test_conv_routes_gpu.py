"""The general convolution kernels -- dh_conv2d_nhwc_bn_act, dh_conv1x1_dual_nhwc, dh_conv2d_nhwc_bn_relu_maxpool (csrc/gemm_bf16.hip)
and the fp32 dh_conv2d_bn_act / dh_stem_conv_nhwc (csrc/conv.hip) -- on every loader, tile route, ring depth, shape edge, epilogue
form and type, against the plain fp64 statement of the operation (conv_ref.py) on the same operands, rounded to the 16-bit type
first.  Every specialised trunk kernel is held bit-identical to these (the ``*_equals_*`` tests of test_bf16_gpu.py and
test_encoder_schedule_cpu.py), so what is checked here is the root of that chain.  The cases, their references and the restated
launcher rules are in conv_ref.py; tests/test_conv_ref_cpu.py checks the references against F.conv2d, every case table against
the route set asserted here, and that in every integer case a dropped K slab or filter tap changes every output tile it reaches.

  route = <loader>_<tile> for dh_conv2d_nhwc_bn_act, dual_<tile> for dh_conv1x1_dual_nhwc, pool for the fused stem
  dense    1x1 stride 1 pad 0: the dense A loader           t128   gemm_bf16_kernel<128, 128>: >= 192 big tiles
  tap      Cin % 64 == 0: incremental (kh, kw, ci)          c256   <256, 64, CONV>: Cout <= 64 and >= 131072 pixels
  generic  k -> (tap, ci) by multiply-shift                 n64    <128, 64>: the same, dense
                                                            r4 r8 r3 r2   64 x 64, ring of 4 / 8 / 3 / 2 slabs
  tm64_k3_vec ...  conv_bn_act_kernel<TM, KS>, 16-byte (Ho Wo % 4 == 0) or per-pixel epilogue; stem_tm64_k7 ...: its 16-bit stem form

Every case runs in two operand flavours.  "int": small integer operands whose every partial sum is exact in fp32 in any order;
the output must EQUAL the exact result (rounded once for 16 bits), which no dropped or doubled slab, stale tap state, wrong
border test or missed epilogue term survives.  "real": randn operands against fp64 -- 16-bit outputs in ulps at
max(|want|, 2^-6), never above 0.75; fp32 outputs by absolute error, never above F32_ATOL = 2e-5.  Both tables hold 1.25 x the
worst error measured on an MI355X over the route's cases (the 1.25 covers another, equally valid accumulation order).  Every
tensor a kernel is given -- inputs, weights, vectors, residual, output -- is a 16-byte-aligned view between 64-element guards
filled with the sentinel 768: a read outside a tensor brings 768 into an exact integer sum, a write outside the output changes
a guard.  Every test prints its worst error per (route, type)."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402
from conv_ref import BF16, DT16, DT16_IDS, F16, F32  # noqa: E402

# 1.25 x the worst error measured on an MI355X over every real-flavour case of the route; check() prints it.
# 16-bit outputs, ulps at max(|want|, 2^-6); keyed by the operands' (= the output's) type:
ULP_GATE = {
    "tap_r2": {BF16: 1.25 * 0.5027, F16: 1.25 * 0.5491},
    "tap_r3": {BF16: 1.25 * 0.5020, F16: 1.25 * 0.5311},
    "tap_r4": {BF16: 1.25 * 0.5045, F16: 1.25 * 0.5406},
    "tap_r8": {BF16: 1.25 * 0.5002, F16: 1.25 * 0.5144},
    "generic_r4": {BF16: 1.25 * 0.5007, F16: 1.25 * 0.5129},
    "generic_r8": {BF16: 1.25 * 0.5010, F16: 1.25 * 0.5110},
    "generic_t128": {BF16: 1.25 * 0.5002, F16: 1.25 * 0.5055},
    "tap_t128": {BF16: 1.25 * 0.5017, F16: 1.25 * 0.5206},
    "dense_n64": {BF16: 1.25 * 0.5013, F16: 1.25 * 0.5099},
    "generic_c256": {BF16: 1.25 * 0.5003, F16: 1.25 * 0.5097},
    "tap_c256": {BF16: 1.25 * 0.5022, F16: 1.25 * 0.5355},
    "dense_r4": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5016},
    "dense_r8": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5099},
    "dual_r2": {BF16: 1.25 * 0.5009, F16: 1.25 * 0.5146},
    "dual_r3": {BF16: 1.25 * 0.5010, F16: 1.25 * 0.5194},
    "dual_r4": {BF16: 1.25 * 0.5008, F16: 1.25 * 0.5241},
    "dual_r8": {BF16: 1.25 * 0.5002, F16: 1.25 * 0.5037},
    "dual_t128": {BF16: 1.25 * 0.5010, F16: 1.25 * 0.5179},
    "pool": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5007},
    "stem_tm128_k3": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5010},
    "stem_tm128_k7": {BF16: 1.25 * 0.5001, F16: 1.25 * 0.5083},
    "stem_tm64_k3": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5003},
    "stem_tm64_k7": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5112},
}
# fp32 outputs (dh_conv2d_bn_act), absolute:
ABS_GATE = {
    "tm128_k1_px": {F32: 1.25 * 7.996e-07},
    "tm128_k1_vec": {F32: 1.25 * 1.050e-06},
    "tm128_k3_px": {F32: 1.25 * 1.192e-06},
    "tm128_k3_vec": {F32: 1.25 * 1.219e-06},
    "tm128_k7_px": {F32: 1.25 * 2.191e-06},
    "tm128_k7_vec": {F32: 1.25 * 1.924e-06},
    "tm64_k1_px": {F32: 1.25 * 7.229e-07},
    "tm64_k1_vec": {F32: 1.25 * 1.186e-06},
    "tm64_k3_px": {F32: 1.25 * 1.095e-06},
    "tm64_k3_vec": {F32: 1.25 * 1.561e-06},
    "tm64_k7_px": {F32: 1.25 * 1.345e-06},
    "tm64_k7_vec": {F32: 1.25 * 1.995e-06},
}
# Conditions on the tables, not measurements: an fp32 result rounded once sits just over 0.5 ulp, a second rounding near 1.0;
# nothing in between may be entered (the dense-linear tests' condition).  AbsGate.check holds every fp32 entry under F32_ATOL.
assert all(v <= 0.75 for row in ULP_GATE.values() for v in row.values())
assert all(v <= R.F32_ATOL for row in ABS_GATE.values() for v in row.values())


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print(f"[test_conv_routes_gpu] module wall time {time.time() - t0:.1f} s")


class Guarded:
    """Device tensors as views between sentinel guards; ``check`` asserts that every guard kept the sentinel."""

    def __init__(self):
        self.bufs = []

    def view(self, shape, dt):
        numel = 1
        for s in shape:
            numel *= s
        buf = torch.full((numel + 2 * R.GUARD,), R.SENTINEL, dtype=dt, device="cuda")
        v = buf[R.GUARD:R.GUARD + numel].view(shape)
        assert v.data_ptr() % 16 == 0 and v.is_contiguous()
        self.bufs.append(buf)
        return v

    def put(self, t):
        if t is None:
            return None
        v = self.view(tuple(t.shape), t.dtype)
        v.copy_(t)
        return v

    def check(self, what):
        for buf in self.bufs:
            assert bool((buf[:R.GUARD] == R.SENTINEL).all()) and bool((buf[-R.GUARD:] == R.SENTINEL).all()), what


def run_case(hip, c):
    """One launch on case ``c``: the output, after the guard checks."""
    g = Guarded()
    out = g.view(c.out_shape, c.out_dt)
    if isinstance(c, R.DualCase):
        hip.conv1x1_dual_nhwc(g.put(c.y), g.put(c.x), g.put(c.w_cat), g.put(c.shift), c.stride, relu=c.relu, out=out)
    elif isinstance(c, R.NchwCase):
        args = (g.put(c.x), g.put(c.wgt), g.put(c.scale), g.put(c.shift))
        if c.stem_dt is not None:
            hip.stem_conv_nhwc(*args, stride=c.stride, pad=c.pad, relu=c.relu, out_dtype=c.stem_dt, out=out)
        else:
            hip.conv2d_bn_act(*args, residual=g.put(c.residual), relu=c.relu, stride=c.stride, pad=c.pad, out=out)
    elif c.pool:
        hip.conv2d_nhwc_bn_relu_maxpool(g.put(c.x), g.put(c.wgt), g.put(c.scale), g.put(c.shift), stride=c.stride, pad=c.pad, out=out)
    else:
        hip.conv2d_nhwc_bn_act(g.put(c.x), g.put(c.wgt), g.put(c.scale), g.put(c.shift), residual=g.put(c.residual), relu=c.relu,
                               stride=c.stride, pad=c.pad, out=out)
    g.check(c.what())
    return out


def run_cases(hip, dt, cases, routes, key=lambda c: c.route):
    """Both flavours of one case table: torch.equal for "int", the route's gate for "real".  Returns {key(c)} over the cases."""
    gates, reached, seen, unequal = R.RouteGates(dt, ULP_GATE, ABS_GATE), set(), set(), []
    for fl in R.FLAVOURS:
        for c in cases(fl):
            reached.add(c.route)
            seen.add(key(c))
            got = run_case(hip, c)
            if fl == "int":
                want = c.want_out()
                if not torch.equal(got.cpu(), want):
                    unequal.append((c.route, c.what(), int((got.cpu() != want).sum())))
            else:
                gates.add(c.route, got, c.want(), c.what(), c.out_dt == F32)
    assert not unequal, unequal
    assert reached == routes, sorted(reached)
    gates.check()
    return seen


def run_table(hip, dt, name, key=lambda c: c.route):
    cases, routes = R.ROUTES_A[name]
    return run_cases(hip, dt, lambda fl: cases(dt, fl), routes, key)


# ---- A. dh_conv2d_nhwc_bn_act ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_ring_switches(hip, dt):
    """The CONV kernel (1x1 stride 2, Cin 192) at workgroup counts on both sides of each switch of the ring depth (320 | 321,
    512 | 513, 768 | 769, 1280 | 1281); and r4 for its other reason, K <= 128 (Cin 64, a single slab), at a count that gives r8."""
    seen = run_table(hip, dt, "ring_switch", lambda c: (c.blocks, c.tile))
    assert seen == {want for _, want in R.RING_SWITCH}, sorted(seen)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_tap_loader_against_ring_depth(hip, dt):
    """The tap-uniform loader on each ring depth NS: 3x3 with Cin 64 / 128 / 256 and 2x2 with Cin 64 / 128 (the tap changes every
    slab, every second, every fourth: the incremental state crosses the prologue | loop boundary at every position), 1x1 stride 2
    with NS - 2 .. NS + 1 and 2 NS + 1 slabs, and one long reduction (Cin 512, 3x3, 7 x 9: K = 4608)."""
    seen = run_table(hip, dt, "tap", lambda c: (c.tile, c.ks, c.nslab))
    assert {(r, 1, s) for r in R.NS for s in R.tap_slab_counts(r)} <= seen and ("r8", 3, 72) in seen
    assert {(r, ks, s) for r in R.NS for ks, s in ((3, 9), (3, 18), (2, 4), (2, 8))} <= seen


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_generic_loader(hip, dt):
    """Cin 8 / 16 / 24 / 40 x KS 2 / 3 / 5 / 7 with strides 1 and 2 and pads 0, 1, 3 (one pad >= KS): K % 64 != 0 (the
    non-stepping W loader) and == 0."""
    seen = run_table(hip, dt, "generic", lambda c: (c.cin, c.ks))
    assert seen == {(ci, ks) for ci in R.GENERIC_CIN for ks in R.GENERIC_KS}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_big_tiles(hip, dt):
    """The 128 x 128 kernel at exactly 192 tiles with the tap and the generic loader, in both tile orders (n_fast 0 and 1, its
    activation bytes counted as 2 M Cin); 191 tiles, M = 95 and N = 95 fall back to the rings."""
    seen = run_table(hip, dt, "big_tiles", lambda c: (c.route, c.n_fast) if c.tile == "t128" else c.route)
    assert seen == {("tap_t128", 0), ("tap_t128", 1), ("generic_t128", 0), "tap_r3", "tap_r4"}, seen


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_narrow(hip, dt):
    """Cout <= 64: the 256 x 64 CONV kernel at 131072 pixels (generic) and 131712 (tap), a ring at 131064; the dense 1x1 on the
    128 x 64 kernel."""
    run_table(hip, dt, "narrow")


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_shape_edges(hip, dt):
    """1 .. 130 output pixels (1 x 1 maps, maps smaller than the filter reach, images that share a 64-row tile) x Cout 8 .. 130
    (60: the element-wise epilogue; 68: a partial last chunk inside the 16-byte path; 130: scalar scale / shift loads) x the
    three loaders."""
    seen = run_table(hip, dt, "edges", lambda c: (c.m, c.cout))
    assert {(m, co) for m in (1, 63, 64, 65, 130) for co in R.EDGE_COUT} <= seen


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_epilogue_forms(hip, dt):
    """Affine, + residual, + relu, all, on a 16-byte Cout and on Cout = 60, with each loader."""
    seen = run_table(hip, dt, "forms", lambda c: (c.form, c.cout))
    assert seen == {(f, co) for f in R.FORM_NAMES for co in R.FORM_COUT}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_refusals(hip, dt):
    """Cin = 1000, KS = 3: no exact multiplier for k / 1000 below 9000 -- the launcher must refuse, not compute."""
    for c in R.refusal_cases(dt):
        assert not R.accepted(c.cin, c.ks)
        g = Guarded()
        out = g.view(c.out_shape, c.out_dt)
        with pytest.raises(RuntimeError):
            hip.conv2d_nhwc_bn_act(g.put(c.x), g.put(c.wgt), g.put(c.scale), g.put(c.shift), relu=c.relu, stride=c.stride, pad=c.pad, out=out)
        torch.cuda.synchronize()
        assert bool((out == R.SENTINEL).all()), c.what()
        g.check(c.what())


# ---- B. dh_conv1x1_dual_nhwc ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_dual_source(hip, dt):
    """[y | x at the strided pixels] on each ring depth NS with C1 / 64 in {1, NS - 2, NS - 1, NS} (the switch to the second
    source in the prologue, on its last slab, inside the loop), C2 64 / 256, stride 1 and 2 on odd maps, a wider x than the
    stride needs, partial M and N tiles, relu on and off; the 128 x 128 kernel once per stride."""
    seen = run_cases(hip, dt, lambda fl: R.dual_cases(dt, fl), R.ROUTES_DUAL, lambda c: (c.tile, c.c1 // 64))
    assert {(r, s) for r in R.NS for s in R.dual_c1_slabs(r)} <= seen, sorted(seen)


# ---- C. dh_conv2d_nhwc_bn_relu_maxpool ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_conv_with_fused_maxpool(hip, dt):
    """Cin 8, 7x7 / 2 / 3 (and 3x3 / 1 / 1), Cout 8 / 40 / 64, pooled maps of 1 x 1, 7 x 7, 8 x 7, 7 x 15 and 16 x 12 (one 7 x 7
    block, an exact one, a one-row spill, partial blocks in both directions), two and three images."""
    seen = run_cases(hip, dt, lambda fl: R.pool_cases(dt, fl), {"pool"}, lambda c: c.out_shape[1:3])
    assert seen == set(R.POOL_MAPS)


# ---- D. dh_conv2d_bn_act, fp32 ----------------------------------------------------------------------------------------------------
def test_f32_conv(hip):
    """conv_bn_act_kernel<64 | 128, 1 | 3 | 7>: Cout 60 / 64 / 130, Ho Wo % 4 == 0 and odd (7 x 7: a thread's four pixels straddle
    two images), P % 128 != 0, K % 16 != 0 (Cin 3, 7x7: K = 147), stride 2 on odd sizes, with and without residual and relu."""
    run_cases(hip, F32, R.f32_cases, R.ROUTES_F32)


# ---- E. dh_stem_conv_nhwc ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_stem_conv(hip, dt):
    """fp32 NCHW image in, channels-last 16-bit out: KS 7 and 3, Cout 4 / 64 / 132."""
    run_cases(hip, dt, lambda fl: R.stem_cases(dt, fl), R.ROUTES_STEM)
