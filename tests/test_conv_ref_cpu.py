"""The general-convolution tests' own references and case tables (conv_ref.py), checked without a GPU: the fp64 references against
F.conv2d (+ F.max_pool2d) in double, every case table against the route set its GPU test asserts (from the restated launcher
rules alone), the restated magic() check on every generic case and on the refusals, the integer flavour's premise, and its
sensitivity: zeroing any one 64-wide K slab (16-wide for the fp32 kernel) or any one filter tap changes at least one element of
every 64 x 64 output tile that the dropped weights reach -- so a kernel that dropped, doubled or mixed up a slab or a tap cannot
pass torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from conv_ref import BF16, DT16, F16, F32

MAX_SENSITIVITY_OUTPUTS = 1 << 21
MAX_SENSITIVITY_WORK = 1 << 33                               # outputs x K x masks


def rnd64(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float64)


def test_conv_ref_equals_f_conv2d():
    g = torch.Generator().manual_seed(0)
    x, w, scale, shift = rnd64(g, 2, 9, 7, 16), rnd64(g, 12, 3, 3, 16), rnd64(g, 12), rnd64(g, 12)
    xc, wc = x.permute(0, 3, 1, 2).contiguous(), w.permute(0, 3, 1, 2).contiguous()
    for stride, pad in ((1, 1), (2, 0), (2, 3)):
        bare = F.conv2d(xc, wc, stride=stride, padding=pad)
        res = rnd64(g, *bare.shape)
        want = torch.relu(bare * scale[None, :, None, None] + shift[None, :, None, None] + res)
        got = R.conv_ref(x, w, scale, shift, res.permute(0, 2, 3, 1), True, stride, pad)
        assert torch.allclose(got.permute(0, 3, 1, 2), want, atol=1e-12, rtol=0) and bool((want == 0).any()) and bool((want > 0).any())
        got = R.conv_ref(x, w, scale, shift, None, False, stride, pad)
        assert torch.allclose(got.permute(0, 3, 1, 2), bare * scale[None, :, None, None] + shift[None, :, None, None], atol=1e-12, rtol=0)
        assert torch.allclose(R.conv_nchw_ref(xc, wc, scale, shift, res, True, stride, pad), want, atol=1e-12, rtol=0)
    x = rnd64(g, 2, 27, 28, 8)
    w = rnd64(g, 12, 7, 7, 8)
    want = F.max_pool2d(torch.relu(F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=2, padding=3) * scale[None, :, None, None]
                                   + shift[None, :, None, None]), 3, 2, 1)
    got = R.conv_pool_ref(x, w, scale, shift, 2, 3)
    assert got.shape == (2, 7, 7, 12) and torch.allclose(got.permute(0, 3, 1, 2), want, atol=1e-12, rtol=0)


def test_dual_ref_equals_two_convolutions():
    g = torch.Generator().manual_seed(1)
    for stride, (h, w) in ((1, (5, 7)), (2, (9, 13)), (2, (10, 14)), (1, (7, 8))):
        y, x, w_cat, shift = rnd64(g, 2, 5, 7, 8), rnd64(g, 2, h, w, 24), rnd64(g, 12, 32), rnd64(g, 12)
        want = F.conv2d(y.permute(0, 3, 1, 2), w_cat[:, :8, None, None]) + shift[None, :, None, None]
        want = want + F.conv2d(x.permute(0, 3, 1, 2), w_cat[:, 8:, None, None], stride=stride)[:, :, :5, :7]
        got = R.dual_ref(y, x, w_cat, shift, stride, False)
        assert torch.allclose(got.permute(0, 3, 1, 2), want, atol=1e-12, rtol=0)
        assert torch.allclose(R.dual_ref(y, x, w_cat, shift, stride, True), torch.relu(got))


def test_cases_state_their_references():
    """The cases' own ``want`` (cached accumulators, layouts) is the plain reference on their operands."""
    for fl in R.FLAVOURS:
        c = R.ConvCase(F16, fl, 2, 9, 25, 24, 60, 3, 2, 1, "all", seed=1)
        assert torch.allclose(c.want(), R.conv_ref(c.x, c.wgt, c.scale, c.shift, c.residual, True, 2, 1), atol=1e-12, rtol=0)
        c = R.ConvCase(BF16, fl, 2, 27, 28, 8, 40, 7, 2, 3, pool=True)
        assert c.want().shape == c.out_shape and torch.allclose(c.want(), R.conv_pool_ref(c.x, c.wgt, c.scale, c.shift, 2, 3), atol=1e-12, rtol=0)
        c = R.DualCase(BF16, fl, 2, 9, 14, 128, 64, 2, 72, True, extra_hw=(2, 1))
        assert (c.h, c.w) == (19, 28) and torch.allclose(c.want(), R.dual_ref(c.y, c.x, c.w_cat, c.shift, 2, True), atol=1e-12, rtol=0)
        c = R.NchwCase(fl, 3, 5, 13, 14, 60, 3, 2, 1, "all")
        assert torch.allclose(c.want(), R.conv_nchw_ref(c.x, c.wgt, c.scale, c.shift, c.residual, True, 2, 1), atol=1e-12, rtol=0)
        c = R.NchwCase(fl, 2, 3, 17, 22, 64, 7, 2, 3, "relu", stem_dt=F16)
        assert torch.allclose(c.want(), R.conv_nchw_ref(c.x, c.wgt, c.scale, c.shift, None, True, 2, 3).permute(0, 2, 3, 1), atol=1e-12, rtol=0)
        assert c.x.dtype == F32 and c.out_dt == F16 and c.out_shape == (2, 9, 11, 64)


def test_route_mirrors():
    """The rules at their thresholds."""
    assert R.loader(64, 1, 1, 0) == "dense" and R.loader(64, 1, 2, 0) == "tap" and R.loader(64, 1, 1, 1) == "tap"
    assert R.loader(8, 1, 1, 0) == "dense" and R.loader(72, 3, 1, 1) == "generic" and R.loader(128, 3, 1, 1) == "tap"
    assert R.tile(3072, 1024, 576, True) == "t128" and R.tile(95, 128 * 192, 576, True) == "r3" and R.tile(128 * 192, 95, 576, True) == "r3"
    assert R.tile(128, 128 * 191, 576, True) == "r3"
    assert R.tile(131072, 64, 72, True) == "c256" and R.tile(131072, 64, 64, False) == "n64"
    assert R.tile(131071, 64, 72, True) == "r4" and R.tile(131072, 65, 72, True) == "r4"
    assert [R.tile(64 * b, 64, 192, True) for b in (320, 321, 512, 513, 768, 769, 1280, 1281)] == ["r8", "r4", "r4", "r3", "r3", "r2", "r2", "r4"]
    assert R.tile(64 * 600, 64, 128, True) == "r4" and R.tile(64 * 600, 64, 136, True) == "r3"
    # a_bytes counts the input's channels once on the CONV path: 3x3 Cin 64, M = 3069 against N = 1024 rows of 576
    assert R.n_fast(3069, 1024, 576, 64, True) == 0 and R.n_fast(3069, 1024, 576, 64, False) == 1
    assert R.n_fast(3069, 1016, 192, 192, True) == 1 and R.n_fast(100000, 8192, 1024, 1024, True) == 0
    assert R.f32_route(127, 1, 6, 10) == "tm64_k1_vec" and R.f32_route(128, 7, 7, 7) == "tm128_k7_px"
    assert R.f32_route(4, 3, 9, 11, stem=True) == "stem_tm64_k3" and R.f32_route(132, 7, 9, 11, stem=True) == "stem_tm128_k7"


def test_magic_accepts_the_generic_cases_and_rejects_the_refusals():
    assert R.magic(8, 392) == 131072 and R.magic(7, 49) == 149797 and R.magic(24, 24 * 49) == 43691
    # k / 1000 for k < 9000: mg = 1049, and 2999 * 1049 >> 20 = 3
    assert R.magic(1000, 9000) == 0 and (2999 * 1049) >> 20 == 3 and R.magic(1000, 2999) == 1049
    assert R.magic(3, 1 << 14) == 0                           # limit * mg >= 2^32
    for cin, ks in R.REFUSED:
        assert cin % 8 == 0 and not R.accepted(cin, ks)       # refused by the magic check, not by Cin % 8
    assert [c.route for c in R.refusal_cases(BF16)] == ["generic_r8"]
    n_generic = 0
    for name, (cases, _) in R.ROUTES_A.items():
        for c in cases(BF16, "int"):
            assert R.accepted(c.cin, c.ks), (name, c.what())
            n_generic += c.loader == "generic"
    assert n_generic > 100 and all(R.accepted(c.cin, c.ks) for c in R.pool_cases(BF16, "int"))
    assert not R.accepted(12, 3) and R.accepted(1024, 3)


def is_listed_square(c):
    return (c.n, c.h, c.w) in R.SQUARE


@pytest.mark.parametrize("fl", R.FLAVOURS)
def test_case_tables_reach_their_routes(fl):
    """What every GPU test asserts with ``==``, from the mirrors alone."""
    for dt in DT16:
        for name, (cases, routes) in R.ROUTES_A.items():
            cs = list(cases(dt, fl))
            assert {c.route for c in cs} == routes, name
            assert all(c.h != c.w or is_listed_square(c) for c in cs), name
            assert all(c.h % 2 and c.w % 2 for c in cs if c.stride == 2), name      # stride 2 on odd sizes
        assert {c.route for c in R.dual_cases(dt, fl)} == R.ROUTES_DUAL
        assert {c.route for c in R.pool_cases(dt, fl)} == {"pool"}
        assert {c.route for c in R.stem_cases(dt, fl)} == R.ROUTES_STEM
    assert {c.route for c in R.f32_cases(fl)} == R.ROUTES_F32
    for cases in (R.dual_cases(BF16, fl), R.pool_cases(BF16, fl), R.stem_cases(BF16, fl), R.f32_cases(fl)):
        assert all(c.h != c.w for c in cases)
    dt = BF16
    # A1: both sides of every switch, K > 128, and r4 for its other reason
    cs = list(R.ring_switch_cases(dt, fl))
    assert [(c.blocks, c.tile) for c in cs] == [want for _, want in R.RING_SWITCH]
    assert all(c.loader == "tap" and c.ks == 1 and c.stride == 2 for c in cs) and [c.k for c in cs] == [192] * 8 + [64]
    # A2: every ring depth with NS - 2 .. NS + 1 and 2 NS + 1 slabs, and with the tap changing every slab / second / fourth slab
    seen = {}
    for c in R.tap_cases(dt, fl):
        assert c.loader == "tap"
        seen.setdefault(c.tile, set()).add((c.ks, c.nslab))
    for route, ns in R.NS.items():
        counts = {s for ks, s in seen[route] if ks == 1}
        assert counts == set(R.tap_slab_counts(route)) and {ns + 1, 2 * ns + 1} <= counts, route
        assert {(3, 9), (3, 18), (2, 4), (2, 8)} <= seen[route], route
    assert R.tap_slab_counts("r4") == [2, 3, 4, 5, 9] and R.tap_slab_counts("r8") == [6, 7, 8, 9, 17]
    assert R.tap_slab_counts("r3") == [3, 4, 7] and R.tap_slab_counts("r2") == [3, 5]
    assert (3, 36) in seen["r8"] and (3, 36) in seen["r4"] and (3, 72) in seen["r8"]
    # A3
    cs = list(R.generic_cases(dt, fl))
    assert {(c.cin, c.ks) for c in cs} >= {(ci, ks) for ci in R.GENERIC_CIN for ks in R.GENERIC_KS}
    assert {c.k % 64 == 0 for c in cs} == {True, False} and any(c.k == 392 for c in cs) and any(c.pad >= c.ks for c in cs)
    assert {c.stride for c in cs} == {1, 2} and {c.pad for c in cs} == {0, 1, 3} and all(c.loader == "generic" for c in cs)
    # A4: exactly 192 big tiles in both tile orders; one step below on each condition
    cs = list(R.big_tile_cases(dt, fl))
    big = [c for c in cs if c.tile == "t128"]
    assert {R.cdiv(c.m, 128) * R.cdiv(c.cout, 128) for c in big} == {192} and {c.n_fast for c in big} == {0, 1}
    assert {(R.cdiv(c.m, 128), R.cdiv(c.cout, 128)) for c in big} == {(24, 8), (8, 24)}
    rest = [(c.m, c.cout, R.cdiv(c.m, 128) * R.cdiv(c.cout, 128)) for c in cs if c.tile != "t128"]
    assert [r[2] for r in rest] == [191, 192, 195] and rest[1][0] == 95 and rest[2][1] == 95
    # A5
    cs = list(R.narrow_cases(dt, fl))
    assert [(c.m, c.route) for c in cs] == [(131072, "generic_c256"), (131712, "tap_c256"), (131064, "generic_r4"), (131072, "dense_n64")]
    # A6
    cs = list(R.edge_cases(dt, fl))
    assert len(cs) == 150 and [c.m for c in cs[::15]] == [m for _, m in R.EDGE_MAPS] and {1, 63, 64, 65, 130} <= {c.m for c in cs}
    assert {c.cout for c in cs} == set(R.EDGE_COUT) and any(c.ho == c.wo == 1 for c in cs) and any(c.h < c.ks - c.pad for c in cs)
    # A7
    cs = list(R.form_cases(dt, fl))
    assert {(c.form, c.cout % 8 == 0, c.loader) for c in cs} == {(f, a, ld) for f in R.FORM_NAMES for a in (True, False) for ld in ("tap", "generic", "dense")}
    # B: per ring, the second source starts in the prologue, on its last slab and inside the loop; both widths, both strides
    cs = list(R.dual_cases(dt, fl))
    seen = {(c.tile, c.c1 // 64) for c in cs}
    assert seen >= {(r, s) for r in R.NS for s in R.dual_c1_slabs(r)} and R.dual_c1_slabs("r8") == [1, 6, 7, 8] and R.dual_c1_slabs("r2") == [1, 2]
    for r in R.NS:
        assert {(c.c2, c.stride) for c in cs if c.tile == r} >= {(64, 2), (256, 1)} and {c.relu for c in cs if c.tile == r} == {True, False}, r
    assert all(c.m % 64 and c.cout % 64 for c in cs if c.tile != "t128") and all((c.ho - 1) * c.stride < c.h for c in cs)
    assert all(c.h % 2 and c.w % 2 for c in cs if c.stride == 2 and c.h == 2 * c.ho - 1) and any(c.h > (c.ho - 1) * c.stride + 1 for c in cs)
    assert sum(c.tile == "t128" for c in cs) == 2
    # C
    cs = list(R.pool_cases(dt, fl))
    assert {c.out_shape[1:3] for c in cs} == set(R.POOL_MAPS) and {c.cout for c in cs} == set(R.POOL_COUT) and {c.n for c in cs} == {2, 3}
    assert {(c.ks, c.stride, c.pad) for c in cs} == {(7, 2, 3), (3, 1, 1)} and all(c.cin % 8 == 0 and c.cout % 8 == 0 and c.cout <= 64 for c in cs)
    # D
    cs = list(R.f32_cases(fl))
    assert {c.cout for c in cs} == {60, 64, 130} and {c.k % 16 == 0 for c in cs} == {True, False} and any(c.k == 147 for c in cs)
    assert any(c.ho == c.wo == 7 and c.n > 1 for c in cs) and all(c.m % 128 for c in cs) and any(c.m > 256 for c in cs)
    assert {(c.form, c.route[:4]) for c in cs} >= {(f, t) for f in R.FORM_NAMES for t in ("tm64", "tm12")}
    assert any(c.stride == 2 and c.h % 2 and c.w % 2 for c in cs)
    # E
    cs = list(R.stem_cases(dt, fl))
    assert {(c.ks, c.cout) for c in cs} == {(ks, co) for ks in (7, 3) for co in (4, 64, 132)} and all(c.cout % 4 == 0 for c in cs)


def int_cases():
    """Every integer case once: its operands do not depend on the 16-bit type."""
    for name, (cases, _) in R.ROUTES_A.items():
        for c in cases(BF16, "int"):
            yield name, c
    for name, cases in (("dual", R.dual_cases), ("pool", R.pool_cases), ("stem", R.stem_cases)):
        for c in cases(BF16, "int"):
            yield name, c
    for c in R.f32_cases("int"):
        yield "f32", c


def operands(c):
    if isinstance(c, R.DualCase):
        return ((c.y, 3), (c.x, 3), (c.w_cat, 3), (c.shift, 8))
    return ((c.x, 3), (c.wgt, 3), (c.shift, 8), (c.residual, 8))


def test_integer_cases_keep_their_premise():
    """Entries are integers exactly representable in every type, scale is a power of two, and (9 K) * scale + |shift| + |res|
    stays below 2^24: every partial result is exact in fp32 in any order, so the fp32 CPU convolution that builds the expectation
    is exact too (checked against fp64 here).  The results themselves lie inside fp16's range."""
    n_cases = 0
    for name, c in int_cases():
        assert c.flavour == "int" and 9 * c.k * 2 + 16 < 2 ** 24, (name, c.what())
        if c.m * c.cout > MAX_SENSITIVITY_OUTPUTS:            # the few big ones draw from the same code
            continue
        n_cases += 1
        for x, lim in operands(c):
            if x is None:
                continue
            assert float(x.double().abs().max()) <= lim and torch.equal(x.double(), x.double().round()), (name, c.what())
            for dt in DT16:
                assert torch.equal(x.double(), x.to(dt).double())
        if not isinstance(c, R.DualCase):
            assert set(c.scale.tolist()) <= {0.5, 1.0, 2.0}
        want = c.want()
        assert float(want.abs().max()) <= min(9.0 * c.k * 2 + 16, 65504.0) and torch.equal(want * 2, (want * 2).round()), (name, c.what())
        if isinstance(c, R.DualCase):
            exact = R.dual_ref(c.y, c.x, c.w_cat, c.shift, c.stride, c.relu)
        elif isinstance(c, R.NchwCase):
            exact = R.conv_nchw_ref(c.x, c.wgt, c.scale, c.shift, c.residual, c.relu, c.stride, c.pad)
            exact = exact.permute(0, 2, 3, 1) if c.stem_dt is not None else exact
        elif c.pool:
            exact = R.conv_pool_ref(c.x, c.wgt, c.scale, c.shift, c.stride, c.pad)
        else:
            exact = R.conv_ref(c.x, c.wgt, c.scale, c.shift, c.residual, c.relu, c.stride, c.pad)
        assert torch.equal(want, exact), (name, c.what())
        assert c.out_dt != F32 or torch.equal(c.want_out().double(), want)
    assert n_cases > 250


def test_a_dropped_slab_or_tap_is_visible():
    """For every integer case of moderate size: zeroing the weights of any one K slab (the tail included) or of any one filter tap
    changes, in the output's own type, at least one element of every 64 x 64 tile of the [pixels, channels] output in which
    those weights meet the image at all (a border tap lies in the padding for some pixels; on a 1 x 1 map, for all but one)."""
    n_cases = n_masks = n_tiles = 0
    for name, c in int_cases():
        masks = list(c.slab_masks())
        if c.m * c.cout > MAX_SENSITIVITY_OUTPUTS or c.m * c.cout * c.k * len(masks) > MAX_SENSITIVITY_WORK:
            continue
        n_cases += 1
        want = R.as_rows(c, c.want_out())
        rows, cols = want.shape
        tm, tn = R.cdiv(rows, 64), R.cdiv(cols, 64)
        for what, mask in masks:
            n_masks += 1
            changed, live = torch.zeros(2, tm * 64, tn * 64, dtype=torch.bool)
            changed[:rows, :cols] = R.as_rows(c, c.want(drop=mask).to(c.out_dt)) != want
            live[:rows, :cols] = R.as_rows(c, c.live(mask))
            changed, live = (t.view(tm, 64, tn, 64).any(3).any(1) for t in (changed, live))
            n_tiles += int(live.sum())
            assert bool((changed | ~live).all()), (name, c.what(), what, int((live & ~changed).sum()))
            assert not bool((changed & ~live).any()), (name, c.what(), what)
    print(f"[sensitivity] {n_cases} integer cases, {n_masks} slabs and taps, {n_tiles} tiles")
    assert n_cases > 250 and n_masks > 2000
