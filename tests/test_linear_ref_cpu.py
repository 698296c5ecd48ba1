"""The dense-linear tests' own reference and case tables (linear_ref.py), checked without a GPU: the fp64 references against
F.linear / F.layer_norm, every case set against the route set its GPU test asserts (from the restated launcher rules alone, so
a typo in a shape is found here), the integer flavour's premise, and its sensitivity: zeroing any one K slab of the operands,
or the K tail, changes at least one element of every 64 x 64 output tile -- so a kernel that dropped, doubled or mixed up a
slab cannot pass torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import linear_ref as R
from linear_ref import BF16, DT16, DT16_IDS, F16, F32

MAX_SENSITIVITY_OUTPUTS = 1 << 22


def test_linear_ref_equals_f_linear():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)    # noqa: E731
    a, w, bias, scale, shift, res = rnd(7, 24), rnd(13, 24), rnd(13), rnd(13), rnd(13), rnd(7, 13)
    assert torch.allclose(R.linear_ref(a, w, bias), F.linear(a, w, bias), atol=1e-13, rtol=0)
    assert torch.allclose(R.linear_ref(a, w), F.linear(a, w), atol=1e-13, rtol=0)
    want = torch.relu(F.linear(a, w, bias) * scale + shift + res)
    assert torch.allclose(R.linear_ref(a, w, bias, scale, shift, res, True), want, atol=1e-13, rtol=0)
    assert bool((want == 0).any()) and bool((want > 0).any())
    assert torch.allclose(R.linear_ref(a, w, None, scale, shift, res), F.linear(a, w) * scale + shift + res, atol=1e-13, rtol=0)


def test_linear_ln_ref_equals_layer_norm_plus_linear():
    """Both sides, with the fold done exactly (fp64 weights), and the per-tile statistics."""
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)    # noqa: E731
    m, k, n = 9, 128, 64
    y, gamma, beta, w, b = rnd(m, k) * 1.7 + 0.3, rnd(k).abs() + 0.5, rnd(k) * 0.2, rnd(n, k) / k ** 0.5, rnd(n)
    want = F.linear(F.layer_norm(y, (k,), gamma, beta, R.LN_EPS), w, b)
    got = R.linear_ln_ref(y, w * gamma[None, :], b + w @ beta, a_eps=R.LN_EPS)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    res, g2, b2, a = rnd(m, n) * 1.7 + 0.3, rnd(n).abs() + 0.5, rnd(n) * 0.2, rnd(m, k)
    want = torch.relu(F.layer_norm(res, (n,), g2, b2, R.LN_EPS) + F.linear(a, w, b))
    assert torch.allclose(R.linear_ln_ref(a, w, b, res, True, r_ln=(R.LN_EPS, g2, b2)), want, atol=1e-12, rtol=0)
    assert torch.allclose(R.linear_ln_ref(a, w, b, res), res + F.linear(a, w, b), atol=1e-12, rtol=0)
    st = R.tile_stats(y)
    assert st.shape == (m, 2, 2)
    assert torch.allclose(st[:, 1, 0], y[:, 64:].mean(1)) and torch.allclose(st[:, 1, 1], y[:, 64:].var(1, unbiased=False) * 64)


def test_route_mirrors():
    """The rules at their thresholds."""
    assert [R.ring_route(b, 256) for b in (1, 320, 321, 512, 513, 768, 769, 1280, 1281)] == ["r8", "r8", "r4", "r4", "r3", "r3", "r2", "r2", "r4"]
    assert [R.ring_route(b, 128) for b in (1, 600, 1000)] == ["r4"] * 3 and R.ring_route(600, 136) == "r3"
    assert R.route16(3072, 1024, 64) == "t128" and R.route16(3072, 1024, 64, ln=True) == "r4"
    assert R.route16(95, 128 * 192, 256) == "r3" and R.route16(128 * 192, 95, 256) == "r3" and R.route16(128, 128 * 191, 256) == "r3"
    assert R.route16(131072, 64, 64) == "n64" and R.route16(131072, 65, 64) == "r4" and R.route16(131071, 64, 64) == "r4"
    pers = dict(out_f32=True, ldc=4160)
    assert R.route16(4096, 4097, 128, **pers) == "pers" and R.route16(4096, 4097, 128, ldc=4160) == "t128"
    assert R.route16(4096, 4097, 64, **pers) == "t128" and R.route16(4096, 4097, 136, **pers) == "t128"
    assert R.route16(4096, 4097, 128, out_f32=True, ldc=4097) == "t128"
    assert R.route16(4096, 4097, 128, c_aligned=False, **pers) == "t128"
    assert R.route16(4096, 4097, 128, plain_epilogue=False, **pers) == "t128" and R.route16(3968, 4097, 128, **pers) == "t128"
    assert R.route32(3072, 1024) == "t128" and R.route32(95, 128 * 192) == "t64" and R.route32(128 * 192, 95) == "t128"
    assert R.route32(128, 128 * 191) == "t64"
    assert R.n_fast(3067, 1021, 520) == 1 and R.n_fast(1019, 3069, 520) == 0 and R.n_fast(100000, 8192, 1024) == 0
    assert R.wrapper_ldc(BF16, 4096, 4097, True) == 4160 and R.wrapper_ldc(BF16, 4096, 4097, False) == 4097
    assert R.wrapper_ldc(BF16, 4095, 4097, True) == 4097 and R.wrapper_ldc(F32, 4096, 4097, False) == 4097


@pytest.mark.parametrize("fl", R.FLAVOURS)
def test_case_sets_reach_their_routes(fl):
    """What every GPU test asserts with ``==``, from the mirrors alone."""
    for dt in DT16:
        for name, (cases, routes) in R.CASE_SETS.items():
            assert {c.route for c in cases(dt, fl)} == routes, name
    for name, (cases, routes) in R.CASE_SETS32.items():
        assert {c.route for c in cases(fl)} == routes, name
    cases = list(R.ring_switch_cases(BF16, fl))
    assert [(c.blocks, c.route) for c in cases] == [want for _, want in R.RING_SWITCH]
    assert all(c.m % 64 and c.k in (128, 192, 256) for c in cases)
    assert {(c.blocks > 320, c.k <= 128) for c in cases if c.route == "r4"} == {(True, False), (False, True)}     # both reasons
    # slabs: every ring depth with fewer slabs than it holds (where K > 128 allows), as many, one more, and over two turns
    seen = {}
    for c in R.slab_cases(F16, fl):
        seen.setdefault(c.route, set()).add((R.cdiv(c.k, 64), c.k % 64 == 0))
    assert seen == {r: {(s, st) for s in R.slab_counts(r) for st in (True, False)} for r in R.NS}
    assert R.slab_counts("r4") == [1, 2, 3, 4, 5, 9] and R.slab_counts("r8") == [3, 6, 7, 8, 9, 17]
    assert R.slab_counts("r3") == [3, 4, 7] and R.slab_counts("r2") == [3, 5]
    assert {c.k % 64 for c in R.slab_cases(F16, fl)} == {0, 8, 56}
    big = [c for c in R.big_tile_cases(BF16, fl) if c.route == "t128"]
    assert {R.cdiv(c.m, 128) * R.cdiv(c.n, 128) for c in big} == {192} and {R.n_fast(c.m, c.n, c.k) for c in big} == {0, 1}
    assert {c.k for c in big} == set(R.BIG_TILE_K) and all(R.cdiv(c.m, 128) != R.cdiv(c.n, 128) for c in big)
    assert [c.route for c in R.narrow_cases(BF16, fl)] == ["n64", "r4", "n64", "r4"]
    assert [c.route for c in R.persistent_cases(BF16, fl)] == ["pers", "pers", "pers", "t128", "t128", "t128", "t128"]
    assert next(R.persistent_cases(BF16, fl)).ldc == 4160
    assert [c.route for c in R.f32_big_tile_cases(fl)] == ["t128"] * 4 + ["t64"] * 2
    for dt in DT16:
        assert sum(1 for _ in R.edge_cases(dt, fl)) == 150 and sum(1 for _ in R.form_cases(dt, fl)) == 3 * 6 * 2 * 3
        # 16-bit epilogue paths: 16-byte, element-wise by stride, partial last chunk, scalar bias loads
        assert {(c.ldc % 8 == 0, c.ldres % 8 == 0) for c in R.form_cases(dt, fl) if not c.out_f32} == {(True, True), (False, True), (True, False)}
        assert {c.ldc % 4 == 0 for c in R.form_cases(dt, fl) if c.out_f32} == {True, False}
        assert all(c.lda > c.k and c.ldw > c.k and c.lda % 8 == 0 and c.ldw % 8 == 0 for c in R.form_cases(dt, fl))
        assert all(c.ldc % 8 == 0 and c.ldres % 8 == 0 and not (c.c_aligned and c.res_off == 0) for c in R.align_cases(dt, fl))
    assert sum(1 for _ in R.edge_cases(F32, fl)) == 150 and all(c.k % 4 == 0 and c.lda % 4 == 0 for c in R.edge_cases(F32, fl))


def test_ln_case_tables():
    a, r = list(R.ln_a_cases(BF16)), list(R.ln_r_cases(F16))
    assert [(c.blocks, c.route) for c in a] == [want for _, want in R.LN_A_SHAPES]
    assert [(c.blocks, c.route) for c in r] == [want for _, want in R.LN_R_SHAPES]
    for cases in (a, r):
        assert {c.route for c in cases} == {"r8", "r4", "r3", "r2"}
        assert {(c.blocks > 1280, 320 < c.blocks <= 512, c.k <= 128) for c in cases if c.route == "r4"} == {
            (True, False, False), (False, True, False), (False, False, True)}
        assert all(c.m % 64 for c in cases)
    assert {c.k for c in a} == {128, 256, 384, 512} and {c.n for c in a} == {512, 1536, 2048} and {c.n for c in r} == {128, 512}
    assert len(R.LN_R_FORMS) == 8
    c = R.LnCase(BF16, 1, 37, 512, 128)
    assert c.w.dtype == BF16 and c.stats.shape == (37, 2, 2) and c.stats.dtype == F32
    # the folded operands state LayerNorm + linear up to the folded weight's own rounding
    want = F.linear(F.layer_norm(c.y.double(), (128,), c.gamma.double(), c.beta.double(), R.LN_EPS), c.w_plain.double(), c.b.double())
    assert float((c.want() - want).abs().max()) < 0.05 and float((c.want() - want).abs().mean()) < 0.005


def int_cases():
    """Every integer case once: its operands do not depend on the 16-bit type."""
    for name, (cases, _) in R.CASE_SETS.items():
        for c in cases(BF16, "int"):
            yield name, c
    for name, (cases, _) in R.CASE_SETS32.items():
        for c in cases("int"):
            yield name + "32", c


def test_integer_cases_keep_their_premise():
    """Entries are integers exactly representable in every type (scale: a power of two) and 9 K + |bias| + |res|, through the
    affine, stays below 2^24: every partial result is exact in fp32."""
    n_cases = 0
    for name, c in int_cases():
        assert c.k <= 2048 and c.flavour == "int"
        if c.m * c.n > MAX_SENSITIVITY_OUTPUTS:               # the few big ones draw from the same code
            continue
        n_cases += 1
        peak = 9.0 * c.k
        for x, lim in ((c.a_buf, 3), (c.w_buf, 3), (c.bias, 8), (c.shift, 8), (c.res_buf, 8)):
            if x is None:
                continue
            assert float(x.double().abs().max()) <= lim and torch.equal(x.double(), x.double().round()), (name, c.what())
            for dt in (BF16, F16):
                assert torch.equal(x.double(), x.to(dt).double())
        if c.scale is not None:
            assert set(c.scale.tolist()) <= {0.5, 1.0, 2.0}
        peak = (peak + 8) * 2 + 8 + 8
        assert peak < 2 ** 24 and float(c.want().abs().max()) <= peak
        assert torch.equal(c.want() * 2, (c.want() * 2).round())
        assert torch.equal(c.want_out().double(), c.want()) or c.out_dt != F32     # fp32 holds the result itself
    assert n_cases > 400


def test_a_dropped_slab_is_visible():
    """For every integer case of at most 2^22 outputs: zeroing any one K slab (the tail included) changes at least one
    element of every 64 x 64 output tile, in the output's own type."""
    n_cases = n_slabs = 0
    for name, c in int_cases():
        if c.m * c.n > MAX_SENSITIVITY_OUTPUTS:
            continue
        n_cases += 1
        want = c.want_out()
        tm, tn = R.cdiv(c.m, 64), R.cdiv(c.n, 64)
        for k0, k1 in c.slabs():
            n_slabs += 1
            changed = torch.zeros(tm * 64, tn * 64, dtype=torch.bool)
            changed[:c.m, :c.n] = c.want(drop=(k0, k1)).to(c.out_dt) != want
            per_tile = changed.view(tm, 64, tn, 64).any(3).any(1)
            assert bool(per_tile.all()), (name, c.what(), (k0, k1), int((~per_tile).sum()))
    print(f"[sensitivity] {n_cases} integer cases, {n_slabs} slabs")
    assert n_cases > 400
