"""dh_linear and dh_linear_ln on every tile route, ring depth, shape edge, epilogue form, stride and type, against the plain fp64
statement of the operation (linear_ref.linear_ref / linear_ln_ref) on the same operands -- rounded to the 16-bit type first
for bf16 / fp16.  The cases, their references and the restated launcher rules are in linear_ref.py; tests/test_linear_ref_cpu.py
checks the references against F.linear / F.layer_norm, every case table against the route set asserted here, and that in every
integer case a dropped K slab changes every 64 x 64 output tile.

  t128   gemm_bf16_kernel<128, 128> (2-slab ring, 8 waves) / fp32: linear_f32_kernel<128, 128>: >= 192 big tiles
  n64    gemm_bf16_kernel<128, 64>: N <= 64 and M >= 131072
  r4 r8  the 64 x 64 kernels with an LDS ring of 4 / 8 / 3 / 2 slabs, chosen by workgroup count (320 | 512 | 768 | 1280) and
  r3 r2  K <= 128
  pers   vocab_logits_kernel<2, 128, 128>: fp32 output, >= 1024 big tiles, bias-only epilogue, 16-byte rows
  t64    fp32: linear_f32_kernel<64, 64>
  ln_a_* dh_linear_ln, LayerNorm folded on the A side (EXT 1); ln_r_*: residual LayerNorm / output statistics (EXT 3)

Every case runs in two operand flavours.  "int": small integer operands whose every partial sum is exact in fp32 in any order;
the output must EQUAL the exact result (rounded once for 16 bits), which no dropped or doubled K chunk, stale slab, wrong tile
mapping or missed epilogue term survives.  "real": randn operands against fp64 -- 16-bit outputs in ulps at max(|want|, 2^-6)
(attn_ref.ulps), fp32 outputs by absolute error, never above F32_ATOL = 2e-5.  Both tables hold 1.25 x the worst error measured
on an MI355X over the route's cases (the 1.25 covers another, equally valid accumulation order).  Every call writes into a
sentinel-filled buffer with spare rows and a row stride wider than N; whatever [M, N] does not address must keep the sentinel.
Every test prints its worst error per (route, type)."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import linear_ref as R  # noqa: E402
from linear_ref import BF16, DT16, DT16_IDS, F16, F32  # noqa: E402

# 1.25 x the worst error measured on an MI355X over every real-flavour case of the route; check() prints it.
# 16-bit outputs, ulps at max(|want|, 2^-6); keyed by the operands' (= the output's) type:
ULP_GATE = {
    "t128": {BF16: 1.25 * 0.5011, F16: 1.25 * 0.5305},
    "n64": {BF16: 1.25 * 0.5004, F16: 1.25 * 0.5068},
    "r4": {BF16: 1.25 * 0.5014, F16: 1.25 * 0.5233},
    "r8": {BF16: 1.25 * 0.5003, F16: 1.25 * 0.5079},
    "r3": {BF16: 1.25 * 0.5012, F16: 1.25 * 0.5222},
    "r2": {BF16: 1.25 * 0.5006, F16: 1.25 * 0.5176},
    "ln_a_r4": {BF16: 1.25 * 0.5027, F16: 1.25 * 0.5544},
    "ln_a_r8": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5081},
    "ln_a_r3": {BF16: 1.25 * 0.5013, F16: 1.25 * 0.5228},
    "ln_a_r2": {BF16: 1.25 * 0.5031, F16: 1.25 * 0.5308},
    "ln_r_r4": {BF16: 1.25 * 0.5013, F16: 1.25 * 0.5387},
    "ln_r_r8": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5153},
    "ln_r_r3": {BF16: 1.25 * 0.5027, F16: 1.25 * 0.5296},
    "ln_r_r2": {BF16: 1.25 * 0.5028, F16: 1.25 * 0.5475},
}
# fp32 outputs, absolute; keyed by the operands' type.  ln_mean / ln_m2: the output statistics of dh_linear_ln against fp64
# statistics of the kernel's own rounded output -- the tile mean, and the tile's sum of squared deviations relative to max(it, 1)
ABS_GATE = {
    "t128": {F32: 1.25 * 1.884e-06, BF16: 1.25 * 1.159e-06, F16: 1.25 * 1.373e-06},
    "t64": {F32: 1.25 * 1.961e-06},
    "pers": {BF16: 1.25 * 9.760e-07, F16: 1.25 * 1.150e-06},
    "r4": {BF16: 1.25 * 6.697e-07, F16: 1.25 * 8.413e-07},
    "r8": {BF16: 1.25 * 5.662e-07, F16: 1.25 * 7.165e-07},
    "ln_mean": {BF16: 1.25 * 7.823e-08, F16: 1.25 * 8.941e-08},
    "ln_m2": {BF16: 1.25 * 2.343e-07, F16: 1.25 * 2.410e-07},
}
# Conditions on the tables, not measurements.  A plain 16-bit entry: an fp32 result rounded once sits just over 0.5 ulp, a
# second rounding near 1.0; nothing in between may be entered.  dh_linear_ln: test_linear_with_deferred_layernorm
# (test_bf16_gpu.py) asserts |err| <= atol + rtol |want| with rtol >= 1e-2; one ulp is at most 2^-7 |want| (bf16), so that
# test allows more than 1.28 ulp everywhere -- no entry here may.  (Its statistics: atol 2e-5 / rtol 1e-4; AbsGate.check
# holds both entries under F32_ATOL = 2e-5.)
assert all(v <= 0.75 for name, row in ULP_GATE.items() if not name.startswith("ln_") for v in row.values())
assert all(v <= 1.28 for name, row in ULP_GATE.items() if name.startswith("ln_") for v in row.values())


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
    print(f"[test_linear_routes_gpu] module wall time {time.time() - t0:.1f} s")


def full(shape, dt):
    return torch.full(shape, R.SENTINEL, dtype=dt, device="cuda")


def kept(t):
    return bool((t == R.SENTINEL).all())


def dev(x):
    return None if x is None else x.cuda()


def run_case(hip, c):
    """One hip.linear call on case ``c``: the [m, n] output, after the sentinel checks."""
    a, w, res = c.a_buf.cuda()[:, :c.k], c.w_buf.cuda()[:, :c.k], dev(c.res_buf)
    if res is not None:
        res = res[:, c.res_off:c.res_off + c.n]
        assert res.stride(0) == c.ldres and (res.data_ptr() % 16 == 0) == (c.res_off % 8 == 0 or c.dt == F32)
    assert a.stride(0) == c.lda and w.stride(0) == c.ldw
    kw = dict(bias=dev(c.bias), scale=dev(c.scale), shift=dev(c.shift), relu=c.relu, residual=res)
    if c.wrapper_out:
        out = hip.linear(a, w, out_dtype=c.out_dt, **kw)
        assert out.shape == (c.m, c.n) and out.stride(0) == c.ldc and out.dtype == c.out_dt, (c.what(), out.stride())
        return out
    buf = full((c.m + R.EXTRA_ROWS, c.ldc), c.out_dt)
    out = buf[:c.m, c.c_off:c.c_off + c.n]
    assert (out.data_ptr() % 16 == 0) == c.c_aligned
    hip.linear(a, w, out=out, **kw)
    assert kept(buf[c.m:]) and kept(buf[:c.m, :c.c_off]) and kept(buf[:c.m, c.c_off + c.n:]), c.what()
    return out


def run_set(hip, dt, name, key=lambda c: c.route):
    """Both flavours of one case set: torch.equal for "int", the route's gate for "real".  Returns {key(c)} over the cases."""
    cases, routes = (R.CASE_SETS32 if dt == F32 else R.CASE_SETS)[name]
    gates, reached, seen, unequal = R.RouteGates(dt, ULP_GATE, ABS_GATE), set(), set(), []
    for fl in R.FLAVOURS:
        for c in (cases(fl) if dt == F32 else cases(dt, fl)):
            reached.add(c.route)
            seen.add(key(c))
            got = run_case(hip, c)
            if fl == "int":
                want = c.want_out()
                if not torch.equal(got.cpu(), want):
                    unequal.append((c.route, c.what(), int((got.cpu() != want).sum())))
            else:
                gates.add(c.route, got, c.want(), c.what(), c.out_f32)
    assert not unequal, unequal
    assert reached == routes, sorted(reached)
    gates.check()
    return seen


# ---- 1 .. 5: the routes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_ring_switches(hip, dt):
    """Workgroup counts on both sides of each switch of the ring depth (320 | 321, 512 | 513, 768 | 769, 1280 | 1281), the last
    row tile partial, K = 192 / 256; and r4 for its other reason, K <= 128, at a count that would give r8."""
    seen = run_set(hip, dt, "ring_switch", lambda c: (c.blocks, c.route))
    assert seen == {want for _, want in R.RING_SWITCH}, sorted(seen)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_slabs_against_ring_depth(hip, dt):
    """Each ring depth NS with NS - 2 .. NS + 1 and 2 NS + 1 slabs (K <= 128: always r4, which also runs 1 and 2; r8 also 3),
    each count once with K % 64 == 0 (the pointer-stepping loader) and once with a K tail of 8 or 56."""
    seen = run_set(hip, dt, "slabs", lambda c: (c.route, R.cdiv(c.k, 64), c.k % 64 == 0))
    assert seen == {(r, s, st) for r in R.NS for s in R.slab_counts(r) for st in (True, False)}, sorted(seen)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_big_tiles(hip, dt):
    """The 128 x 128 kernel at exactly 192 tiles (24 x 8: workgroups walk N first; 8 x 24: M first), K = 64 / 128 (its
    stepping loader, one and two slabs) / 520 (the K-tail loader); 191 tiles, M = 95 and N = 95 fall to the 64 x 64 kernels."""
    seen = run_set(hip, dt, "big_tiles", lambda c: (c.route, R.n_fast(c.m, c.n, c.k)) if c.route == "t128" else c.route)
    assert seen == {("t128", 0), ("t128", 1), "r3", "r4"}, seen


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_narrow(hip, dt):
    """N = 40 / 64, K = 64: 131072 rows run the 128 x 64 kernel, 131071 the 64 x 64 one."""
    run_set(hip, dt, "narrow")


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_persistent_fp32_out(hip, dt):
    """M 4096, K 128, N 4097 (a last partial group of four columns) in fp32: hip.linear pads the rows to 4160 and the
    persistent kernel runs, with and without a bias; ldc % 4 != 0, relu, a residual or 1023 tiles keep the call on t128."""
    seen = run_set(hip, dt, "persistent", lambda c: (c.route, c.form, c.ldc, c.wrapper_out))
    assert ("pers", "bias", 4160, True) in seen and ("pers", "none", 4160, False) in seen and ("t128", "bias", 4097, False) in seen


# ---- 6 .. 8: edges, epilogue forms, strides, alignment -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_shape_edges(hip, dt):
    """M 1 .. 130 x N 8 .. 4567 (68: a partial last chunk inside a 16-byte call; 130: scalar bias loads) x K 8 .. 136, lda
    and ldw wider than K."""
    seen = run_set(hip, dt, "edges", lambda c: (c.m, c.n, c.k))
    assert len(seen) == 150


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_epilogue_forms_and_strides(hip, dt):
    """bias / scale and shift / all three (the bias fold) / residual / relu / everything, 16-bit and fp32 output, with ldc and
    ldres multiples of the 16-byte chunk (the row-contiguous epilogue) and not (the element-wise one)."""
    seen = run_set(hip, dt, "forms", lambda c: (c.form, c.out_f32))
    assert seen == {(f, o) for f in R.FORM_NAMES for o in (False, True)}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_base_alignment(hip, dt):
    """out and / or residual are column slices starting 4 elements (8 bytes) into 16-bit buffers whose rows are multiples of 8
    elements: the 16-byte epilogue must not run on them (it did before ``fast`` looked at the base pointers)."""
    seen = run_set(hip, dt, "align", lambda c: (c.c_off, c.res_off))
    assert seen == set(R.ALIGN_OFFS)


# ---- 9: fp32 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASE_SETS32))
def test_f32(hip, name):
    """linear_f32_kernel<128, 128> at 192 tiles (K 4 .. 68) and <64, 64> below, the shape edges with K 4 .. 68, every form."""
    run_set(hip, F32, name)


# ---- 10: deferred LayerNorm --------------------------------------------------------------------------------------------------
def run_ln(hip, c, res, relu, **kw):
    buf = full((c.m + R.EXTRA_ROWS, c.ldc), c.dt)
    out = hip.linear_ln(dev(c.a), dev(c.w), dev(c.bias), out=buf[:c.m, :c.n], residual=dev(c.res) if res else None, relu=relu, **kw)
    out, st = out if isinstance(out, tuple) else (out, None)
    assert kept(buf[c.m:]) and kept(buf[:c.m, c.n:]), c.what()
    return out, st


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_ln_a_side(hip, dt):
    """EXT 1: a_tiles 2 .. 8, workgroup counts in each ring range (r4 for each of its three reasons), a partial last row tile
    (its statistics loads are clamped to M - 1); plain, relu, and a plain residual."""
    gates, reached = R.RouteGates(dt, ULP_GATE, ABS_GATE, "ln_a_"), set()
    for c in R.ln_a_cases(dt):
        reached.add((c.blocks, c.route))
        a_ln = (dev(c.stats), R.LN_EPS, dev(c.colsum))
        for res, relu in R.LN_A_FORMS:
            out, _ = run_ln(hip, c, res, relu, a_ln=a_ln)
            gates.add(c.route, out, c.want(res, relu), dict(c.what(), res=res, relu=relu))
    assert reached == {want for _, want in R.LN_A_SHAPES}, sorted(reached)
    gates.check()


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_ln_residual_side_and_statistics(hip, dt):
    """EXT 3: residual rows pre-LayerNorm (r_ln) with and without output statistics, plain or no residual with statistics, each
    with and without relu; N 128 / 512, up to 10297 rows.  The statistics are those of the rounded output, per 64-column tile."""
    gates, reached = R.RouteGates(dt, ULP_GATE, ABS_GATE, "ln_r_"), set()
    mean, m2 = R.AbsGate("ln_mean", dt, ABS_GATE, "tile mean"), R.AbsGate("ln_m2", dt, ABS_GATE, "tile M2, relative")
    for c in R.ln_r_cases(dt):
        reached.add((c.blocks, c.route))
        r_ln = (dev(c.stats), R.LN_EPS, dev(c.gamma), dev(c.beta))
        for res, stats, relu in R.LN_R_FORMS:
            what = dict(c.what(), res=res, stats=stats, relu=relu)
            out, st = run_ln(hip, c, res, relu, r_ln=r_ln if res == "ln" else None, want_stats=stats)
            gates.add(c.route, out, c.want(res, relu), what)
            if stats:
                want = R.tile_stats(out.cpu())
                assert st.shape == want.shape, what
                mean.add(st[..., 0], want[..., 0], what)
                scale = want[..., 1].clamp(min=1.0)
                m2.add(st[..., 1].cpu().double() / scale, want[..., 1] / scale, what)
    assert reached == {want for _, want in R.LN_R_SHAPES}, sorted(reached)
    failed = []
    for g in (gates, mean, m2):
        try:
            g.check()
        except AssertionError as e:
            failed.append(e)
    assert not failed, failed
