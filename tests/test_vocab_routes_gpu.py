"""dh_vocab_logits, dh_vocab_logits_wreg and dh_vocab_logprob on every kernel route, option, K, shape edge, stride and type,
against the plain fp64 statement of the operation (vocab_ref.logits_ref / group_max_ref / logprob_ref) on the same operands,
rounded to bf16 / fp16 first.  The cases, their references and the restated launcher rules are in vocab_ref.py;
tests/test_vocab_ref_cpu.py checks the references against F.linear / log_softmax, every case table against the route set asserted
here, and that in every integer case a dropped K slab changes every 16-row x 64-column block.

  a256    vocab_areg256_kernel (A in registers, 256-row tiles), one launch or several by a plan: K = 512, M % 256 == 0
  a128    vocab_areg_kernel (128-row tiles): K = 512, <= 32 row tiles and enough panels for them
  pers    vocab_logits_kernel<2, 128, 128>: K >= 128, K % 64 == 0
  g256    vocab256_kernel: group maxima only, M >= 512
  tile    gemm_bf16_kernel<128, 128> with the group-maxima epilogue: K < 128, a K tail, logits rows or base off 16 bytes
  wreg    vocab_wreg_kernel (dh_vocab_logits_wreg)
  lse128  vocab_logits_kernel / vocab256_kernel in LSE mode + lse_combine_kernel (dh_vocab_logprob)
  lse256

Every case runs in two operand flavours.  "int": small integer operands whose every partial sum is exact in fp32 in any order;
logits and group maxima must EQUAL the exact result.  "real": randn operands; the logits go through the route's AbsGate against
fp64 and the group maxima must equal the maxima of the kernel's own stored logits over the real columns; without logits the group
maxima go through the same gate against group_max_ref (a maximum is 1-Lipschitz).  ABS_GATE holds 1.25 x the worst error measured
on an MI355X over the route's cases (the 1.25 covers another, equally valid accumulation order).

Every call writes into sentinel-filled buffers with spare rows, a logits row stride wider than the route needs and spare
group-maxima columns; whatever the call's contract does not address must keep the sentinel.  THE ROUTE WITNESS: a256 and wreg are
the only routes that write logits columns past V -- copies of logit[V - 1] up to whole 128-column panels / 256-column chunks --
and on every other route those columns keep the sentinel; every case asserts this from the restated route(), the one output that
tells which kernel ran.  Every test prints its worst error per (route, type), the module its wall time."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import vocab_ref as R  # noqa: E402
from vocab_ref import BF16, DT16, DT16_IDS, F16, F32  # noqa: E402

# 1.25 x the worst absolute error measured on an MI355X over every real-flavour case of the route; check() prints it.
ABS_GATE = {
    "a256": {BF16: 1.25 * 2.363e-06, F16: 1.25 * 2.259e-06},
    "a128": {BF16: 1.25 * 2.363e-06, F16: 1.25 * 2.167e-06},
    "pers": {BF16: 1.25 * 2.393e-06, F16: 1.25 * 2.205e-06},
    "g256": {BF16: 1.25 * 1.704e-06, F16: 1.25 * 1.597e-06},
    "tile": {BF16: 1.25 * 2.021e-06, F16: 1.25 * 1.675e-06},
    "wreg": {BF16: 1.25 * 1.994e-06, F16: 1.25 * 1.835e-06},
}
# dh_vocab_logprob against logprob_ref; *_spike: the rows with one logit 60 above the rest (a log-prob of -60: one fp32 ulp is 3.8e-6,
# and the 60 is in the accumulator from the first of the K products on)
LOGP_GATE = {
    "lse128": {BF16: 1.25 * 1.454e-06, F16: 1.25 * 1.773e-06},
    "lse256": {BF16: 1.25 * 1.187e-06, F16: 1.25 * 1.448e-06},
    "lse128_spike": {BF16: 1.25 * 2.925e-05, F16: 1.25 * 3.635e-05},
    "lse256_spike": {BF16: 1.25 * 2.933e-05, F16: 1.25 * 2.991e-05},
}
# Conditions on the tables, not measurements: fp32 logits stay under the project's bar for fp32 outputs, log-probs under the bar
# test_vocab_logprob_matches_log_softmax (test_bf16_gpu.py) sets.
assert all(v <= R.F32_ATOL for row in ABS_GATE.values() for v in row.values())
assert all(v <= R.LOGP_ATOL for row in LOGP_GATE.values() for v in row.values())


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
    print(f"[test_vocab_routes_gpu] module wall time {time.time() - t0:.1f} s")


def full(shape, dt=F32):
    return torch.full(shape, R.SENTINEL, dtype=dt, device="cuda")


def kept(t):
    return bool((t == R.SENTINEL).all())


def dev(x):
    return None if x is None else x.cuda()


def launch(hip, c, a, w, bias, logits, gm):
    """The case's entry point under its option value."""
    old = hip.set_option("vocab_areg", c.areg)
    try:
        if c.entry == "wreg":
            wp, bp = hip.pack_vocab_weights(w, bias)
            hip.vocab_logits_wreg(a, wp, bp, c.v, logits, gm)
        else:
            hip.vocab_logits(a, w, bias, logits, gm)
        torch.cuda.synchronize()
    finally:
        hip.set_option("vocab_areg", old)


def buffers(c, rows):
    """Sentinel-filled (logits buffer or None, group-maxima buffer) for ``rows`` rows of case ``c``."""
    return (full((rows + R.EXTRA_ROWS, c.ldl)) if c.logits else None), full((rows + R.EXTRA_ROWS, c.groups + R.GM_SPARE))


def check_outputs(c, route, lbuf, gbuf, want, gates, unequal):
    """``lbuf`` / ``gbuf``: the CPU copies of the whole buffers the call(s) wrote rows [0, rows) of; ``want``: fp64 [rows, v]."""
    rows, v, what = want.shape[0], c.v, dict(c.what(), route=route)
    assert kept(gbuf[rows:]) and kept(gbuf[:rows, c.groups:]), what
    gm = gbuf[:rows, :c.real_groups]
    assert bool((gbuf[:rows, c.real_groups:c.groups] == R.NEG_INF).all()), what          # groups that start past V
    got = None
    if c.logits:
        lo, pad_to = c.l_off, c.l_off + R.roundup(v, {"a256": 128, "wreg": 256}.get(route, 1))
        got = lbuf[:rows, lo:lo + v]
        assert kept(lbuf[rows:]) and kept(lbuf[:rows, :lo]) and kept(lbuf[:rows, pad_to:]), what
        assert bool((lbuf[:rows, lo + v:pad_to] == got[:, v - 1:v]).all()), what         # the route witness
    if c.flavour == "int":
        exact = want.float()
        if got is not None and not torch.equal(got, exact):
            unequal.append((what, "logits", int((got != exact).sum())))
        if not torch.equal(gm, R.group_max_ref(exact)):
            unequal.append((what, "group maxima", int((gm != R.group_max_ref(exact)).sum())))
    elif got is not None:
        gates.add(route, got, want, what, out_f32=True)
        if not torch.equal(gm, R.group_max_ref(got)):
            unequal.append((what, "group maxima of the stored logits", int((gm != R.group_max_ref(got)).sum())))
    else:
        gates.add(route, gm, R.group_max_ref(want), what, out_f32=True)


def run_case(hip, c, gates, unequal):
    a, w = c.a_buf.cuda()[:, :c.k], c.w_buf.cuda()[:, :c.k]
    assert a.stride(0) == c.lda and w.stride(0) == c.ldw
    lbuf, gbuf = buffers(c, c.m)
    logits = None
    if c.logits:
        logits = lbuf[:c.m] if c.entry == "wreg" else lbuf[:c.m, c.l_off:c.l_off + c.v]
        assert logits.stride(0) == c.ldl and (logits.data_ptr() % 16 == 0) == c.aligned
    launch(hip, c, a, w, dev(c.bias), logits, gbuf[:c.m, :c.groups])
    check_outputs(c, c.route, lbuf.cpu() if c.logits else None, gbuf.cpu(), c.want(), gates, unequal)


def run_cases(hip, dt, cases, routes):
    """Both flavours of ``cases(dt, fl)``; the routes reached must be ``routes``.  Returns the cases run."""
    gates, unequal, done = R.RouteGates(dt, {}, ABS_GATE), [], []
    for fl in R.FLAVOURS:
        for c in cases(dt, fl):
            run_case(hip, c, gates, unequal)
            done.append(c)
    assert not unequal, unequal
    assert {c.route for c in done} == routes, sorted({c.route for c in done})
    gates.check()
    return done


def run_set(hip, dt, name):
    return run_cases(hip, dt, *R.CASE_SETS[name])


# ---- the routes of dh_vocab_logits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_a256_single_launch(hip, dt):
    """vocab_areg256_kernel in one launch of 8 / 16 / 5 / 2 row tiles: V ends inside a group with the panel's second group past V
    (4000), one real column in the last of the fewest panels 16 row tiles take (1921), V a multiple of 128 (8192), 128 panels
    for the two-tile launch (16300)."""
    done = run_set(hip, dt, "a256_single")
    assert [R.areg256_plan(c.m, c.v, c.ldl) for c in done] == [p for _, p in R.A256_SINGLE] * 2


@pytest.mark.parametrize("shape,plan", R.A256_MULTI, ids=[f"{m}x{v}" for (m, v), _ in R.A256_MULTI])
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_a256_multi_launch(hip, dt, shape, plan):
    """Row counts whose 256-row tiles do not fit one launch: 26 tiles as [16, 10], 11 as [8, 3].  Each launch offsets A, the
    logits and the group maxima by its first row; rows on both sides of each boundary are compared like all others."""
    m, v = shape
    done = run_cases(hip, dt, lambda dt, fl: [R.VocabCase(dt, fl, m, v)], {"a256"})
    assert all(R.areg256_plan(c.m, c.v, c.ldl) == plan and len(plan) > 1 for c in done)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_abandoned_plan(hip, dt):
    """Shapes whose rows are multiples of 256 and that still do not run the 256-row kernel: too few panels for 2 / 8 row tiles,
    12 row tiles (no launch size fits), and a row stride of whole groups instead of whole panels."""
    done = run_set(hip, dt, "abandoned")
    assert [c.route for c in done[:4]] == [r for _, r in R.ABANDONED] + ["a128"]
    assert all(R.areg256_plan(c.m, c.v, c.ldl) is None for c in done)
    assert R.areg256_plan(*R.LDL_64[:2]) is not None          # ... which only the stride keeps off the 256-row kernel


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_a128(hip, dt):
    """vocab_areg_kernel: a partial last row tile on one and on three row tiles at 286 panels, 16 full row tiles at 31 panels (the
    last one partial), with and without bias."""
    run_set(hip, dt, "a128")


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_option_vocab_areg_128(hip, dt):
    """vocab_areg = 128 ("never the 256-row form") at every single-launch a256 shape gives the 128-row kernel, and at 52 row
    tiles of 128 the tile kernel."""
    done = run_set(hip, dt, "areg128")
    assert all(R.route(c.m, c.v, c.k, True, c.ldl) == "a256" for c in done)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_pers(hip, dt):
    """vocab_logits_kernel: vocab_areg = 0 at K = 512; K = 128 (two slabs, the ring's minimum) / 192 / 256 / 1024 at default
    options; at most one tile per workgroup (16 tiles) and several (858 tiles on 512 workgroups: interior -> edge -> interior,
    the vmcnt bookkeeping with prev_full; 640 interior tiles); group maxima only below 512 rows."""
    done = run_set(hip, dt, "pers")
    tiles = {R.cdiv(c.m, 128) * R.cdiv(c.v, 128) > 512 for c in done}
    assert tiles == {False, True} and {c.k for c in done} == {512} | set(R.PERS_K) and {c.logits for c in done} == {False, True}
    assert {c.areg for c in done if c.k == 512 and c.logits} == {0}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_g256(hip, dt):
    """vocab256_kernel, group maxima only, at 512 / 600 / 1280 rows: V ends inside a 256-column tile's first half (1100: the
    tile's last two groups do not exist), its second half (4000) and on a multiple of 256 (2048); K = 128 / 192 / 512."""
    done = run_set(hip, dt, "g256")
    assert {(c.v - 1) % 256 // 128 for c in done} == {0, 1} and {c.v % 256 == 0 for c in done} == {False, True}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_tile_fallback(hip, dt):
    """gemm_bf16_kernel<128, 128> with the group-maxima epilogue: K = 64 / 72 / 136 / 520; K = 512 with logits rows that are no
    multiple of 16 bytes, and with a logits view that starts 8 bytes into 16-byte rows."""
    done = run_set(hip, dt, "tile")
    assert {c.k for c in done} == {512} | set(R.TILE_K)
    assert {(c.ldl % 4 == 0, c.aligned) for c in done if c.k == 512} == {(False, True), (True, False)}


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_operand_strides(hip, dt):
    """lda = K + 8 and ldw = K + 16 with every column drawn, on every route of dh_vocab_logits."""
    done = run_set(hip, dt, "strides")
    assert all(c.lda == c.k + 8 and c.ldw == c.k + 16 for c in done)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_row_sliced_calls(hip, dt):
    """One buffer of 1100 rows computed as [:1024] then [1024:], the way classifier_groups (csrc/runtime.hip) splits a row count
    that is no multiple of 256: a256 on the head, vocab_logits_kernel on the 76 rows behind it; equal to the references row for row."""
    gates, unequal, reached = R.RouteGates(dt, {}, ABS_GATE), [], set()
    for fl in R.FLAVOURS:
        c, parts = R.sliced_parts(dt, fl)
        a, w = c.a_buf.cuda(), c.w_buf.cuda()
        lbuf, gbuf = buffers(c, c.m)
        for row0, rows in parts:
            launch(hip, c, a[row0:row0 + rows], w, dev(c.bias), lbuf[row0:row0 + rows, :c.v], gbuf[row0:row0 + rows, :c.groups])
        L, G, want = lbuf.cpu(), gbuf.cpu(), c.want()
        for row0, rows in parts:                              # each part against its own route's witness and gate
            route = R.route(rows, c.v, c.k, True, c.ldl)
            reached.add(route)
            check_outputs(c, route, torch.cat([L[row0:row0 + rows], L[c.m:]]), torch.cat([G[row0:row0 + rows], G[c.m:]]),
                          want[row0:row0 + rows], gates, unequal)
    assert not unequal, unequal
    assert reached == R.SLICED_ROUTES, reached
    gates.check()


# ---- dh_vocab_logits_wreg ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_wreg(hip, dt):
    """vocab_wreg_kernel against fp64 and the exact integer result: 5 / 80 / 81 / 380 / 640 / 1280 rows (a masked last block,
    idle padding blocks, 16 full blocks); V ends inside a group, inside a chunk and on a chunk boundary; with and without bias,
    with and without logits, lda > K.  Every group of the padded vocabulary is defined (-inf past V), every padding column holds
    logit[V - 1]."""
    done = run_set(hip, dt, "wreg")
    assert {c.m for c in done} == {5, 80, 81, 380, 640, 1280} and {c.lda > c.k for c in done} == {False, True}
    assert {(c.has_bias, c.logits) for c in done} == {(b, lg) for b in (False, True) for lg in (False, True)}
    assert all(hip.vocab_logits_wreg_supported(c.m, c.v, c.k, c.ldl, c.groups + R.GM_SPARE) for c in done)


def test_wreg_supported_matches_its_restatement(hip):
    """dh_vocab_logits_wreg_supported over a grid of (M, V, K, ldl, gm_ld) around each threshold."""
    grid = list(R.wreg_grid())
    wrong = [g for g in grid if hip.vocab_logits_wreg_supported(*g) != R.wreg_supported(*g)]
    assert not wrong, wrong[:10]
    assert {R.wreg_supported(*g) for g in grid} == {False, True}


# ---- dh_vocab_logprob ----------------------------------------------------------------------------------------------------------
def run_logprob(hip, dt, cases, suffix=""):
    gates, reached = {}, set()
    for c in cases(dt):
        reached.add(c.route)
        got = hip.vocab_logprob(dev(c.a), dev(c.w), dev(c.bias), dev(c.targets)).cpu()
        want = c.want()
        assert got.shape == (c.m,) and got.dtype == F32
        assert bool((got[2:4] == 0).all()) and bool((want[2:4] == 0).all()), c.what()    # targets -1 and V
        assert bool((want[:2] < 0).all()) and float(want[4]) < 0
        name = c.route + suffix
        gates.setdefault(name, R.LogpGate(name, dt, LOGP_GATE, "log-prob")).add(got, want, c.what())
    assert reached == {"lse128", "lse256"}, reached
    failed = []
    for g in gates.values():
        try:
            g.check()
        except AssertionError as e:
            failed.append(e)
    assert not failed, failed


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_logprob(hip, dt):
    """dh_vocab_logprob against log_softmax in fp64: 37 / 300 rows (vocab_logits_kernel in LSE mode), 512 / 600 (vocab256_kernel);
    K = 128 / 512 / 1024; V = 1000 (ends in a 256-column tile's second half), 4100 (four columns into its first half) and 36541;
    targets 0, V - 1 and V - 2 (the last partial group), and -1 and V, which give 0."""
    run_logprob(hip, dt, R.logprob_cases)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_logprob_wide_range_rows(hip, dt):
    """Every row holds one logit about 60 above the rest: each other group's sum enters through exp(gmax - M) alone."""
    cases = list(R.logprob_spike_cases(dt))
    for c in cases:
        lg = c.logits()
        top2 = lg.topk(2, -1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > R.SPIKE - 15 and bool((lg.argmax(-1) == c.v // 2).all()), c.what()
        assert float(c.want()[5]) > -1e-6 and float(c.want()[6:].max()) < -(R.SPIKE - 15)
    run_logprob(hip, dt, lambda dt: cases, "_spike")


# ---- refused calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_refused_calls(hip, dt):
    """Arguments DH_REQUIRE rejects before any launch (csrc/gemm_bf16.hip dh_vocab_logits, csrc/vocab_wreg.hip): each raises and
    leaves every buffer at the sentinel."""
    m, v = 130, 1000
    ng = R.n_groups(v)

    def operands(k, pad=0, off=0):
        g = torch.Generator().manual_seed(k + pad)
        a = torch.randn(m, k + pad, generator=g).to(dt).cuda()[:, off:off + k]
        return a, (torch.randn(v, k, generator=g) / k ** 0.5).to(dt).cuda(), torch.randn(v, generator=g).cuda()

    def refused(call, *bufs):
        with pytest.raises(RuntimeError):
            call()
        torch.cuda.synchronize()
        assert all(kept(b) for b in bufs)

    lbuf, gbuf = full((m + R.EXTRA_ROWS, 1032)), full((m + R.EXTRA_ROWS, ng + R.GM_SPARE))
    logits, gm = lbuf[:m, :v], gbuf[:m, :ng]
    # "DH_REQUIRE(logits || (K >= 128 && (K % 64) == 0))": group maxima only at K = 64
    a, w, b = operands(64)
    refused(lambda: hip.vocab_logits(a, w, b, None, gm), gbuf)
    a, w, b = operands(512)
    # "gm_ld >= 2 * dh_cdiv(V, 128)": one short
    short = full((m + R.EXTRA_ROWS, ng - 1))
    refused(lambda: hip.vocab_logits(a, w, b, logits, short[:m]), lbuf, short)
    # "(!logits || ldl >= V)": rows of V - 4 elements
    narrow = full((m + R.EXTRA_ROWS, v - 4))
    refused(lambda: hip.vocab_logits(a, w, b, narrow[:m], gm), narrow, gbuf)
    # "(lda % 8) == 0": lda = K + 4
    a4, _, _ = operands(512, pad=4)
    assert a4.stride(0) % 8 == 4 and a4.data_ptr() % 16 == 0
    refused(lambda: hip.vocab_logits(a4, w, b, logits, gm), lbuf, gbuf)
    # "((uintptr_t)A % 16) == 0": the view starts 4 elements into rows of K + 8
    a8, _, _ = operands(512, pad=8, off=4)
    assert a8.stride(0) % 8 == 0 and a8.data_ptr() % 16 == 8
    refused(lambda: hip.vocab_logits(a8, w, b, logits, gm), lbuf, gbuf)
    # dh_vocab_logits_wreg: "dh_vocab_logits_wreg_supported(M, V, K, ...)" needs K == 512
    a, w, b = operands(256)
    wp, bp = hip.pack_vocab_weights(w, b)
    wl, wg = full((m + R.EXTRA_ROWS, 1032)), full((m + R.EXTRA_ROWS, 16 + R.GM_SPARE))
    assert not hip.vocab_logits_wreg_supported(m, v, 256, 1032, 16 + R.GM_SPARE) and hip.vocab_logits_wreg_supported(m, v, 512, 1032, 16 + R.GM_SPARE)
    refused(lambda: hip.vocab_logits_wreg(a, wp, bp, v, wl[:m], wg[:m, :16]), wl, wg)
