"""The decode attention (what ``generate()`` runs) on every kernel route, history length and type, against the plain fp64
statement of the reference's attention (transformers.py:106-120) on the same operands -- rounded to the 16-bit type first
for bf16 / fp16.  The cases and their vectorised reference are in attn_ref.py; tests/test_attn_ref_cpu.py checks, from the
reference alone, that in every self-attention case a dropped key t or t - 1 moves every even row by more than 8 x the gate.

``dh_attn_self_decode`` (L = t + 1 keys, head dim dh; launch_fast / launch_self in csrc/attention.hip):
  self_reg      attn_decode_reg_kernel<.., 64, 2 | 5 | 7>: dh 64, L <= 16 | 40 | 56 (the last in 16 bits only)
  self_fast     attn_decode_fast_kernel<.., 64 | 128 | 32>: dh 64 beyond that, dh 128, dh 32
  self_generic  attn_decode_kernel: any other head dim (16, 96)
``dh_attn_cross_decode`` (S keys):
  cross_lds     attn_cross_lds_kernel: dh 64, S <= 64
  cross_fast    attn_decode_fast_kernel<.., CROSS>: dh 64 with S > 64, dh 128, dh 32
  cross_generic attn_decode_kernel<.., CROSS>: any other head dim
``dh_attn_cross_pack`` + ``dh_attn_cross_decode_packed``:
  cross_packed  attn_cross_mfma_kernel, 16-bit only, both head-dim slot orders (``dperm``)

Gates.  fp32: ``atol = 2e-5, rtol = 0``.  16-bit: ulps at max(|want|, 2^-6) as in test_prefill_gpu.py, 1.25 x the worst error
measured on an MI355X against the fp64 reference, one entry per route.  Every route but the packed one computes in fp32 and
rounds once: half an ulp, plus the fp32 error of the fast softmax (v_rcp / v_exp, SmFast in attn_items.h) where |want| is small.
The packed kernel rounds its softmax weights to the operand type before the P V product (cross_core), so its error is that of
those roundings: the test prints the error of that same arithmetic restated in torch (``cross_packed_restated``: fp64 with the
weights rounded to the type, the result rounded once) next to the kernel's.  Measured: 26.5546 / 28.9929 ulp (bf16 / fp16, S = 7,
weights near 1/7 and |out| near 0) for the kernel AND for the restatement."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as A  # noqa: E402
from attn_ref import BF16, DT_IDS, DTYPES, F16, F32  # noqa: E402

# 1.25 x the worst 16-bit error measured on an MI355X over every case of the route (ulps at max(|want|, 2^-6)); check() prints it.
ULP_GATE = {
    "self_reg": {BF16: 1.25 * 0.5002, F16: 1.25 * 0.5055},
    "self_fast": {BF16: 1.25 * 0.5003, F16: 1.25 * 0.5032},
    "self_generic": {BF16: 1.25 * 0.5001, F16: 1.25 * 0.5052},
    "cross_lds": {BF16: 1.25 * 0.5003, F16: 1.25 * 0.5035},
    "cross_fast": {BF16: 1.25 * 0.5001, F16: 1.25 * 0.5016},
    "cross_generic": {BF16: 1.25 * 0.5000, F16: 1.25 * 0.5003},
    "cross_packed": {BF16: 1.25 * 26.5546, F16: 1.25 * 28.9929},
}
SENTINEL = 768.0                                              # exact in every type


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
    print(f"[test_attn_decode_gpu] module wall time {time.time() - t0:.1f} s")


class Gates:
    """One attn_ref.Gate per route a test reaches."""

    def __init__(self, dt):
        self.dt, self.gates = dt, {}

    def add(self, route, got, want, what):
        if route not in self.gates:
            self.gates[route] = A.Gate(route, self.dt, ULP_GATE)
        self.gates[route].add(got, want, what)

    def check(self, *routes):
        assert set(self.gates) == set(routes), (sorted(self.gates), routes)       # every route the test is there for was taken
        failed = []
        for g in self.gates.values():
            try:
                g.check()
            except AssertionError as e:
                failed.append(e)
        assert not failed, failed


def run_self(hip, c, tokens="live"):
    """One call on fresh copies of the caches: the result [rows, D], after checking that the sentinel rows behind ``out``
    survive and that the caches hold the new K / V at slot t of each row's own logical row and are otherwise unchanged."""
    if "dev" not in c.cache:
        c.cache["dev"] = (c.kc.cuda(), c.vc.cuda(), c.src.cuda())
    kc0, vc0, src = c.cache["dev"]
    kcd, vcd, qkv = kc0.clone(), vc0.clone(), c.qkv.cuda()
    out = torch.full((c.rows + A.EXTRA_ROWS, c.d), SENTINEL, dtype=c.dt, device="cuda")
    tok = c.tokens.cuda() if tokens == "live" else None
    hip.attn_self_decode(qkv, kcd, vcd, src, tok, out, c.n_img, c.rows_per_img, c.row_mult, c.rows_total, c.t, c.d, c.n_heads,
                         c.scale, c.pad_index)
    rl = torch.arange(c.rows, device="cuda") * c.row_mult
    kc0, vc0 = kc0.clone(), vc0.clone()
    kc0[c.t, rl], vc0[c.t, rl] = qkv[:, c.d:2 * c.d], qkv[:, 2 * c.d:]
    assert torch.equal(kcd, kc0) and torch.equal(vcd, vc0), c.what()                    # the whole cache, bit for bit
    assert bool((out[c.rows:] == SENTINEL).all()), c.what()
    return out[:c.rows]


# ---- 1. self-attention --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["pad0", "pad5", "nopad", "null"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_self_decode_every_history_length(hip, dt, pad):
    """dh 64, beam 4, 3 images, L = 1 .. 128: across 16 | 17, 40 | 41 (fp32: to the fast kernel) and 56 | 57 (16 bits).
    ``nopad`` is ``pad_index = -1`` with a live token array that never matches; ``null`` passes no token array at all and
    must give the same bits."""
    gates = Gates(dt)
    pad_index = {"pad0": 0, "pad5": 5, "nopad": -1, "null": -1}[pad]
    routes = set()
    for c in A.self_sweep_cases(dt, pad_index):
        got = run_self(hip, c)
        gates.add(c.route, got, c.want(), c.what())
        routes.add((c.route, c.t + 1))
        if pad == "null":
            assert torch.equal(run_self(hip, c, tokens=None), got), c.what()
    top = 40 if dt == F32 else 56
    assert ("self_reg", top) in routes and ("self_fast", top + 1) in routes and len(routes) == 128
    gates.check("self_reg", "self_fast")


@pytest.mark.parametrize("cases", ["row_blocks", "row_mult"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_self_decode_rows(hip, dt, cases):
    """``row_blocks``: 1 .. 64 rows per image (beyond 16 the image takes blockIdx.z row blocks, whose last one holds clamped
    clone waves that must store nothing) with ancestors anywhere in the image; ``row_mult``: compact rows, one per image,
    whose logical row is ``rc * row_mult``.  At the lengths where the route changes."""
    gates = Gates(dt)
    for c in A.SELF_CASE_SETS[cases](dt):
        gates.add(c.route, run_self(hip, c), c.want(), c.what())
    gates.check("self_reg", "self_fast")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_self_decode_head_dims(hip, dt):
    """Head dim 16 and 96 (generic kernel), 128 and 32 (fast kernel), beam 3 and 20, with a random ancestor table."""
    gates = Gates(dt)
    seen = set()
    for c in A.self_head_dim_cases(dt):
        gates.add(c.route, run_self(hip, c), c.want(), c.what())
        seen.add((c.dh, c.route))
    assert seen == {(16, "self_generic"), (96, "self_generic"), (128, "self_fast"), (32, "self_fast")}
    gates.check("self_fast", "self_generic")


# ---- 2. cross-attention -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_form", ["contiguous", "slice"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_cross_decode(hip, dt, q_form):
    """S = 1 .. 128 x 1 .. 40 rows per image at dh 64, dh 32 / 128 / 16 at three S; one image fully masked, one with only its
    last key live, one key masked elsewhere; q contiguous or a column slice of a [rows, 3D] buffer."""
    gates = Gates(dt)
    for c in A.cross_cases(dt):
        q = c.wide.cuda()[:, c.d:2 * c.d]
        if q_form == "contiguous":
            q = q.contiguous()
        assert q.stride(0) == (c.d if q_form == "contiguous" else 3 * c.d)
        out = torch.full((c.rows + A.EXTRA_ROWS, c.d), SENTINEL, dtype=dt, device="cuda")
        hip.attn_cross_decode(q, c.kv.cuda(), c.mask.cuda(), out, c.n_img, c.rows_per_img, c.s, c.d, c.n_heads, c.scale)
        assert bool((out[c.rows:] == SENTINEL).all()), c.what()
        gates.add(A.cross_route(c.dh, c.s), out[:c.rows], c.want(), c.what())
    gates.check("cross_lds", "cross_fast", "cross_generic")


@pytest.mark.parametrize("dt", [BF16, F16], ids=DT_IDS[1:])
def test_cross_decode_packed(hip, dt):
    """The matrix-core form: every rows_per_img 1 .. 16 x S x both head-dim slot orders.  ``dperm = 1`` (the order the default
    plan of the caption models uses) sums the same dot products in another order, so the same fp64 reference holds."""
    gate = A.Gate("cross_packed", dt, ULP_GATE)
    restated = apart = 0.0
    for c in A.packed_cases(dt):
        want, same = c.want(), c.want_weights_rounded()
        restated = max(restated, A.err_ulps(same.to(dt), want, dt))
        q = c.wide.cuda()[:, c.d:2 * c.d]
        for dperm in (0, 1):
            kp, vt = hip.attn_cross_pack(c.kv.cuda(), c.n_img, c.s, c.d, c.n_heads, dperm=bool(dperm))
            out = torch.full((c.rows + A.EXTRA_ROWS, c.d), SENTINEL, dtype=dt, device="cuda")
            hip.attn_cross_decode_packed(q, kp, vt, c.mask.cuda(), out, c.n_img, c.rows_per_img, c.s, c.d, c.n_heads, c.scale,
                                         dperm=bool(dperm))
            assert bool((out[c.rows:] == SENTINEL).all()), (c.what(), dperm)
            what = dict(c.what(), dperm=dperm)
            gate.add(out[:c.rows], want, what)
            apart = max(apart, A.err_ulps(out[:c.rows], same, dt))
    print(f"[cross_packed_restated] {dt}: the same arithmetic in torch is {restated:.4f} ulp from fp64, the kernel {apart:.4f} ulp from it")
    gate.check()
