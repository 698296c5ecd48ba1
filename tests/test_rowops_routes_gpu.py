"""The row-wise kernels of rowops.hip on every launcher route, shape edge, call form and storage type, against the references of
rowops_ref.py (cases, references and the restated launcher rules live there; tests/test_rowops_ref_cpu.py proves the references
against torch in fp64, the case tables against the route sets asserted here, and recomputes the yardstick tables below).

  dh_add_layernorm        NV = 1 | 2 | 4 | 8 | 16 register passes by width (fp32 256 elements a pass, 16 bit 512; NV = 16 is
                          unreachable in 16 bit under D <= 4096), widths at each route's boundary and with dead lanes in the last
                          pass, rows that leave 0, 1 and 3 waves of the tail workgroup idle, y given | None | in place, both eps
  dh_add_layernorm_f32x   the same fp32 cases: output bit-equal to dh_add_layernorm, planes bit-equal to the CPU split, range flag
  dh_embed_rows           bit exact; dh_enc_key_mask / dh_enc_nonzero_rows / pad / autoregressive / or masks: exact
  dh_label_mean           bit exact (sequential fp32 sum); dh_token_logprob, dh_seq_perplexity: fp64

Every gate is one of: exact equality; YARD_MULT = 4 x a tabulated error of the CPU fp32 computation of the same operands against
fp64 (the tables below -- measured on the CPU reference, never on the kernel); or, for a 16-bit layer norm, the derived
0.5 + fp32 gate / ulp(2^-6) ulps at max(|want|, 2^-6) (rowops_ref.ulp16_gate), which no entry may push over one ulp.  Outputs
go into sentinel-filled buffers with spare rows where the wrapper takes ``out``; what the call does not address keeps the
sentinel.  Every test prints its worst error per (kernel, route, type)."""
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_ref as R  # noqa: E402
from attn_ref import ulps  # noqa: E402
from rowops_ref import BF16, DT_IDS, DTYPES, F16, F32, NAME  # noqa: E402

# Worst |F.layer_norm(fp32(x + y)) on the CPU in fp32 - fp64 layer norm of fp32(x + y)| over the cases of (flavour, type, NV);
# the gate is YARD_MULT x the entry.  "plain": the operands of test_kernels_gpu.test_add_layernorm_embed_mask.
LN_YARD = {
    ("plain", "f32", 1): 7.993e-07,
    ("plain", "f32", 2): 8.945e-07,
    ("plain", "f32", 4): 9.241e-07,
    ("real", "bf16", 1): 1.513e-06,
    ("real", "bf16", 2): 1.706e-06,
    ("real", "bf16", 4): 2.261e-06,
    ("real", "bf16", 8): 1.739e-06,
    ("real", "f16", 1): 6.387e-07,
    ("real", "f16", 2): 6.907e-07,
    ("real", "f16", 4): 8.273e-07,
    ("real", "f16", 8): 7.062e-07,
    ("real", "f32", 1): 3.207e-05,
    ("real", "f32", 2): 2.602e-05,
    ("real", "f32", 4): 3.424e-05,
    ("real", "f32", 8): 1.977e-05,
    ("real", "f32", 16): 2.504e-05,
    ("spike", "bf16", 1): 4.895e-07,
    ("spike", "bf16", 2): 7.080e-07,
    ("spike", "bf16", 4): 7.846e-07,
    ("spike", "bf16", 8): 1.775e-06,
    ("spike", "f16", 1): 4.895e-07,
    ("spike", "f16", 2): 7.080e-07,
    ("spike", "f16", 4): 7.846e-07,
    ("spike", "f16", 8): 1.775e-06,
    ("spike", "f32", 1): 1.257e-07,
    ("spike", "f32", 2): 2.096e-07,
    ("spike", "f32", 4): 5.956e-07,
    ("spike", "f32", 8): 4.771e-07,
    ("spike", "f32", 16): 8.163e-07,
}
# max(worst CPU fp32 torch.log_softmax error against fp64, half an fp32 ulp of the result) over the rows of (V, kind)
LP_YARD = {
    (1, "plain"): 0.000e+00, (1, "neg_inf"): 0.000e+00, (1, "max_last"): 0.000e+00, (1, "scaled"): 0.000e+00,
    (2, "plain"): 5.960e-08, (2, "neg_inf"): 0.000e+00, (2, "max_last"): 1.192e-07, (2, "scaled"): 1.907e-06,
    (255, "plain"): 2.767e-07, (255, "neg_inf"): 2.647e-07, (255, "max_last"): 4.967e-07, (255, "scaled"): 3.926e-06,
    (256, "plain"): 2.384e-07, (256, "neg_inf"): 4.335e-07, (256, "max_last"): 2.767e-07, (256, "scaled"): 7.629e-06,
    (257, "plain"): 2.779e-07, (257, "neg_inf"): 4.853e-07, (257, "max_last"): 4.055e-07, (257, "scaled"): 7.629e-06,
    (1000, "plain"): 4.768e-07, (1000, "neg_inf"): 4.768e-07, (1000, "max_last"): 4.768e-07, (1000, "scaled"): 7.629e-06,
    (36541, "plain"): 4.768e-07, (36541, "neg_inf"): 8.573e-07, (36541, "max_last"): 8.935e-07, (36541, "scaled"): 1.454e-05,
}
# the same for the fp32 statement of metrics.perplexity per sequence, by L
PP_YARD = {1: 2.384e-07, 63: 2.384e-07, 64: 4.593e-07, 65: 9.066e-07, 200: 4.871e-07}

# Conditions on the tables, not measurements: the gate on the operands of test_add_layernorm_embed_mask is no looser than that
# test's 5e-6, and no 16-bit layer norm gate is above one ulp.
assert all(R.YARD_MULT * v <= R.PLAIN_ATOL for k, v in LN_YARD.items() if k[0] == "plain")
assert all(R.ulp16_gate(R.YARD_MULT * v, dt) <= 1.0 for dt in (BF16, F16) for k, v in LN_YARD.items() if k[1] == NAME[dt])


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
    print(f"[test_rowops_routes_gpu] module wall time {time.time() - t0:.1f} s")


def full(shape, dt):
    return torch.full(shape, R.SENTINEL, dtype=dt, device="cuda")


def kept(t):
    return bool((t == R.SENTINEL).all())


def dev(x):
    return None if x is None else x.cuda()


class Worst:
    """Worst error per key, printed and asserted against ``gate(key)`` at the end of a test."""

    def __init__(self, kernel, unit):
        self.kernel, self.unit, self.worst = kernel, unit, {}

    def add(self, key, err, what):
        if key not in self.worst or err > self.worst[key][0]:
            self.worst[key] = (err, what)

    def check(self, gate):
        bad = []
        for key, (err, what) in self.worst.items():
            print(f"[{self.kernel}] {key}: worst {err:.4g} {self.unit} (gate {gate(key):.4g}) at {what}")
            if not err <= gate(key):
                bad.append((key, err, gate(key), what))
        assert not bad, bad


# ---- 1. dh_add_layernorm ------------------------------------------------------------------------------------------------------
def run_ln(hip, c):
    """One hip.add_layernorm call in the form of case ``c``: the [rows, d] result, after the sentinel checks."""
    buf = full((c.rows + R.EXTRA_ROWS, c.d), c.dt)
    out = buf[:c.rows]
    if c.form == "inplace":
        out.copy_(c.x)
        got = hip.add_layernorm(out, dev(c.y), c.gamma.cuda(), c.beta.cuda(), out=out, eps=c.eps)
    else:
        got = hip.add_layernorm(c.x.cuda(), dev(c.y), c.gamma.cuda(), c.beta.cuda(), out=out, eps=c.eps)
    assert got is out and kept(buf[c.rows:]), c.what()
    return out


def ln_gate(key, dt):
    g = R.YARD_MULT * LN_YARD[key]
    return g if dt == F32 else R.ulp16_gate(g, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_layernorm_routes(hip, dt):
    """real, spike and (fp32) plain operands against the fp64 layer norm of fp32(x + y), on every reachable NV."""
    worst, routes = Worst("add_layernorm", "abs" if dt == F32 else "ulp"), set()
    for c in R.ln_gated_cases(dt):
        got, want = run_ln(hip, c), c.want()
        err = R.abs_err(got, want) if dt == F32 else float(ulps(got, want, dt).max())
        worst.add(R.ln_key(c), err, c.what())
        routes.add(c.nv)
    assert routes == set(R.LN_REACHABLE[dt])
    worst.check(lambda key: ln_gate(key, dt))


def test_layernorm_without_out(hip):
    """``out=None``: the wrapper's own buffer, same bits as the call with ``out``."""
    for dt in DTYPES:
        c = next(iter(R.ln_real_cases(dt)))
        got = hip.add_layernorm(c.x.cuda(), dev(c.y), c.gamma.cuda(), c.beta.cuda(), eps=c.eps)
        assert got.shape == c.x.shape and got.dtype == dt and got.is_contiguous() and torch.equal(got, run_ln(hip, c))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_layernorm_constant_rows_give_beta(hip, dt):
    """Variance 0: rstd = 1 / sqrt(eps) (316 or 10^6) multiplies an exact 0, the output is beta rounded once."""
    n = 0
    for c in R.ln_const_cases(dt):
        got = run_ln(hip, c).cpu()
        assert torch.equal(got, c.beta.to(dt).expand(c.rows, c.d)), c.what()
        n += 1
    print(f"[add_layernorm] const {NAME[dt]}: {n} cases equal beta")


def f32_cases():
    yield from R.ln_gated_cases(F32)
    yield from R.ln_const_cases(F32)


def test_layernorm_f32x_matches_and_splits(hip):
    """dh_add_layernorm_f32x at every fp32 case: the fp32 output bit-equal to dh_add_layernorm, the planes bit-equal to the CPU
    split of that output (hi = fp16(w), lo = fp16((w - hi) * 2048): the subtraction and the product are exact in fp32), and the
    stream's range flag clear -- set only by an output element of magnitude >= 65504, and cleared again by reading it."""
    from deephumor_amd import f32xp
    hip.f32x_take_overflow()
    n, routes = 0, set()
    for c in f32_cases():
        if c.form == "inplace":
            continue                                            # (the f32x wrapper owns its output)
        want = run_ln(hip, c)
        out, planes = f32xp.add_layernorm(c.x.cuda(), dev(c.y), c.gamma.cuda(), c.beta.cuda(), eps=c.eps)
        assert torch.equal(out, want), c.what()
        assert planes.shape == (2, c.rows, c.d) and torch.equal(planes.cpu().view(torch.int16), R.split_planes(out.cpu()).view(torch.int16)), c.what()
        assert hip.f32x_take_overflow() is False, c.what()
        routes.add(c.nv)
        n += 1
    assert routes == set(R.LN_REACHABLE[F32])
    c = next(iter(R.ln_const_cases(F32)))
    beta = c.beta.clone()
    beta[c.d - 3] = -65504.0
    out, _ = f32xp.add_layernorm(c.x.cuda(), dev(c.y), c.gamma.cuda(), beta.cuda(), eps=c.eps)
    assert float(out[0, c.d - 3]) == -65504.0
    assert hip.f32x_take_overflow() is True and hip.f32x_take_overflow() is False
    f32xp.add_layernorm(c.x.cuda(), dev(c.y), c.gamma.cuda(), c.beta.cuda(), eps=c.eps)
    assert hip.f32x_take_overflow() is False
    print(f"[add_layernorm_f32x] f32: {n} cases bit-equal, planes exact, range flag clear; one overflow case flagged once")


def test_layernorm_rejects_bad_arguments(hip):
    """What dh_add_layernorm rejects before any launch: D % 8 != 0, D > 4096, a misaligned gamma / beta."""
    for d in (12, 4104):
        out = full((3, d), F32)
        with pytest.raises(RuntimeError, match="dh_add_layernorm"):
            hip.add_layernorm(torch.zeros(3, d, device="cuda"), None, torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"), out=out)
        torch.cuda.synchronize()
        assert kept(out)
    d, out = 64, full((3, 64), F32)
    odd = torch.ones(d + 1, device="cuda")[1:]
    assert odd.data_ptr() % 16 != 0 and odd.is_contiguous()
    for g, b in ((odd, torch.zeros(d, device="cuda")), (torch.ones(d, device="cuda"), odd)):
        with pytest.raises(RuntimeError, match="dh_add_layernorm"):
            hip.add_layernorm(torch.zeros(3, d, device="cuda"), None, g, b, out=out)
    torch.cuda.synchronize()
    assert kept(out)


# ---- 2. dh_embed_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_embed_rows_is_bit_exact(hip, dt):
    """x = fp32(fp32(src / fp32(scale)) + pos) rounded once, over widths below, at and past one 64-lane pass, every row grouping,
    positions with and without the start slot, and a token table whose row stride differs from its width."""
    n = 0
    for d in R.EMB_D:
        scale = math.sqrt(d)
        tok, pos_emb = R.randn(R.EMB_VOCAB, d, seed=d + 1).to(dt), R.randn(8, d, seed=d + 2).to(dt)
        tok_g, pos_g = tok.cuda(), pos_emb.cuda()
        for rows in R.EMB_ROWS:
            for rpi, mult in R.EMB_GROUPS:
                start = R.randn((rows - 1) // rpi + 1, d, seed=d + 3).to(dt)
                start_g = start.cuda()
                ids_buf = torch.randint(0, R.EMB_VOCAB, (rows * mult, R.EMB_TOK_LD), generator=R.gen(rows * mult), dtype=torch.int32)
                ids = ids_buf[:, R.EMB_TOK_OFF:R.EMB_TOK_OFF + R.EMB_TOK_W]
                ids_g = ids_buf.cuda()[:, R.EMB_TOK_OFF:R.EMB_TOK_OFF + R.EMB_TOK_W]
                assert ids_g.stride(0) == R.EMB_TOK_LD != ids_g.shape[1]
                for pos in R.EMB_POS:
                    for with_start in (True, False):
                        forms = (ids_g, None) if with_start and pos == 0 else (ids_g,)
                        want = R.embed_ref(tok, pos_emb, start if with_start else None, ids, rows, rpi, mult, pos, scale)
                        for tokens in forms:
                            buf = full((rows + R.EXTRA_ROWS, d), dt)
                            got = hip.embed_rows(tok_g, pos_g, start_g if with_start else None, tokens, buf, rows, rpi, mult, pos, scale)
                            what = (NAME[dt], d, rows, rpi, mult, pos, with_start, tokens is None)
                            assert got is buf and torch.equal(buf[:rows].cpu(), want), what
                            assert kept(buf[rows:]), what
                            n += 1
    print(f"[embed_rows] {NAME[dt]}: {n} cases bit exact")


# ---- 3. masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_encoder_masks_are_exact(hip, dt):
    """enc_key_mask = not enc_nonzero_rows = (e == 0).any(-1) in the storage type: a zero at either end of the row and a -0.0
    mask it, a subnormal of the type and a NaN do not."""
    n = 0
    for d in R.MASK_D:
        for rows in R.MASK_ROWS:
            for shift in range(1 if rows == 37 else len(R.MASK_KINDS)):
                e, kinds = R.mask_rows(rows, d, dt, shift)
                want = R.key_mask_ref(e)
                assert want.tolist() == [bool(R.MASKED[k]) for k in kinds]
                eg = e.cuda()
                key = hip.enc_key_mask(eg)
                nz = hip.enc_nonzero_rows(eg.view(1, rows, d))
                assert key.dtype == torch.uint8 and key.shape == (rows,) and nz.dtype == torch.int64 and nz.shape == (1, rows)
                assert torch.equal(key.cpu().bool(), want), (NAME[dt], d, rows, kinds, key.tolist())
                assert torch.equal(nz.cpu()[0], (~want).long()), (NAME[dt], d, rows, kinds, nz.tolist())
                n += 1
    print(f"[enc_key_mask / enc_nonzero_rows] {NAME[dt]}: {n} cases exact")


@pytest.mark.parametrize("dt", R.DT16, ids=R.DT16_IDS)
def test_round16_keep_nonzero_feeds_the_key_mask(hip, dt):
    """Tiny fp32 features through round16_keep_nonzero straight into enc_key_mask: never masked (the chain the fp16 encoder
    relies on; a compare that flushes denormals would mask them), and the rounding itself equals its CPU statement."""
    tiny = torch.tensor([1e-10, -1e-12, 1e-30, -1e-40, 3e-8, -2.9e-8, 1e-20, 1.4e-45])
    for rows, d in ((1, 8), (5, 64), (4, 65), (37, 2048)):
        x = tiny[torch.randint(0, len(tiny), (rows, d), generator=R.gen(rows + d))]
        x[0, 0] = 1.0
        assert bool((x != 0).all())
        got = hip.round16_keep_nonzero(x.cuda(), dt)
        assert torch.equal(got.cpu().view(torch.int16), R.round16_keep_nonzero_ref(x, dt).view(torch.int16)), (NAME[dt], rows, d)
        assert bool((got.cpu().float() != 0).all())
        assert hip.enc_key_mask(got).cpu().tolist() == [0] * rows, (NAME[dt], rows, d)
        x[rows - 1, d - 1] = 0.0
        assert hip.enc_key_mask(hip.round16_keep_nonzero(x.cuda(), dt)).cpu().tolist() == [0] * (rows - 1) + [1]
    print(f"[round16_keep_nonzero -> enc_key_mask] {NAME[dt]}: tiny features stay keys")


def test_module_masks_match_the_torch_formulas(hip):
    """pad_mask, autoregressive_mask and mask_or at small odd shapes and one shape each just past the 4,194,304 elements of one
    trip of the capped grid (the second trip of the grid-stride loop)."""
    shapes = [(s, False) for s in R.MASK_SMALL] + [(R.MASK_WRAP["pad_mask"], True)]
    for (bs, lq, lk), wrap in shapes:
        assert R.mask_wraps(bs * lq * lk) == wrap
        for pad in (0, 3):
            key = torch.randint(0, 5, (bs, lk), generator=R.gen(lq + lk + pad))
            got = hip.pad_mask(torch.empty(bs, lq, device="cuda"), key.cuda(), pad_index=pad)
            want = (key == pad)[:, None, :].expand(bs, lq, lk)
            assert got.dtype == torch.bool and torch.equal(got.cpu(), want), ("pad_mask", bs, lq, lk, pad)
        a = torch.rand(bs, lq, lk, generator=R.gen(bs + lq)) < 0.3
        b = torch.rand(bs, lq, lk, generator=R.gen(bs + lk + 1)) < 0.3
        ag = a.cuda()
        got = hip.mask_or(ag, b.cuda())
        assert got.dtype == torch.bool and torch.equal(got.cpu(), a | b) and torch.equal(ag.cpu(), a), ("mask_or", bs, lq, lk)
    for bs, L in [(1, 1), (2, 5), (3, 33), R.MASK_WRAP["autoregressive_mask"]]:
        got = hip.autoregressive_mask(torch.empty(bs, L, device="cuda"))
        want = torch.triu(torch.ones(L, L), 1).bool()[None].expand(bs, L, L)
        assert got.dtype == torch.bool and torch.equal(got.cpu(), want), ("autoregressive_mask", bs, L)
    assert R.mask_wraps(R.MASK_WRAP["autoregressive_mask"][0] * R.MASK_WRAP["autoregressive_mask"][1] ** 2)
    print("[pad_mask / autoregressive_mask / mask_or] exact, second grid trip included")


# ---- 4. label mean, token log-prob, sequence perplexity -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_label_mean_is_bit_exact(hip, dt):
    """The kernel's own order (sequential fp32 sum over L, one division, one rounding) on repeated labels, into a column window
    of a wider sentinel buffer."""
    n = 0
    for e in R.LM_E:
        emb = R.randn(R.LM_VOCAB, e, seed=e).to(dt)
        for L in R.LM_L:
            for N in R.LM_N:
                labels = torch.randint(0, R.LM_VOCAB, (N, L), generator=R.gen(e + L + N))
                if L > 1:
                    labels[:, 1] = labels[:, 0]
                buf = full((N + R.EXTRA_ROWS, e + 5), dt)
                out = buf[:N, 3:3 + e]
                assert hip.label_mean(emb.cuda(), labels.cuda(), out) is out
                assert torch.equal(out.cpu(), R.label_mean_ref(emb, labels)), (NAME[dt], e, L, N)
                assert kept(buf[N:]) and kept(buf[:N, :3]) and kept(buf[:N, 3 + e:]), (NAME[dt], e, L, N)
                n += 1
    print(f"[label_mean] {NAME[dt]}: {n} cases bit exact")


def test_token_logprob_against_fp64(hip):
    """log_softmax(logits)[target] against fp64 of the same fp32 logits, rows wider than V; out-of-range targets give exactly 0."""
    worst = Worst("token_logprob", "abs")
    for v, kind, rows, x, t in R.logprob_cases():
        buf = torch.full((rows, v + R.LP_PAD), 1e30)
        buf[:, :v] = x
        xg = buf.cuda()[:, :v]
        assert xg.stride(0) == v + R.LP_PAD
        got = hip.token_logprob(xg, t.cuda())
        assert got.shape == (rows,) and got.dtype == F32
        worst.add((v, kind), R.abs_err(got, R.logprob_ref(x, t)), f"V={v} {kind} rows={rows}")
        bad = torch.tensor([-1, v] * rows)[:rows]
        assert hip.token_logprob(xg, bad.cuda()).cpu().tolist() == [0.0] * rows, (v, kind, rows)
    assert set(worst.worst) == set(LP_YARD)
    worst.check(lambda key: R.YARD_MULT * LP_YARD[key])


def test_seq_perplexity_against_fp64(hip):
    """exp(-sum of the non-pad log-probs / length) against fp64 from the same fp32 log-probs: L around the 64-lane wave, a length
    under the token count, a sequence of one token."""
    worst = Worst("seq_perplexity", "abs")
    for L in R.PP_L:
        logp, targets, lengths = R.perplexity_case(L)
        got = hip.seq_perplexity(logp.cuda(), targets.cuda(), lengths.cuda(), pad_index=R.PP_PAD)
        assert got.shape == (4,) and got.dtype == F32
        worst.add(L, R.abs_err(got, R.perplexity_ref(logp, targets, lengths)), f"L={L}")
    worst.check(lambda key: R.YARD_MULT * PP_YARD[key])


# ---- 6. wrapper contracts -------------------------------------------------------------------------------------------------------
def right_or_refused(call, want):
    """A wrapper given a view it cannot address either refuses it (AssertionError) or returns the right answer."""
    try:
        got = call()
    except AssertionError:
        return "refused"
    assert torch.equal(got.cpu(), want), "silently wrong"
    return "right"


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rowops_wrappers_refuse_or_answer(hip, dt):
    """Row-strided views of a wider buffer, 16-bit gamma / beta and int64 tokens: never a silent wrong answer."""
    rows, d = 5, 64
    c = R.LnCase("real", dt, d, rows, "y", R.randn(rows, d, seed=1).to(dt), R.randn(rows, d, seed=2).to(dt), R.randn(d, seed=3),
                 R.randn(d, seed=4))
    want = run_ln(hip, c).cpu()
    wide = lambda t: torch.cat([t, t + 1], 1).cuda()[:, :t.shape[1]]      # noqa: E731  (row stride 2 * width)
    x, y, g, b = c.x.cuda(), c.y.cuda(), c.gamma.cuda(), c.beta.cuda()
    res = {}
    res["ln x"] = right_or_refused(lambda: hip.add_layernorm(wide(c.x), y, g, b), want)
    res["ln y"] = right_or_refused(lambda: hip.add_layernorm(x, wide(c.y), g, b), want)
    buf = full((rows, 2 * d), dt)
    res["ln out"] = right_or_refused(lambda: hip.add_layernorm(x, y, g, b, out=buf[:, :d]), want)
    assert res["ln out"] == "right" or kept(buf)
    res["ln gamma16"] = right_or_refused(lambda: hip.add_layernorm(x, y, g.to(BF16), b), want)
    res["ln beta16"] = right_or_refused(lambda: hip.add_layernorm(x, y, g, b.to(F16)), want)

    tok, pos_emb, start = R.randn(20, d, seed=5).to(dt), R.randn(4, d, seed=6).to(dt), R.randn(rows, d, seed=7).to(dt)
    ids = torch.randint(0, 20, (rows, 4), generator=R.gen(8), dtype=torch.int32)
    for pos, key in ((2, "tok"), (0, "start")):
        want = R.embed_ref(tok, pos_emb, start, ids, rows, 1, 1, pos, 8.0)
        args = lambda **kw: [kw.get("tok", tok.cuda()), kw.get("pos", pos_emb.cuda()), kw.get("start", start.cuda()),   # noqa: E731
                             kw.get("ids", ids.cuda())]
        out = lambda: torch.empty(rows, d, dtype=dt, device="cuda")       # noqa: E731
        res[f"embed {key} tok_emb"] = right_or_refused(lambda: hip.embed_rows(*args(tok=wide(tok)), out(), rows, 1, 1, pos, 8.0), want)
        res[f"embed {key} pos_emb"] = right_or_refused(lambda: hip.embed_rows(*args(pos=wide(pos_emb)), out(), rows, 1, 1, pos, 8.0), want)
        res[f"embed {key} start_emb"] = right_or_refused(lambda: hip.embed_rows(*args(start=wide(start)), out(), rows, 1, 1, pos, 8.0), want)
        res[f"embed {key} int64"] = right_or_refused(lambda: hip.embed_rows(*args(ids=ids.long().cuda()), out(), rows, 1, 1, pos, 8.0), want)
        buf = full((rows, 2 * d), dt)
        res[f"embed {key} x"] = right_or_refused(lambda: hip.embed_rows(*args(), buf[:, :d], rows, 1, 1, pos, 8.0), want)
        assert res[f"embed {key} x"] == "right" or kept(buf)

    e, _ = R.mask_rows(rows, d, dt, 0)
    res["enc_key_mask"] = right_or_refused(lambda: hip.enc_key_mask(wide(e)).bool(), R.key_mask_ref(e))
    res["enc_nonzero_rows"] = right_or_refused(lambda: hip.enc_nonzero_rows(wide(e)[None]), (~R.key_mask_ref(e)).long()[None])
    print(f"[wrappers] {NAME[dt]}: {res}")
