"""What the row-wise, pooling and layout tests share (test_rowops_routes_gpu.py, test_pools_layout_gpu.py, test_rowops_ref_cpu.py):
the fp64 and exact-emulation references of the streaming kernels between the GEMMs, their case tables, and the launcher rules
restated in Python (which NV a (D, type) runs, which launches wrap their capped grid).  Plain module, no GPU use: every case
is built on the CPU.

Three kinds of reference, by what the kernel does:
  exact      one or two correctly rounded fp32 operations per element, or a sequential fp32 sum (embed_rows, label_mean,
             avgpool_nhwc, the normalisations): the same IEEE operations run here in torch fp32, bit for bit;
  formula    integer / boolean / permutation results (masks, max pools, layouts): the torch formula;
  fp64       tree-reduced results (layer norm, log-softmax, perplexity, avgpool_rows): fp64 on the same fp32 operands, gated at a
             stated multiple of the error of the CPU fp32 computation on those operands (the ``*_yardsticks`` functions)."""
import torch
import torch.nn.functional as F

from attn_ref import BF16, DT_IDS, DTYPES, F16, F32, ulp  # noqa: F401

DT16, DT16_IDS = [BF16, F16], ["bf16", "f16"]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
SENTINEL = -24576.0          # -3 * 2^13: exact in every type, far from every value a case produces
EXTRA_ROWS = 2
YARD_MULT = 4.0              # every fp64 gate: 4 x the CPU fp32 error (a different, equally valid summation order)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed))


def half_ulp_f32(x):
    """Half the fp32 spacing at the largest |x|: the error a correctly rounded fp32 result may have."""
    m = float(x.double().abs().max())
    if m == 0.0 or m != m or m == float("inf"):
        return 0.0
    _, e = torch.frexp(torch.tensor(m, dtype=torch.float64))
    return 0.5 * 2.0 ** (int(e) - 24)


def abs_err(got, want):
    """max |got - want| in fp64; equal infinities count as no error."""
    got, want = got.double().cpu(), want.double()
    return float(torch.where(got == want, torch.zeros_like(want), (got - want).abs()).max())


# ---- 1. dh_add_layernorm ------------------------------------------------------------------------------------------------------
LN_MAX_D = 4096
LN_NVS = (1, 2, 4, 8, 16)


def vec_elems(dt):
    return 4 if dt == F32 else 8


def ln_route(d, dt):
    """The NV (16-byte vectors per lane) dh_add_layernorm instantiates for a row of ``d`` elements of ``dt``."""
    assert d > 0 and d % 8 == 0 and d <= LN_MAX_D
    per_pass = 64 * vec_elems(dt)              # elements one pass of the wave holds: 256 fp32, 512 16-bit
    return next(nv for nv in LN_NVS if d <= nv * per_pass or nv == 16)


# NV = 16 needs D > 8 * 512 = 4096 in 16 bit, which DH_REQUIRE(D <= 4096) rejects: unreachable, the instantiation stays
LN_REACHABLE = {F32: (1, 2, 4, 8, 16), BF16: (1, 2, 4, 8), F16: (1, 2, 4, 8)}
# per route: its upper boundary, the first width of the next route, and a width whose last pass has dead lanes
LN_WIDTHS = {F32: (8, 248, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096),
             BF16: (8, 504, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096),
             F16: (8, 504, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096)}
LN_ROWS = (1, 3, 4, 5, 37)                     # the tail workgroup with 3, 1, 0, 3, 3 idle waves
LN_FORMS = ("y", "none", "inplace", "eps12")   # y given | y=None | out is x | eps = 1e-12 (else 1e-5)
# "real" rows far from mean 0 / variance 1: one row + LN_OFFSET, one row * LN_SCALE, gamma * LN_GAMMA.  The 16-bit scales are
# tighter so that the derived 16-bit gate stays under one ulp: fp16 spacing at 2^-6 is 1.5e-5, so the CPU fp32 error must stay
# under 1.9e-6, which neither a +100 row (3e-5) nor outputs beyond +-16 (fp32 spacing 2e-6) allow
LN_OFFSET = {F32: 100.0, BF16: 4.0, F16: 2.0}
LN_SCALE = {F32: 50.0, BF16: 4.0, F16: 2.0}
LN_GAMMA = {F32: 1.0, BF16: 1.0, F16: 0.5}
LN_SPIKE = 1000.0                              # exact in every type
LN_SPIKE_GAMMA = 0.125                         # the spike's own output is sqrt(D - 1) * gamma: kept under 8


def ln_ref(v, gamma, beta, eps):
    """fp64 LayerNorm of the rows ``v`` (biased variance, as nn.LayerNorm)."""
    v = v.double()
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def split_planes(w):
    """The fp16 planes of an fp32 tensor, as dh_add_layernorm_f32x stores them: hi = fp16(w), lo = fp16((w - hi) * 2048)."""
    hi = w.to(F16)
    lo = ((w - hi.float()) * 2048.0).to(F16)
    return torch.stack([hi, lo])


class LnCase:
    def __init__(self, flavour, dt, d, rows, form, x, y, gamma, beta):
        self.flavour, self.dt, self.d, self.rows, self.form = flavour, dt, d, rows, form
        self.x, self.y, self.gamma, self.beta = x, (None if form == "none" else y), gamma, beta
        self.eps = 1e-12 if form == "eps12" else 1e-5
        self.nv = ln_route(d, dt)
        assert x.dtype == dt and x.shape == (rows, d) and gamma.dtype == F32 and beta.dtype == F32

    def what(self):
        return f"{self.flavour} {NAME[self.dt]} rows={self.rows} D={self.d} NV={self.nv} {self.form}"

    def v(self):
        """fp32(x + y): the first addition, which the kernel and the reference project both perform in fp32."""
        return self.x.float() if self.y is None else self.x.float() + self.y.float()

    def want(self):
        return ln_ref(self.v(), self.gamma, self.beta, self.eps)

    def cpu_f32(self):
        return F.layer_norm(self.v(), (self.d,), self.gamma, self.beta, self.eps)


def ln_last_pass(d, dt):
    """(pass index, first element) of the last register pass with a live lane."""
    p = (d - 1) // (64 * vec_elems(dt))
    return p, p * 64 * vec_elems(dt)


def ln_dead_lanes(d, dt):
    """Lanes of the last live pass whose vector lies past the row."""
    vn = vec_elems(dt)
    _, d0 = ln_last_pass(d, dt)
    return 64 - (d - d0) // vn


def ln_spike_positions(d, dt):
    """First and last element of the row, of the lane-0 vector of the last live pass, of its lane-63 vector where that is live,
    and of the last live vector of the row."""
    vn = vec_elems(dt)
    _, d0 = ln_last_pass(d, dt)
    pos = [0, d - 1, d0, d0 + vn - 1, d0 + 63 * vn, d0 + 64 * vn - 1, d - vn]
    return sorted({p for p in pos if 0 <= p < d})


def ln_real_cases(dt):
    for wi, d in enumerate(LN_WIDTHS[dt]):
        for rows in LN_ROWS:
            for fi, form in enumerate(LN_FORMS):
                seed = 1000 * wi + 10 * rows + fi
                x, y = randn(rows, d, seed=seed), randn(rows, d, seed=seed + 1)
                x[rows // 2] += LN_OFFSET[dt]
                if rows > 1:
                    x[rows - 1] *= LN_SCALE[dt]
                    y[rows - 1] *= LN_SCALE[dt]
                yield LnCase("real", dt, d, rows, form, x.to(dt), y.to(dt), randn(d, seed=seed + 2) * LN_GAMMA[dt],
                             randn(d, seed=seed + 3))


def ln_spike_cases(dt):
    for wi, d in enumerate(LN_WIDTHS[dt]):
        pos = ln_spike_positions(d, dt)
        x = torch.zeros(len(pos), d)
        x[torch.arange(len(pos)), torch.tensor(pos)] = LN_SPIKE
        for form in ("y", "none"):
            yield LnCase("spike", dt, d, len(pos), form, x.to(dt), torch.zeros(len(pos), d, dtype=dt),
                         randn(d, seed=7000 + wi) * LN_SPIKE_GAMMA, randn(d, seed=7100 + wi))


def ln_const_cases(dt):
    """Every element 3 (= 2 + 1 with y): every partial sum of up to 4096 threes is exact in fp32 in any order, so mean = 3,
    variance = 0, rstd = 1 / sqrt(eps), and the output is beta (rounded once to the type)."""
    for wi, d in enumerate(LN_WIDTHS[dt]):
        for rows in (1, 5):
            for form in LN_FORMS:
                x = torch.full((rows, d), 3.0 if form == "none" else 2.0)
                yield LnCase("const", dt, d, rows, form, x.to(dt), torch.ones(rows, d, dtype=dt), randn(d, seed=8000 + wi),
                             randn(d, seed=8100 + wi))


def kernels_rnd(*shape, seed=0):
    """test_kernels_gpu.rnd: the operand generator of test_add_layernorm_embed_mask."""
    return torch.randn(*shape, generator=gen(seed + sum(shape)))


PLAIN_WIDTHS = (512, 256, 1024)
PLAIN_ATOL = 5e-6            # test_add_layernorm_embed_mask's own tolerance: no gate on its operands may exceed it


def ln_plain_cases():
    """The operands of test_kernels_gpu.test_add_layernorm_embed_mask."""
    for d in PLAIN_WIDTHS:
        yield LnCase("plain", F32, d, 37, "y", kernels_rnd(37, d, seed=1), kernels_rnd(37, d, seed=2), kernels_rnd(d, seed=3),
                     kernels_rnd(d, seed=4))


def ln_gated_cases(dt):
    yield from ln_real_cases(dt)
    yield from ln_spike_cases(dt)
    if dt == F32:
        yield from ln_plain_cases()


def ln_key(c):
    return (c.flavour, NAME[c.dt], c.nv)


def ln_yardsticks():
    """{(flavour, type, NV): worst |F.layer_norm(fp32(x + y)) in fp32 on the CPU - fp64|} over the gated cases."""
    out = {}
    for dt in DTYPES:
        for c in ln_gated_cases(dt):
            out[ln_key(c)] = max(out.get(ln_key(c), 0.0), abs_err(c.cpu_f32(), c.want()))
    return out


def ulp16_gate(f32_gate, dt):
    """An fp32 result within ``f32_gate`` of fp64, rounded once to ``dt``: 0.5 ulp of rounding + the fp32 error in ulps at 2^-6."""
    return 0.5 + f32_gate / float(ulp(torch.tensor(2.0 ** -6, dtype=torch.float64), dt))


# ---- 2. dh_embed_rows ---------------------------------------------------------------------------------------------------------
EMB_D = (8, 64, 512, 520, 4096)
EMB_ROWS = (1, 3, 6, 37)
EMB_GROUPS = ((2, 1), (1, 2), (5, 3))          # (rows_per_img, row_mult)
EMB_POS = (0, 1, 7)
EMB_VOCAB, EMB_TOK_LD, EMB_TOK_OFF, EMB_TOK_W = 50, 12, 2, 9


def embed_ref(tok_emb, pos_emb, start_emb, tokens, rows, rows_per_img, row_mult, pos, scale):
    """fp32(fp32(src / fp32(scale)) + pos_emb[pos]) rounded once to the type; compact row rc reads the start embedding of image
    rc // rows_per_img at position 0, else token [rc * row_mult, pos - 1] (pos without a start embedding)."""
    rc = torch.arange(rows)
    if start_emb is not None and pos == 0:
        src = start_emb[rc // rows_per_img]
    else:
        src = tok_emb[tokens[rc * row_mult, pos - (1 if start_emb is not None else 0)].long()]
    return (src.float() / torch.tensor(scale, dtype=F32) + pos_emb[pos].float()).to(tok_emb.dtype)


# ---- 3. masks -----------------------------------------------------------------------------------------------------------------
MASK_D = (1, 8, 63, 64, 65, 512, 2048)
MASK_ROWS = (1, 4, 5, 37)
MASK_KINDS = ("zero_first", "zero_last", "neg_zero", "subnormal", "nan", "plain")
MASKED = {"zero_first": 1, "zero_last": 1, "neg_zero": 1, "subnormal": 0, "nan": 0, "plain": 0}
MASK_WRAP_CAP = 16384 * 256                    # threads of one trip of pad_mask / autoregressive_mask / mask_or


def smallest_subnormal(dt):
    """fp32: 1e-40 (a subnormal); bf16 2^-133 and fp16 2^-24 from their bit pattern 0x0001."""
    if dt == F32:
        return torch.tensor(1e-40, dtype=F32)
    return torch.tensor([1], dtype=torch.int16).view(dt)[0]


def mask_rows(rows, d, dt, shift):
    """[rows, d] of non-zero values; row i is of kind MASK_KINDS[(i + shift) % 6] -> (tensor, kinds)."""
    g = gen(31 * d + rows + shift)
    e = ((torch.rand(rows, d, generator=g) + 0.5) * (torch.randint(0, 2, (rows, d), generator=g) * 2 - 1)).to(dt)
    kinds = [MASK_KINDS[(i + shift) % len(MASK_KINDS)] for i in range(rows)]
    for i, k in enumerate(kinds):
        if k == "zero_first":
            e[i, 0] = 0.0
        elif k == "zero_last":
            e[i, d - 1] = 0.0
        elif k == "neg_zero":
            e[i, d // 2] = -0.0
        elif k == "subnormal":
            e[i, (2 * d) // 3] = smallest_subnormal(dt)
        elif k == "nan":
            e[i, d // 3] = float("nan")
    return e, kinds


def key_mask_ref(e):
    return (e == 0).any(-1)


def round16_keep_nonzero_ref(x, dt):
    """Round to nearest even; a non-zero value that rounds to zero becomes the smallest subnormal of its sign."""
    h = x.to(dt).view(torch.int16).clone()
    flushed = ((h & 0x7FFF) == 0) & (x != 0)
    h[flushed] |= 1
    return h.view(dt)


def mask_wraps(total):
    return total > MASK_WRAP_CAP


MASK_SMALL = ((1, 1, 1), (2, 3, 5), (3, 7, 4), (2, 33, 65))      # (bs, Lq, Lk), Lq != Lk but for the first
MASK_WRAP = {"pad_mask": (5, 917, 915), "autoregressive_mask": (17, 497), "mask_or": (5, 917, 915)}


# ---- 4. label mean, token log-prob, sequence perplexity -------------------------------------------------------------------------
LM_E, LM_L, LM_N, LM_VOCAB = (1, 255, 256, 257, 600), (1, 3, 17), (1, 7), 20


def label_mean_ref(emb, labels):
    """Sequential fp32 sum over the L positions, one division by fp32(L), rounded once: the kernel's own order."""
    s = torch.zeros(labels.shape[0], emb.shape[1])
    for j in range(labels.shape[1]):
        s = s + emb[labels[:, j]].float()
    return (s / torch.tensor(float(labels.shape[1]), dtype=F32)).to(emb.dtype)


LP_V = (1, 2, 255, 256, 257, 1000, 36541)
LP_KINDS = ("plain", "neg_inf", "max_last", "scaled")
LP_PAD = 5                                     # ldl = V + LP_PAD


def logprob_rows(v, kind, rows, seed):
    """fp32 logits [rows, v] of ``kind`` and in-range targets (0, v - 1, then random), never on a -inf entry."""
    g = gen(seed)
    x = torch.randn(rows, v, generator=g)
    t = torch.randint(0, v, (rows,), generator=g)
    t[0] = 0
    if rows > 1:
        t[1] = v - 1
    if kind == "neg_inf" and v > 1:            # (V = 1: the only entry -inf has no log-softmax)
        x[:, 1 if v > 2 else 0] = float("-inf")
        t[t == (1 if v > 2 else 0)] = v - 1
    elif kind == "max_last":
        x[:, v - 1] = x.max(-1).values + 1.0
    elif kind == "scaled":
        x *= 30.0                              # exp underflows for most entries
    return x, t


def logprob_cases():
    for vi, v in enumerate(LP_V):
        for ki, kind in enumerate(LP_KINDS):
            for rows in (1, 5):
                yield (v, kind, rows) + logprob_rows(v, kind, rows, 100 * vi + 10 * ki + rows)


def logprob_ref(x, t):
    return torch.log_softmax(x.double(), -1).gather(-1, t[:, None]).squeeze(-1)


def logprob_cpu_f32(x, t):
    return torch.log_softmax(x, -1).gather(-1, t[:, None]).squeeze(-1)


def logprob_yardsticks():
    """{(V, kind): max(worst CPU fp32 log_softmax error against fp64, half an fp32 ulp of the largest result)}."""
    out = {}
    for v, kind, rows, x, t in logprob_cases():
        want = logprob_ref(x, t)
        out[(v, kind)] = max(out.get((v, kind), 0.0), abs_err(logprob_cpu_f32(x, t), want), half_ulp_f32(want))
    return out


PP_L, PP_PAD = (1, 63, 64, 65, 200), 0


def perplexity_case(L):
    """logp fp32 [4, L], targets, lengths: all tokens | length under the token count | all pad but one token | random pads."""
    g = gen(900 + L)
    logp = -2.0 * torch.rand(4, L, generator=g)
    targets = torch.randint(1, 50, (4, L), generator=g)
    targets[2] = PP_PAD
    targets[2, L // 2] = 7
    targets[3, torch.rand(L, generator=g) < 0.4] = PP_PAD
    count = (targets != PP_PAD).sum(-1)
    lengths = count.clamp(min=1)
    lengths[1] = max(1, L // 2)
    return logp, targets, lengths


def perplexity_ref(logp, targets, lengths, dtype=torch.float64):
    """metrics.perplexity per sequence: exp(-sum_t [target != pad] logp / length), from the same fp32 logp."""
    lv = logp.to(dtype) / lengths[:, None].to(dtype)
    lv = lv.masked_fill(targets == PP_PAD, 0.0)
    return (-lv.sum(-1)).exp()


def perplexity_yardsticks():
    out = {}
    for L in PP_L:
        logp, targets, lengths = perplexity_case(L)
        want = perplexity_ref(logp, targets, lengths)
        out[L] = max(abs_err(perplexity_ref(logp, targets, lengths, F32), want), half_ulp_f32(want))
    return out


# ---- 5. pools and layout --------------------------------------------------------------------------------------------------------
POOL_HW = tuple((h, w) for h in (1, 2, 3, 7, 8, 15) for w in (1, 2, 3, 7, 8, 15) if h != w)
POOL_C, POOL_C_F32, POOL_N = (8, 24, 64), (4, 12), (1, 3)


def negative(*shape, seed):
    """All-negative values: a padding cell read as 0 would win the maximum."""
    return -(randn(*shape, seed=seed).abs() + 0.1)


def maxpool_ref(x):
    return F.max_pool2d(x, 3, 2, 1)


AVG_HW = (1, 7, 8, 9, 49, 50)                  # below, at and above the eight-position round of avgpool_nhwc
AVG_C = (8, 2048)
ROWS_HW = (1, 49, 63, 64, 65, 200)
ROWS_NC = ((1, 1), (1, 2), (1, 3), (1, 4), (3, 7))      # N * C = 1, 2, 3, 0, 1 modulo 4


def avgpool_seq_ref(x):
    """x [N, HW, C] -> [N, C]: sequential fp32 sum over the positions, one division by fp32(HW), rounded once."""
    s = torch.zeros(x.shape[0], x.shape[2])
    for j in range(x.shape[1]):
        s = s + x[:, j].float()
    return (s / torch.tensor(float(x.shape[1]), dtype=F32)).to(x.dtype)


def avgpool_rows_case(n, c, hw):
    return randn(n, c, hw, 1, seed=50 * hw + n * c) + 0.5


def avgpool_rows_yardsticks():
    out = {}
    for hw in ROWS_HW:
        for n, c in ROWS_NC:
            x = avgpool_rows_case(n, c, hw)
            want = x.double().mean(dim=(2, 3))
            out[hw] = max(out.get(hw, 0.0), abs_err(x.mean(dim=(2, 3)), want), half_ulp_f32(want))
    return out


LAYOUT_DIMS = (1, 31, 32, 33, 49, 100)


def pack_nhwc8_ref(x, dt):
    """NCHW fp32 -> channels-last [N, H, W, 8] of ``dt``: one rounding, channels C..7 zero."""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, 8, dtype=dt)
    out[..., :c] = x.permute(0, 2, 3, 1).to(dt)
    return out


def nhwc_pad_ref(x, cp):
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, cp)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


NORM_MEAN = torch.tensor([0.485, 0.456, 0.406, 0.5])
NORM_STD = torch.tensor([0.229, 0.224, 0.225, 0.25])


def normalize_ref(x, mean, std):
    """uint8 [N, H, W, C] -> fp32 [N, C, H, W]: ((x / 255) - mean) / std, three correctly rounded fp32 operations."""
    return ((x.float() / 255.0 - mean) / std).permute(0, 3, 1, 2).contiguous()


def bytes_image(n, h, w, c, seed):
    """uint8 [n, h, w, c] that holds all 256 byte values in every channel."""
    assert n * h * w >= 256
    g = gen(seed)
    x = torch.randint(0, 256, (n * h * w, c), generator=g, dtype=torch.uint8)
    for ch in range(c):
        x[torch.randperm(n * h * w, generator=g)[:256], ch] = torch.arange(256, dtype=torch.uint8)
    return x.view(n, h, w, c)


# capped launchers: (threads of one trip, the work items of the wrap case); every wrap case is less than 10 % over its cap
WRAP = {
    "maxpool3x3s2": (16384 * 256, dict(shape=(3, 64, 299, 299))),               # 3 * 64 * 150 * 150 outputs
    "maxpool3x3s2_nhwc": (16384 * 256, dict(shape=(4100, 3, 3, 2048))),          # 4100 * 2 * 2 * 256 eight-channel groups
    "normalize_u8_hwc": (32768 * 256, dict(shape=(1, 2897, 2897, 3))),           # pixels
    "normalize_pack_u8": (32768 * 256, dict(shape=(1, 2897, 2897, 3))),
    "pack_nchw_to_nhwc8": (32768 * 256, dict(shape=(1, 3, 2897, 2897))),
    "round16_keep_nonzero": (65536 * 256, dict(shape=(16777216 + 12345,))),
}


def work_items(name, shape):
    """The number of grid-stride items the launcher of ``name`` spreads over its capped grid."""
    if name == "maxpool3x3s2":
        n, c, h, w = shape
        return n * c * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    if name == "maxpool3x3s2_nhwc":
        n, h, w, c = shape
        return n * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * (c // 8)
    if name in ("normalize_u8_hwc", "normalize_pack_u8"):
        return shape[0] * shape[1] * shape[2]
    if name == "pack_nchw_to_nhwc8":
        return shape[0] * shape[2] * shape[3]
    if name == "round16_keep_nonzero":
        return shape[0]
    raise KeyError(name)


def wraps(name, shape):
    return work_items(name, shape) > WRAP[name][0]
