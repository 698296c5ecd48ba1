"""What the dense-linear tests share (test_linear_routes_gpu.py, test_linear_ref_cpu.py): dh_linear and dh_linear_ln stated
plainly in fp64, the restated route rules of their launchers, and the cases of every tile route, ring depth, shape edge,
epilogue form and stride with their operands and expected results.  Plain module, no GPU use: the cases are built on the CPU.

Every case set comes in two operand flavours.  "int": operand entries are integers in [-3, 3], bias / shift / residual are
integers in [-8, 8] and scale is a power of two, so every product and every partial sum is an integer (or a half-integer)
below 2^24 -- exact in fp32 in ANY accumulation order; the fp32 result is that number and a 16-bit output is it rounded once:
compared with torch.equal.  "real": randn operands with w / sqrt(K), compared with fp64 in ulps (16-bit outputs) or by absolute
error (fp32 outputs)."""
import functools

import torch

from attn_ref import BF16, F16, F32, F32_ATOL, ULP_FLOOR, Gate, ulps  # noqa: F401  (re-exported for the two test modules)
from lstm_ref import DT16, DT16_IDS, AbsGate  # noqa: F401

EXTRA_ROWS = 16                                               # sentinel rows behind every output buffer
SENTINEL = 768.0                                              # exact in every type (the LSTM tests' sentinel)
FLAVOURS = ("int", "real")
NS = {"r4": 4, "r8": 8, "r3": 3, "r2": 2}                     # LDS ring depth of the 64 x 64 16-bit kernels


def cdiv(a, b):
    return -(-a // b)


def roundup(a, b):
    return cdiv(a, b) * b


# ---- the references ---------------------------------------------------------------------------------------------------------
def epilogue_ref(acc, bias=None, scale=None, shift=None, residual=None, relu=False):
    y = acc
    if bias is not None:
        y = y + bias.double()
    if scale is not None:
        y = y * scale.double() + shift.double()
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def linear_ref(a, w, bias=None, scale=None, shift=None, residual=None, relu=False):
    """act((a @ w.T + bias) * scale + shift + residual) in fp64, on the operands as the kernel sees them."""
    return epilogue_ref(a.double() @ w.double().t(), bias, scale, shift, residual, relu)


def row_norm(y, eps):
    """(y - mu) * rstd per row, mean and (population) variance taken from the row itself in fp64."""
    y = y.double()
    mu = y.mean(1, keepdim=True)
    var = ((y - mu) ** 2).mean(1, keepdim=True)
    return (y - mu) / torch.sqrt(var + eps)


def linear_ln_ref(a, w, bias, residual=None, relu=False, a_eps=None, r_ln=None):
    """dh_linear_ln in fp64.  ``a_eps`` given: the A rows are pre-LayerNorm and ``w`` / ``bias`` are the FOLDED weight (16 bit,
    as passed to the kernel) and bias: ((a - mu) * rstd) @ w.T + bias.  ``r_ln = (eps, gamma, beta)``: the residual rows are
    pre-LayerNorm: + (res - mu) * rstd * gamma + beta."""
    x = row_norm(a, a_eps) if a_eps is not None else a.double()
    y = x @ w.double().t() + bias.double()
    if residual is not None:
        if r_ln is not None:
            eps, gamma, beta = r_ln
            y = y + row_norm(residual, eps) * gamma.double() + beta.double()
        else:
            y = y + residual.double()
    return torch.relu(y) if relu else y


def tile_stats(y):
    """Per (row, 64-column tile) mean and sum of squared deviations from it, fp64: [M, N / 64, 2]."""
    t = y.double().view(y.shape[0], -1, 64)
    mean = t.mean(-1)
    return torch.stack([mean, ((t - mean[..., None]) ** 2).sum(-1)], -1)


# ---- the launchers' choices, restated -------------------------------------------------------------------------------------------
def ring_route(blocks, k):
    """csrc/gemm_bf16.hip launch_gemm_bf16, the 64 x 64 kernels' ring depth ("if (blocks > 1280 || (blocks > 320 && blocks <=
    512) || p.K <= 128)" and the three branches under it; DH_LN_LAUNCH makes the same choice)."""
    if blocks > 1280 or 320 < blocks <= 512 or k <= 128:
        return "r4"
    return "r8" if blocks <= 320 else "r3" if blocks <= 768 else "r2"


def route16(m, n, k, out_f32=False, plain_epilogue=True, ln=False, ldc=0, c_aligned=True):
    """The kernel a 16-bit dh_linear / dh_linear_ln call runs.  ``plain_epilogue``: no scale, residual or relu (a bias is
    plain); ``ldc`` / ``c_aligned``: row stride in elements and 16-byte alignment of the output (fp32 outputs only).
    Mirrors csrc/gemm_bf16.hip: launch_persistent_f32 (its three "return false" lines, tried first by dh_linear_bf16_impl when
    out_f32), then launch_gemm_bf16: "big_tiles >= 192 && p.M >= 96 && p.N >= 96 && !lnx" (128 x 128),
    "p.N <= 64 && p.M >= 256 * 512 && !lnx" (dense: 128 x 64), then the ring choice (ring_route)."""
    big_tiles = cdiv(m, 128) * cdiv(n, 128)
    if (out_f32 and not ln and plain_epilogue and k % 64 == 0 and k >= 128 and ldc % 4 == 0 and c_aligned
            and big_tiles >= 1024):
        return "pers"
    if big_tiles >= 192 and m >= 96 and n >= 96 and not ln:
        return "t128"
    if n <= 64 and m >= 256 * 512 and not ln:
        return "n64"
    return ring_route(cdiv(m, 64) * cdiv(n, 64), k)


def route32(m, n):
    """csrc/gemm.hip dh_linear, fp32: "if (big_tiles >= 192 && M >= 96)" -> linear_f32_kernel<128, 128>, else <64, 64>."""
    return "t128" if cdiv(m, 128) * cdiv(n, 128) >= 192 and m >= 96 else "t64"


def n_fast(m, n, k):
    """csrc/gemm_bf16.hip launch_gemm_bf16, first block: "p.n_fast = w_bytes <= 8.0 * 1024 * 1024 && a_bytes > w_bytes"."""
    return int(2 * n * k <= 8 * 1024 * 1024 and 2 * m * k > 2 * n * k)


def wrapper_ldc(dt, m, n, out_f32):
    """hip.linear without ``out``: fp32 logits of 16-bit operands with n % 4 != 0 and m * n >= 2^24 get rows padded to 64."""
    return roundup(n, 64) if dt != F32 and out_f32 and n % 4 and m * n >= 1 << 24 else n


# ---- operands ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _operands(dt, flavour, m, n, k, lda, ldw, seed):
    """(a_buf [m, lda], w_buf [n, ldw]) in ``dt``, every column drawn (a kernel that read past K would read other numbers)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * m + 131 * n + k + 17 * lda + 3 * ldw)
    if flavour == "int":
        return torch.randint(-3, 4, (m, lda), generator=g).to(dt), torch.randint(-3, 4, (n, ldw), generator=g).to(dt)
    return torch.randn(m, lda, generator=g).to(dt), (torch.randn(n, ldw, generator=g) / k ** 0.5).to(dt)


@functools.lru_cache(maxsize=2)
def _product(dt, flavour, m, n, k, lda, ldw, seed):
    """a @ w.T in fp64.  int flavour: an fp32 product is already exact (|sum| <= 9 K < 2^24) and half the work."""
    a, w = _operands(dt, flavour, m, n, k, lda, ldw, seed)
    if flavour == "int":
        return (a[:, :k].float() @ w[:, :k].float().t()).double()
    return a[:, :k].double() @ w[:, :k].double().t()


FORMS = {                                                     # (bias, scale and shift, residual, relu)
    "bias": (1, 0, 0, 0), "affine": (0, 1, 0, 0), "bias_affine": (1, 1, 0, 0), "residual": (0, 0, 1, 0), "relu": (0, 0, 0, 1),
    "all": (1, 1, 1, 1), "none": (0, 0, 0, 0), "bias_relu": (1, 0, 0, 1), "bias_residual": (1, 0, 1, 0),
}


class LinearCase:
    """One dh_linear call.  ``dt``: the operands' type (fp32: everything fp32; 16 bits: residual in ``dt``, output in ``dt`` or,
    ``out_f32``, fp32).  a = a_buf[:, :k] (lda = k + pad_a), w likewise; out = buf[:m, c_off : c_off + n] of a sentinel-filled
    [m + EXTRA_ROWS, ldc] buffer, residual = res_buf[:, res_off : res_off + n] of a drawn [m, ldres] one.  By default ldc and
    ldres are the next multiple of 8 (fp32 output: 4) plus one more chunk: the kernels' 16-byte paths with sentinel columns
    behind every row.  ``wrapper_out``: no ``out`` is passed, hip.linear allocates it.  Operands are drawn on first use, so
    the route tables can be checked without them; the int flavour's do not depend on ``dt``."""

    def __init__(self, dt, flavour, m, n, k, form="bias", out_f32=False, pad_a=0, pad_w=0, ldc=None, ldres=None, c_off=0,
                 res_off=0, wrapper_out=False, seed=0):
        assert flavour in FLAVOURS and form in FORMS and not (dt == F32 and out_f32)
        self.dt, self.flavour, self.m, self.n, self.k, self.form, self.out_f32 = dt, flavour, m, n, k, form, out_f32
        self.has_bias, self.has_affine, self.has_res, self.relu = (bool(x) for x in FORMS[form])
        self.out_dt = F32 if out_f32 else dt
        chunk = 4 if self.out_dt == F32 else 8
        self.lda, self.ldw = k + pad_a, k + pad_w
        self.c_off, self.res_off, self.wrapper_out, self.seed = c_off, res_off, wrapper_out, seed
        self.ldc = wrapper_ldc(dt, m, n, out_f32) if wrapper_out else ldc if ldc is not None else roundup(c_off + n, chunk) + chunk
        self.ldres = ldres if ldres is not None else roundup(res_off + n, 4 if dt == F32 else 8) + 8
        assert self.ldc >= c_off + n and self.ldres >= res_off + n and not (wrapper_out and c_off)
        self._vec = self._acc = None

    # -- what the launchers see
    @property
    def c_aligned(self):
        return self.c_off * (4 if self.out_dt == F32 else 2) % 16 == 0

    @property
    def plain_epilogue(self):
        return not (self.has_affine or self.has_res or self.relu)

    @property
    def route(self):
        if self.dt == F32:
            return route32(self.m, self.n)
        return route16(self.m, self.n, self.k, self.out_f32, self.plain_epilogue, False, self.ldc, self.c_aligned)

    @property
    def blocks(self):
        return cdiv(self.m, 64) * cdiv(self.n, 64)

    @property
    def slab(self):
        return 32 if self.dt == F32 else 64                   # BK of linear_f32_kernel / gemm_bf16_kernel

    def what(self):
        return dict(m=self.m, n=self.n, k=self.k, fl=self.flavour, form=self.form, out="f32" if self.out_dt == F32 else "16",
                    ld=(self.lda, self.ldw, self.ldc, self.ldres), off=(self.c_off, self.res_off))

    # -- operands
    @property
    def _key(self):
        return (F32 if self.flavour == "int" else self.dt, self.flavour, self.m, self.n, self.k, self.lda, self.ldw, self.seed)

    @property
    def a_buf(self):
        return _operands(*self._key)[0].to(self.dt)

    @property
    def w_buf(self):
        return _operands(*self._key)[1].to(self.dt)

    @property
    def a(self):
        return self.a_buf[:, :self.k]

    @property
    def w(self):
        return self.w_buf[:, :self.k]

    def _vectors(self):
        if self._vec is None:
            n, m = self.n, self.m
            g = torch.Generator().manual_seed(104729 * self.seed + 31 * m + 7 * n + self.k + 1)
            if self.flavour == "int":
                ints = lambda *shape: torch.randint(-8, 9, shape, generator=g).float()    # noqa: E731
                bias, shift, res = ints(n), ints(n), ints(m, self.ldres)
                scale = 2.0 ** torch.randint(-1, 2, (n,), generator=g).float()
            else:
                bias, shift = 0.1 * torch.randn(n, generator=g), 0.3 * torch.randn(n, generator=g)
                res, scale = torch.randn(m, self.ldres, generator=g), torch.rand(n, generator=g) + 0.5
            self._vec = dict(bias=bias if self.has_bias else None, scale=scale if self.has_affine else None,
                             shift=shift if self.has_affine else None, res_buf=res.to(self.dt) if self.has_res else None)
        return self._vec

    bias = property(lambda self: self._vectors()["bias"])
    scale = property(lambda self: self._vectors()["scale"])
    shift = property(lambda self: self._vectors()["shift"])
    res_buf = property(lambda self: self._vectors()["res_buf"])

    @property
    def residual(self):
        return None if self.res_buf is None else self.res_buf[:, self.res_off:self.res_off + self.n]

    # -- expected
    def acc(self):
        if self._acc is None:
            self._acc = _product(*self._key)
        return self._acc

    def want(self, drop=None):
        """fp64 [m, n].  ``drop = (k0, k1)``: those operand columns are zero (the sensitivity condition)."""
        acc = self.acc()
        if drop is not None:
            k0, k1 = drop
            acc = acc - self.a[:, k0:k1].double() @ self.w[:, k0:k1].double().t()
        return epilogue_ref(acc, self.bias, self.scale, self.shift, self.residual, self.relu)

    def want_out(self):
        """int flavour: the exact result in the output's type (one rounding for 16 bits)."""
        assert self.flavour == "int"
        return self.want().to(self.out_dt)

    def slabs(self):
        """The K ranges the kernel stages one after the other, the tail chunk last."""
        return [(k0, min(k0 + self.slab, self.k)) for k0 in range(0, self.k, self.slab)]


# ---- the cases of test_linear_routes_gpu.py -----------------------------------------------------------------------------------
# 1. ring switches: (m, n, k) and the (workgroups, route) each must give; the last row tile is partial in every one
RING_SWITCH = (
    ((10233, 70, 192), (320, "r8")), ((6841, 182, 256), (321, "r4")), ((16377, 70, 192), (512, "r4")),
    ((1721, 1213, 256), (513, "r3")), ((24569, 70, 192), (768, "r3")), ((57, 49211, 256), (769, "r2")),
    ((65, 40955, 192), (1280, "r2")), ((57, 81979, 192), (1281, "r4")), ((10233, 70, 128), (320, "r4")),   # the last: K <= 128
)


def ring_switch_cases(dt, fl):
    for (m, n, k), _ in RING_SWITCH:
        yield LinearCase(dt, fl, m, n, k)


# 2. slabs against ring depth: one shape per route (by workgroup count), nslab = ceil(K / 64)
SLAB_SHAPES = {"r8": (70, 70), "r4": (6841, 182), "r3": (1721, 1213), "r2": (25593, 70)}     # 4 / 321 / 513 / 800 workgroups


def slab_counts(route):
    ns = NS[route]
    counts = {ns - 2, ns - 1, ns, ns + 1, 2 * ns + 1} | ({1, 2} if route == "r4" else {3} if route == "r8" else set())
    return sorted(c for c in counts if c >= (1 if route == "r4" else 3))      # K <= 128 is always r4


def slab_cases(dt, fl):
    for route, (m, n) in SLAB_SHAPES.items():
        for nslab in slab_counts(route):
            yield LinearCase(dt, fl, m, n, 64 * nslab)                                     # the pointer-stepping loader
            yield LinearCase(dt, fl, m, n, 64 * (nslab - 1) + (8 if nslab % 2 else 56))    # the K-tail loader


# 3. big tiles: 192 of them exactly (24 x 8: n_fast = 1, 8 x 24: n_fast = 0), and one step below on each condition
BIG_TILES = ((3067, 1021), (1019, 3069))
BIG_TILE_K = (64, 128, 520)
BELOW_BIG = ((128, 24445, 520), (95, 24573, 64), (24573, 95, 128), (24573, 95, 520))      # 191 tiles; M = 95; N = 95 (twice)


def big_tile_cases(dt, fl):
    for m, n in BIG_TILES:
        for k in BIG_TILE_K:
            yield LinearCase(dt, fl, m, n, k)
    for m, n, k in BELOW_BIG:
        yield LinearCase(dt, fl, m, n, k)


# 4. narrow outputs with very many rows
def narrow_cases(dt, fl):
    for n in (40, 64):
        for m in (131072, 131071):
            yield LinearCase(dt, fl, m, n, 64)


# 5. fp32 output through the persistent kernel, and every condition that keeps a call off it
PERS = (4096, 4097, 128)


def persistent_cases(dt, fl):
    m, n, k = PERS
    yield LinearCase(dt, fl, m, n, k, out_f32=True, wrapper_out=True)                     # rows padded to 4160 by hip.linear
    yield LinearCase(dt, fl, m, n, k, out_f32=True, ldc=4160)                             # the same with sentinels around it
    yield LinearCase(dt, fl, m, n, k, "none", out_f32=True, ldc=4160)                     # bias = None
    yield LinearCase(dt, fl, m, n, k, out_f32=True, ldc=n)                                # ldc % 4 != 0: t128, scalar stores
    yield LinearCase(dt, fl, m, n, k, "bias_relu", out_f32=True, ldc=4160)                # t128, 16-byte stores
    yield LinearCase(dt, fl, m, n, k, "bias_residual", out_f32=True, ldc=4160)            # t128, scalar stores
    yield LinearCase(dt, fl, 31 * 128 - 5, n, k, out_f32=True, ldc=4160)                  # 31 x 33 = 1023 tiles: t128


# 6. shape edges
EDGE_M = (1, 63, 64, 65, 130)
EDGE_N = (8, 60, 64, 68, 130, 4567)                           # 68: a partial last chunk in a 16-byte call; 130: scalar bias loads
EDGE_K = (8, 56, 64, 72, 136)
EDGE_K32 = (4, 28, 32, 36, 68)


def edge_cases(dt, fl):
    for m in EDGE_M:
        for n in EDGE_N:
            for k in (EDGE_K32 if dt == F32 else EDGE_K):
                yield LinearCase(dt, fl, m, n, k, pad_a=8, pad_w=16)


# 7. epilogue forms and strides
FORM_NAMES = ("bias", "affine", "bias_affine", "residual", "relu", "all")
FORM_SHAPES = ((65, 68, 136), (130, 130, 72), (63, 60, 64))
FORM_SHAPES32 = ((65, 68, 68), (130, 130, 36), (63, 60, 32))
ODD_LD = ((0, 0), (3, 0), (0, 5))                             # added to the default (16-byte) ldc / ldres
FORM_SEED = 1                                                 # (seed 0: one 2 x 2 corner tile does not see the fp32 K tail under relu)


def form_cases(dt, fl):
    for m, n, k in (FORM_SHAPES32 if dt == F32 else FORM_SHAPES):
        for form in FORM_NAMES:
            for out_f32 in ((False,) if dt == F32 else (False, True)):
                for dc, dr in ODD_LD:
                    d = LinearCase(dt, fl, m, n, k, form, out_f32)
                    yield LinearCase(dt, fl, m, n, k, form, out_f32, pad_a=8, pad_w=16, ldc=d.ldc + dc, ldres=d.ldres + dr, seed=FORM_SEED)


# 8. base alignment: out / residual start 4 elements (8 bytes) into rows that are multiples of 8 elements
ALIGN_SHAPES = ((65, 40, 72), (130, 130, 136), (200, 264, 64))
ALIGN_OFFS = ((4, 0), (0, 4), (4, 4))


def align_cases(dt, fl):
    for m, n, k in ALIGN_SHAPES:
        for form in ("bias", "residual", "all"):
            for c_off, res_off in ALIGN_OFFS:
                yield LinearCase(dt, fl, m, n, k, form, pad_a=8, c_off=c_off, res_off=res_off)
    yield LinearCase(dt, fl, 3067, 1021, 64, "all", c_off=4, res_off=4)                    # the 128 x 128 kernel's epilogue


# 9. fp32: big tiles (N < 96 does not keep an fp32 call off the 128 x 128 kernel), edges, forms
BIG_TILES32 = ((3067, 1021, 32), (3067, 1021, 68), (1019, 3069, 36), (24573, 95, 4), (128, 24445, 28), (95, 24573, 32))


def f32_big_tile_cases(fl):
    for m, n, k in BIG_TILES32:
        yield LinearCase(F32, fl, m, n, k)


CASE_SETS = {                                                 # name: (cases(dt, fl), the routes the 16-bit types must reach)
    "ring_switch": (ring_switch_cases, {"r8", "r4", "r3", "r2"}),
    "slabs": (slab_cases, {"r8", "r4", "r3", "r2"}),
    "big_tiles": (big_tile_cases, {"t128", "r3", "r4"}),
    "narrow": (narrow_cases, {"n64", "r4"}),
    "persistent": (persistent_cases, {"pers", "t128"}),
    "edges": (edge_cases, {"r4", "r8"}),
    "forms": (form_cases, {"r4", "r8"}),
    "align": (align_cases, {"r4", "r8", "t128"}),
}
CASE_SETS32 = {                                               # fp32: name: (cases(fl), routes)
    "big_tiles": (f32_big_tile_cases, {"t128", "t64"}),
    "edges": (lambda fl: edge_cases(F32, fl), {"t64"}),
    "forms": (lambda fl: form_cases(F32, fl), {"t64"}),
}


# ---- 10. deferred LayerNorm (dh_linear_ln) ------------------------------------------------------------------------------------
LN_EPS = 1e-5
# EXT 1 (A-side fold): (m, n, k) -> (workgroups, route); a_tiles = k / 64 in {2, 4, 6, 8}, the last row tile partial
LN_A_SHAPES = (
    ((37, 512, 512), (8, "r8")), ((1273, 1536, 512), (480, "r4")), ((1273, 2048, 256), (640, "r3")),
    ((1913, 2048, 384), (960, "r2")), ((2617, 2048, 512), (1312, "r4")), ((1913, 512, 128), (240, "r4")),   # the last: K <= 128
)
# EXT 3 (residual LayerNorm / output statistics)
LN_R_SHAPES = (
    ((37, 512, 256), (8, "r8")), ((3193, 512, 256), (400, "r4")), ((5753, 512, 192), (720, "r3")),
    ((9593, 512, 256), (1200, "r2")), ((10297, 512, 256), (1288, "r4")), ((1273, 128, 128), (40, "r4")), ((130, 128, 256), (6, "r8")),
)
LN_A_FORMS = ((None, False), (None, True), ("plain", False))                                # (residual, relu)
LN_R_FORMS = tuple((res, stats, relu) for res, stats in (("ln", False), ("ln", True), ("plain", True), (None, True)) for relu in (False, True))


class LnCase:
    """One shape of dh_linear_ln, real flavour.  ``y`` [m, k] (EXT 1) / [m, n] (EXT 3) are pre-LayerNorm rows with the existing
    test's distribution (randn * 1.7 + 0.3); their statistics go to the kernel as fp32 per-tile partials (tile_stats)."""

    def __init__(self, dt, ext, m, n, k):
        assert ext in (1, 3)
        self.dt, self.ext, self.m, self.n, self.k = dt, ext, m, n, k
        self.ldc = n + 8
        g = torch.Generator().manual_seed(7919 * m + 31 * n + k + ext)
        d = k if ext == 1 else n
        self.y = (torch.randn(m, d, generator=g) * 1.7 + 0.3).to(dt)
        self.gamma, self.beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2
        w, self.b = (torch.randn(n, k, generator=g) / k ** 0.5).to(dt), torch.randn(n, generator=g) * 0.1
        self.stats = tile_stats(self.y).float()
        if ext == 1:                                          # gamma into the weight (rounded: what the kernel is given), beta into the bias
            self.w_plain = w
            self.w = (w.double() * self.gamma.double()[None, :]).to(dt)
            self.bias = (self.b.double() + w.double() @ self.beta.double()).float()
            self.colsum = self.w.double().sum(1).float()
            self.a = self.y
        else:
            self.w, self.bias = w, self.b
            self.a = torch.randn(m, k, generator=g).to(dt)
        self.res = self.y if ext == 3 else torch.randn(m, n, generator=g).to(dt)      # EXT 1: a plain residual
        self._acc = None

    @property
    def blocks(self):
        return cdiv(self.m, 64) * cdiv(self.n, 64)

    @property
    def route(self):
        return route16(self.m, self.n, self.k, ln=True)

    def what(self):
        return dict(ext=self.ext, m=self.m, n=self.n, k=self.k)

    def want(self, res=None, relu=False):
        """``res``: None, "plain" (the residual rows as they are) or, EXT 3, "ln" (the residual rows are pre-LayerNorm)."""
        if self._acc is None:
            self._acc = linear_ln_ref(self.a, self.w, self.bias, a_eps=LN_EPS if self.ext == 1 else None)
        y = self._acc
        if res == "ln":
            assert self.ext == 3
            y = y + row_norm(self.res, LN_EPS) * self.gamma.double() + self.beta.double()
        elif res == "plain":
            y = y + self.res.double()
        return torch.relu(y) if relu else y


def ln_a_cases(dt):
    for (m, n, k), _ in LN_A_SHAPES:
        yield LnCase(dt, 1, m, n, k)


def ln_r_cases(dt):
    for (m, n, k), _ in LN_R_SHAPES:
        yield LnCase(dt, 3, m, n, k)


# ---- gates ------------------------------------------------------------------------------------------------------------------
class RouteGates:
    """One test's gates, one per route it reaches: ``Gate`` (ulps) for 16-bit outputs, ``AbsGate`` for fp32 outputs.  ``dt`` is
    the operands' type, the tables' second key.  ``check`` prints every route's worst error, then asserts them all."""

    def __init__(self, dt, ulp_table, abs_table, prefix=""):
        self.dt, self.ulp_table, self.abs_table, self.prefix, self.gates = dt, ulp_table, abs_table, prefix, {}

    def add(self, route, got, want, what, out_f32=False):
        f32 = out_f32 or self.dt == F32
        key = (self.prefix + route, f32)
        if key not in self.gates:
            self.gates[key] = AbsGate(key[0], self.dt, self.abs_table, "f32 out") if f32 else Gate(key[0], self.dt, self.ulp_table)
        self.gates[key].add(got, want, what)

    def check(self):
        failed = []
        for g in self.gates.values():
            try:
                g.check()
            except AssertionError as e:
                failed.append(e)
        assert not failed, failed
