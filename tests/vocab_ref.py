"""What the vocabulary-classifier tests share (test_vocab_routes_gpu.py, test_vocab_ref_cpu.py): dh_vocab_logits,
dh_vocab_logits_wreg and dh_vocab_logprob stated plainly in fp64, the restated choices of their launchers, and the cases of
every kernel route, option, K, shape edge and stride with their operands and expected results.  Plain module, no GPU use: the
cases are built on the CPU.

Every case set comes in the two operand flavours of linear_ref.  "int": operand entries are integers in [-3, 3] and the bias
holds integers in [-8, 8], so every product and every partial sum is an integer below 2^24 -- exact in fp32 in ANY accumulation
order: compared with torch.equal.  "real": randn operands with w / sqrt(K) and a bias of order 1, compared with fp64 by absolute
error.  Operands are drawn on first use, so the tables can be checked without them."""
import functools

import torch

from attn_ref import BF16, F16, F32, F32_ATOL  # noqa: F401  (re-exported for the two test modules)
from linear_ref import DT16, DT16_IDS, EXTRA_ROWS, FLAVOURS, SENTINEL, AbsGate, RouteGates, cdiv, roundup  # noqa: F401

GROUP = 64                                                    # columns per group maximum (hip.GROUP_COLS)
GM_SPARE = 3                                                  # sentinel columns behind the group maxima every entry point defines
LOGP_ATOL = 2e-4                                              # the bar test_vocab_logprob_matches_log_softmax (test_bf16_gpu.py) sets
NEG_INF = float("-inf")


def n_groups(v):
    """hip.n_groups: whole 128-column panels of 64-column groups."""
    return 2 * cdiv(v, 128)


# ---- the references -----------------------------------------------------------------------------------------------------------
def logits_ref(a, w, bias=None):
    """a @ w.T + bias in fp64, on the operands as the kernel sees them."""
    y = a.double() @ w.double().t()
    return y if bias is None else y + bias.double()


def group_max_ref(logits, groups=None):
    """[M, groups] maxima over the REAL columns (< V = logits.shape[1]) of each 64-column group; a group that starts past V is
    -inf (csrc/beam.hip: "CONVENTION: the maximum runs over the group's REAL columns (< V) only").  ``groups`` defaults to the
    groups that hold a real column."""
    m, v = logits.shape
    groups = cdiv(v, GROUP) if groups is None else groups
    assert groups * GROUP >= v
    padded = torch.full((m, groups * GROUP), NEG_INF, dtype=logits.dtype)
    padded[:, :v] = logits
    return padded.view(m, groups, GROUP).max(-1).values


def logprob_ref(logits, targets):
    """log_softmax(logits)[target] in fp64; a target outside [0, V) gives 0."""
    m, v = logits.shape
    ok = (targets >= 0) & (targets < v)
    lp = torch.log_softmax(logits.double(), -1)[torch.arange(m), targets.clamp(0, v - 1)]
    return torch.where(ok, lp, torch.zeros_like(lp))


# ---- the launchers' choices, restated ------------------------------------------------------------------------------------------
def areg256_plan(m, v, ldl=None):
    """The row tiles per vocab_areg256_kernel launch, or None when the plan is abandoned.  csrc/gemm_bf16.hip dh_vocab_logits:
    "M >= 512 && (M % 256) == 0 && ldl >= tn128 * 128", then
    "auto fits = [&](int t) { return t >= 1 && t <= 32 && (32 / t) * t >= 28 && tn128 >= 8 * (32 / t); }" and the loop
    "int t = left < 32 ? left : 32; while (t > 0 && !(fits(t) && (left - t == 0 || left - t >= 2))) --t; if (t == 0) break;"
    (at most 64 launches; "if (left == 0)" runs the plan).  ``ldl`` defaults to whole panels."""
    tn128 = cdiv(v, 128)
    ldl = tn128 * 128 if ldl is None else ldl
    if not (m >= 512 and m % 256 == 0 and ldl >= tn128 * 128):
        return None
    fits = lambda t: 1 <= t <= 32 and (32 // t) * t >= 28 and tn128 >= 8 * (32 // t)    # noqa: E731
    plan, left = [], m // 256
    while left > 0 and len(plan) < 64:
        t = min(left, 32)
        while t > 0 and not (fits(t) and (left - t == 0 or left - t >= 2)):
            t -= 1
        if t == 0:
            break
        plan.append(t)
        left -= t
    return plan if left == 0 else None


def route(m, v, k, logits=True, ldl=0, aligned=True, vocab_areg=1):
    """The kernel a dh_vocab_logits call runs (csrc/gemm_bf16.hip).  ``logits``: a logits buffer is passed, ``ldl`` its row
    stride and ``aligned`` its base's 16-byte alignment; ``vocab_areg``: the option's value.
      "if ((!logits || ((ldl % 4) == 0 && ((uintptr_t)logits % 16) == 0)) && K >= 128 && (K % 64) == 0)", else gemm_bf16_kernel
      "if (areg && areg != 128 && logits && K == 512 && M >= 512 && (M % 256) == 0 && ldl >= tn128 * 128)" and a plan that
        reaches "left == 0": vocab_areg256_kernel
      "if (areg && logits && K == 512 && tm128 <= 32 && (32 / tm128) * tm128 >= 28 && tn128 >= 8 * (32 / tm128))": vocab_areg_kernel
      "if (!logits && M >= 512)": vocab256_kernel, else vocab_logits_kernel"""
    if not ((not logits or (ldl % 4 == 0 and aligned)) and k >= 128 and k % 64 == 0):
        return "tile"
    tm128, tn128 = cdiv(m, 128), cdiv(v, 128)
    if vocab_areg and vocab_areg != 128 and logits and k == 512 and areg256_plan(m, v, ldl) is not None:
        return "a256"
    if vocab_areg and logits and k == 512 and tm128 <= 32 and (32 // tm128) * tm128 >= 28 and tn128 >= 8 * (32 // tm128):
        return "a128"
    return "g256" if not logits and m >= 512 else "pers"


def wreg_supported(m, v, k, ldl, gm_ld):
    """csrc/vocab_wreg.hip dh_vocab_logits_wreg_supported (``ldl`` = 0: no logits): "if (K != 512 || M <= 0 || V <= 0) return 0",
    "pow2_blocks = (M % 80) == 0 && (nrb == 1 || ... || nrb == 32)" and "(pow2_blocks || M <= 640) && (ldl == 0 || (ldl >= vpad &&
    (ldl % 4) == 0)) && gm_ld >= vpad / 64"."""
    if k != 512 or m <= 0 or v <= 0:
        return False
    nrb, vpad = cdiv(m, 80), roundup(v, 256)
    pow2_blocks = m % 80 == 0 and nrb in (1, 2, 4, 8, 16, 32)
    return (pow2_blocks or m <= 640) and (ldl == 0 or (ldl >= vpad and ldl % 4 == 0)) and gm_ld >= vpad // 64


def logprob_route(m):
    """csrc/gemm_bf16.hip dh_vocab_logprob: "if (M >= 512)" vocab256_kernel<T, true>, else vocab_logits_kernel<..., true>."""
    return "lse256" if m >= 512 else "lse128"


# ---- operands -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _operands(dt, flavour, m, v, k, lda, ldw, seed):
    """(a_buf [m, lda], w_buf [v, ldw]) in ``dt``, every column drawn (a kernel that read past K would read other numbers)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * m + 131 * v + k + 17 * lda + 3 * ldw + 5)
    if flavour == "int":
        return torch.randint(-3, 4, (m, lda), generator=g).to(dt), torch.randint(-3, 4, (v, ldw), generator=g).to(dt)
    return torch.randn(m, lda, generator=g).to(dt), (torch.randn(v, ldw, generator=g) / k ** 0.5).to(dt)


@functools.lru_cache(maxsize=3)
def _product(dt, flavour, m, v, k, lda, ldw, seed):
    """a @ w.T in fp64, computed once per operand pair.  int flavour: an fp32 product is already exact (|sum| <= 9 K < 2^24)."""
    a, w = _operands(dt, flavour, m, v, k, lda, ldw, seed)
    if flavour == "int":
        return (a[:, :k].float() @ w[:, :k].float().t()).double()
    return a[:, :k].double() @ w[:, :k].double().t()


class VocabCase:
    """One dh_vocab_logits (``entry`` "logits") or dh_vocab_logits_wreg ("wreg") call.  a = a_buf[:, :k] (lda = k + pad_a), w
    likewise.  The logits are the view [:m, l_off : l_off + v] of a sentinel-filled [m + EXTRA_ROWS, ldl] buffer (``logits``
    False: group maxima only); by default ldl is V rounded up to 256 columns plus 8 -- wider than any route needs, rows of
    16 bytes.  The group maxima are the view [:m, :groups] of a sentinel-filled [m + EXTRA_ROWS, groups + GM_SPARE] one.
    ``areg``: the value of option "vocab_areg" during the call."""

    def __init__(self, dt, flavour, m, v, k=512, bias=True, logits=True, pad_a=0, pad_w=0, ldl=None, l_off=0, areg=1,
                 entry="logits", seed=0):
        assert flavour in FLAVOURS and entry in ("logits", "wreg") and 9 * k + 8 < 2 ** 24
        self.dt, self.flavour, self.m, self.v, self.k, self.has_bias, self.logits = dt, flavour, m, v, k, bias, logits
        self.lda, self.ldw, self.l_off, self.areg, self.entry, self.seed = k + pad_a, k + pad_w, l_off, areg, entry, seed
        self.ldl = (roundup(v, 256) + 8 if ldl is None else ldl) if logits else 0
        assert not logits or self.ldl >= l_off + v
        assert entry == "logits" or (l_off == 0 and pad_w == 0 and areg == 1)
        self._bias = None

    # -- what the launchers see
    @property
    def aligned(self):
        return self.l_off * 4 % 16 == 0

    @property
    def route(self):
        if self.entry == "wreg":
            return "wreg"
        return route(self.m, self.v, self.k, self.logits, self.ldl, self.aligned, self.areg)

    @property
    def groups(self):
        """Group maxima the entry point defines per row: the real groups, then -inf up to here."""
        return roundup(self.v, 256) // GROUP if self.entry == "wreg" else n_groups(self.v)

    @property
    def real_groups(self):
        return cdiv(self.v, GROUP)

    @property
    def pad_to(self):
        """The route witness: logits columns [v, pad_to) hold copies of logit[v - 1]; every other route stops at v.
        vocab_areg.h: "the padding columns hold copies of logit[V - 1]" (whole 128-column panels); vocab_wreg.hip: "weight rows /
        bias entries past V are copies of row V - 1" (whole 256-column chunks)."""
        return roundup(self.v, {"a256": 128, "wreg": 256}.get(self.route, 1))

    def what(self):
        return dict(entry=self.entry, m=self.m, v=self.v, k=self.k, fl=self.flavour, bias=self.has_bias, logits=self.logits,
                    ld=(self.lda, self.ldw, self.ldl), l_off=self.l_off, areg=self.areg)

    # -- operands
    @property
    def _key(self):
        return (F32 if self.flavour == "int" else self.dt, self.flavour, self.m, self.v, self.k, self.lda, self.ldw, self.seed)

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

    @property
    def bias(self):
        if not self.has_bias:
            return None
        if self._bias is None:
            g = torch.Generator().manual_seed(104729 * self.seed + 7 * self.v + self.k + 1)
            self._bias = (torch.randint(-8, 9, (self.v,), generator=g).float() if self.flavour == "int"
                          else torch.randn(self.v, generator=g))
        return self._bias

    # -- expected
    def want(self, drop=None):
        """fp64 [m, v].  ``drop = (k0, k1)``: those operand columns are zero (the sensitivity condition)."""
        acc = _product(*self._key)
        if drop is not None:
            k0, k1 = drop
            if self.flavour == "int":
                acc = acc - (self.a[:, k0:k1].float() @ self.w[:, k0:k1].float().t()).double()
            else:
                acc = acc - self.a[:, k0:k1].double() @ self.w[:, k0:k1].double().t()
        return acc if self.bias is None else acc + self.bias.double()

    def slabs(self):
        """The 64-deep K ranges every classifier kernel stages one after the other, the tail chunk last."""
        return [(k0, min(k0 + 64, self.k)) for k0 in range(0, self.k, 64)]


# ---- the cases of test_vocab_routes_gpu.py -------------------------------------------------------------------------------------
# 1. vocab_areg256_kernel in one launch: (m, v) -> the plan
A256_SINGLE = (
    ((2048, 4000), [8]),      # V ends inside group 62, the last panel's second group starts past V
    ((4096, 1921), [16]),     # 16 row tiles on the fewest panels that take them (16); one real column in the last panel
    ((1280, 8192), [5]),      # V an exact multiple of 128: no padding column
    ((512, 16300), [2]),      # the two-tile launch: 128 panels
)
# 2. ... in several launches
A256_MULTI = (((6656, 3000), [16, 10]), ((2816, 10150), [8, 3]))


def a256_single_cases(dt, fl):
    for (m, v), _ in A256_SINGLE:
        yield VocabCase(dt, fl, m, v)


def a256_multi_cases(dt, fl):
    for (m, v), _ in A256_MULTI:
        yield VocabCase(dt, fl, m, v)


# 3. row counts and strides that abandon the plan
LDL_64 = (1280, 8100, 8128)                                   # (m, v, ldl): rows of whole groups, not whole panels (8192)
ABANDONED = (((512, 5000), "pers"), ((2048, 3968), "a128"), ((3072, 10150), "pers"))


def abandoned_cases(dt, fl):
    for (m, v), _ in ABANDONED:
        yield VocabCase(dt, fl, m, v)
    m, v, ldl = LDL_64
    yield VocabCase(dt, fl, m, v, ldl=ldl)


# 4. vocab_areg_kernel: a partial last row tile on one / three row tiles (256 panels: V = 36541 is the smallest the project has),
#    16 full row tiles on 31 panels, with and without bias; option vocab_areg = 128 at shapes of the 256-row kernel
def a128_cases(dt, fl):
    yield VocabCase(dt, fl, 37, 36541)
    yield VocabCase(dt, fl, 300, 36541, bias=False)
    yield VocabCase(dt, fl, 2048, 3968)
    yield VocabCase(dt, fl, 2048, 3968, bias=False)


# 4b. option vocab_areg = 128 at shapes of the 256-row kernel
def areg128_cases(dt, fl):
    for (m, v), _ in A256_SINGLE:
        yield VocabCase(dt, fl, m, v, areg=128)
    yield VocabCase(dt, fl, 6656, 3000, areg=128)             # 52 row tiles of 128: the tile kernel


# 5. vocab_logits_kernel: option vocab_areg = 0 at K = 512; K = 128 (two slabs in a ring of two) / 192 / 256 / 1024 at default
#    options; 16 tiles (one per workgroup) and 858 (> 512 workgroups: interior -> edge -> interior walks); group maxima only
PERS_K = (128, 192, 256, 1024)


def pers_cases(dt, fl):
    yield VocabCase(dt, fl, 300, 36541, areg=0)
    yield VocabCase(dt, fl, 130, 1000, areg=0)
    yield VocabCase(dt, fl, 1280, 8192, areg=0)               # interior tiles only: every wait leaves the previous tile's stores outstanding
    for k in PERS_K:
        yield VocabCase(dt, fl, 130, 1000, k)
    yield VocabCase(dt, fl, 300, 36541, 128)
    yield VocabCase(dt, fl, 300, 36541, 192, bias=False)
    yield VocabCase(dt, fl, 300, 4100, logits=False)
    yield VocabCase(dt, fl, 130, 1000, 256, logits=False)
    yield VocabCase(dt, fl, 511, 4100, 128, bias=False, logits=False)


# 6. vocab256_kernel, group maxima only: V ends in a 256-column tile's first half / second half / on a multiple of 256
def g256_cases(dt, fl):
    yield VocabCase(dt, fl, 512, 1100, logits=False)
    yield VocabCase(dt, fl, 600, 4000, logits=False)
    yield VocabCase(dt, fl, 1280, 2048, logits=False)
    yield VocabCase(dt, fl, 600, 1100, 192, bias=False, logits=False)
    yield VocabCase(dt, fl, 512, 4000, 128, logits=False)


# 7. gemm_bf16_kernel<128, 128> with the group-maxima epilogue: K < 128 or a K tail; logits rows or base off 16 bytes
TILE_K = (64, 72, 136, 520)


def tile_cases(dt, fl):
    for k in TILE_K:
        yield VocabCase(dt, fl, 130, 1000, k)
    yield VocabCase(dt, fl, 300, 4100, 72, bias=False)
    yield VocabCase(dt, fl, 130, 1000, ldl=1003)
    yield VocabCase(dt, fl, 512, 5000, ldl=5130)
    yield VocabCase(dt, fl, 130, 1000, ldl=1264, l_off=2)     # the view starts 8 bytes into 16-byte rows


# 8. lda = K + 8, ldw = K + 16
def stride_cases(dt, fl):
    pads = dict(pad_a=8, pad_w=16)
    yield VocabCase(dt, fl, 2048, 4000, **pads)
    yield VocabCase(dt, fl, 2048, 3968, **pads)
    yield VocabCase(dt, fl, 300, 4100, areg=0, **pads)
    yield VocabCase(dt, fl, 130, 1000, 256, **pads)
    yield VocabCase(dt, fl, 130, 1000, 72, **pads)
    yield VocabCase(dt, fl, 600, 1100, logits=False, **pads)


# 9. dh_vocab_logits_wreg: 1 / 1 / 2 / 5 / 8 / 16 row blocks of 80; V ends inside a group (1000), inside a chunk on a group
#    boundary (1088 = 17 x 64) and on a chunk boundary (2048)
def wreg_cases(dt, fl):
    w = dict(entry="wreg")
    yield VocabCase(dt, fl, 5, 1000, bias=False, **w)
    yield VocabCase(dt, fl, 80, 1088, **w)
    yield VocabCase(dt, fl, 81, 2048, **w)
    yield VocabCase(dt, fl, 81, 1000, pad_a=8, **w)
    yield VocabCase(dt, fl, 380, 1000, logits=False, **w)
    yield VocabCase(dt, fl, 380, 1088, bias=False, logits=False, **w)
    yield VocabCase(dt, fl, 640, 1088, bias=False, **w)
    yield VocabCase(dt, fl, 1280, 1000, **w)
    yield VocabCase(dt, fl, 1280, 2048, pad_a=8, **w)


CASE_SETS = {                                                 # name: (cases(dt, fl), the routes they must reach)
    "a256_single": (a256_single_cases, {"a256"}),
    "a256_multi": (a256_multi_cases, {"a256"}),
    "abandoned": (abandoned_cases, {"pers", "a128"}),
    "a128": (a128_cases, {"a128"}),
    "areg128": (areg128_cases, {"a128", "pers"}),
    "pers": (pers_cases, {"pers"}),
    "g256": (g256_cases, {"g256"}),
    "tile": (tile_cases, {"tile"}),
    "strides": (stride_cases, {"a256", "a128", "pers", "tile", "g256"}),
    "wreg": (wreg_cases, {"wreg"}),
}

# 10. row-sliced calls, the way classifier_groups (csrc/runtime.hip) splits a row count that is no multiple of 256: "head = rows / 256
#     * 256", one call on [:head], one on [head:]
SLICED = (1100, 8192, 1024)                                   # (rows, v, head)
SLICED_ROUTES = {"a256", "pers"}


def sliced_parts(dt, fl):
    """The whole buffer as one case (operands, reference) and the (row0, rows) of the two calls."""
    m, v, head = SLICED
    return VocabCase(dt, fl, m, v), ((0, head), (head, m - head))


# 11. dh_vocab_logits_wreg_supported around each threshold
def wreg_grid():
    for m in (0, 1, 79, 80, 81, 160, 240, 320, 400, 639, 640, 641, 720, 1280, 1281, 1360, 2560, 2640, 5120):
        for k in (256, 512, 576):
            for v in (1, 1000, 1024, 1025):
                vpad = roundup(v, 256)
                for ldl in (0, vpad - 4, vpad, vpad + 2, vpad + 4):
                    for gm_ld in (vpad // 64 - 1, vpad // 64, vpad // 64 + 3):
                        yield m, v, k, ldl, gm_ld


# ---- 12. dh_vocab_logprob ---------------------------------------------------------------------------------------------------------
SPIKE = 60.0                                                  # the spiked column's logit stands about this far above the rest


class LogprobCase:
    """One dh_vocab_logprob call, real flavour.  Targets: row 0 -> 0, row 1 -> V - 1 (the last real column of the last, partial,
    group), row 2 -> -1 and row 3 -> V (outside: 0), row 4 -> V - 2, the rest random.  ``spike``: column 0 of every A row holds 4
    and weight row V / 2 holds 15 there (finite in fp16), so that one logit per row stands about 60 above the others: every other
    group's sum reaches the result only through its rescale exp(gmax - M), and without the rescale the result is off by log V."""

    def __init__(self, dt, m, v, k, spike=False, seed=0):
        self.dt, self.m, self.v, self.k, self.spike = dt, m, v, k, spike
        g = torch.Generator().manual_seed(15485863 * seed + 7919 * m + 131 * v + k)
        a, w = torch.randn(m, k, generator=g), torch.randn(v, k, generator=g) / k ** 0.5
        if spike:
            a[:, 0], w[v // 2, 0] = 4.0, SPIKE / 4.0
        self.a, self.w, self.bias = a.to(dt), w.to(dt), torch.randn(v, generator=g)
        self.targets = torch.randint(0, v, (m,), generator=g)
        self.targets[:5] = torch.tensor([0, v - 1, -1, v, v - 2])
        if spike:                                             # row 5 alone asks for the spiked column
            self.targets[self.targets == v // 2] = v // 2 + 1
            self.targets[5] = v // 2
        self._want = None

    @property
    def route(self):
        return logprob_route(self.m)

    def what(self):
        return dict(m=self.m, v=self.v, k=self.k, spike=self.spike)

    def logits(self):
        return logits_ref(self.a, self.w, self.bias)

    def want(self):
        if self._want is None:
            self._want = logprob_ref(self.logits(), self.targets)
        return self._want


LOGPROB = (                                                   # (m, v, k): both routes at every K, V = 36541 once
    (37, 1000, 512), (300, 4100, 128), (37, 4100, 1024), (300, 1000, 1024), (300, 36541, 512),
    (512, 1000, 1024), (600, 4100, 512), (512, 4100, 128), (600, 1000, 128),
)
LOGPROB_SPIKE = ((300, 4100, 512), (600, 4100, 512), (600, 1000, 128))


def logprob_cases(dt):
    for m, v, k in LOGPROB:
        yield LogprobCase(dt, m, v, k)


def logprob_spike_cases(dt):
    for m, v, k in LOGPROB_SPIKE:
        yield LogprobCase(dt, m, v, k, spike=True)


class LogpGate(AbsGate):
    """AbsGate for log-probabilities: its table's entries stay under LOGP_ATOL (a log-prob of -60 has an fp32 ulp of 3.8e-6)."""

    def check(self):
        bound = self.table[self.name][self.dt]
        print(f"[{self.name}] {self.dt} {self.kind}: worst {self.worst:.3e} abs at {self.where} ({self.n} cases)")
        assert bound <= LOGP_ATOL, (self.name, self.dt, bound)
        assert self.worst <= bound, (self.name, self.dt, self.kind, self.worst, self.where)
