"""What the attention tests share (test_prefill_gpu.py, test_attn_decode_gpu.py, test_attn_ref_cpu.py): the fp64 statement of the
reference's attention (transformers.py:106-120), the ulp error measure and its ``Gate``, and the decode kernels' test cases
with their vectorised fp64 reference.  Plain module, no GPU use: the cases are built on the CPU."""
import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]
ULP_FLOOR = 2.0 ** -6
F32_ATOL = 2e-5


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 7 * sum(shape)))


def ulp(x, dt):
    """Spacing of ``dt`` at |x| (x fp64), at least the type's smallest subnormal step."""
    mant, sub = {BF16: (7, 2.0 ** -133), F16: (10, 2.0 ** -24)}[dt]
    _, e = torch.frexp(x.abs())
    step = torch.ldexp(torch.ones_like(x), e - 1 - mant).clamp(min=sub)
    return torch.where(x == 0, torch.full_like(x, sub), step)


def ulps(got, want, dt):
    """|got - want| elementwise, in ulps of ``dt`` at max(|want|, 2^-6) (fp64 tensor)."""
    want = want.double()
    return (got.double().cpu() - want).abs() / ulp(want.abs().clamp(min=ULP_FLOOR), dt)


def err_ulps(got, want, dt):
    return float(ulps(got, want, dt).max())


class Gate:
    """Accumulates one test's cases: fp32 cases assert ``atol = 2e-5`` as they come, 16-bit cases record the error in ulps;
    ``check`` asserts the worst against ``table[name][dt]`` and prints it (the numbers behind the ``ULP_GATE`` tables)."""

    def __init__(self, name, dt, table):
        self.name, self.dt, self.table, self.worst, self.where, self.n, self.over = name, dt, table, 0.0, None, 0, []

    def add(self, got, want, what):
        self.n += 1
        if self.dt == F32:
            np.testing.assert_allclose(got.cpu().double().numpy(), want.double().numpy(), atol=F32_ATOL, rtol=0, err_msg=str(what))
            return
        e = err_ulps(got, want, self.dt)
        if e > self.table[self.name][self.dt]:
            self.over.append(what)
        if e > self.worst:
            self.worst, self.where = e, what

    def check(self):
        if self.dt == F32:
            return
        print(f"[{self.name}] {self.dt}: worst {self.worst:.4f} ulp at {self.where} ({self.n} cases)")
        if self.over:
            print(f"[{self.name}] {self.dt}: {len(self.over)} cases over the gate: {self.over}")
        assert self.worst <= self.table[self.name][self.dt], (self.name, self.dt, self.worst, self.where)


def attn_ref(q, k, v, masked, scale, dead=None):
    """q [B, H, Tq, dh], k / v [B, H, Tk, dh], masked bool broadcastable to [B, H, Tq, Tk] -> [B, H, Tq, dh], in fp64.
    ``dead`` (same broadcast) removes keys altogether: no weight, unlike a masked key among masked keys only."""
    energy = torch.einsum("bhtd,bhsd->bhts", q.double(), k.double()) / scale
    if masked is not None:
        energy = energy.masked_fill(masked, -1e8)
    if dead is not None:
        energy = energy.masked_fill(dead, -float("inf"))
    return torch.einsum("bhts,bhsd->bhtd", torch.softmax(energy, -1), v.double())


# ---- decode self-attention (dh_attn_self_decode) ---------------------------------------------------------------------------
SELF_ROUTES = ("self_reg", "self_fast", "self_generic")
CROSS_ROUTES = ("cross_lds", "cross_fast", "cross_generic")
BOUNDARY_T = (0, 1, 15, 16, 39, 40, 55, 56, 57, 100)         # L = t + 1 around 16 | 17, 40 | 41, 56 | 57, and a long one
HEAD_DIM_T = (0, 1, 7, 8, 9, 63, 64, 100)
HEAD_DIMS = ((128, 8), (512, 4), (256, 8), (384, 4))          # (D, H): head dim 16 (generic), 128, 32, 96 (generic)
ROW_BLOCKS = (1, 16, 17, 24, 40, 64)                          # rows per image: 16 waves per workgroup, then blockIdx.z
EXTRA_ROWS = 16                                               # sentinel rows behind ``out``: one workgroup's worth of waves


def self_route(dt, dh, L):
    """The kernel launch_self / launch_fast (csrc/attention.hip) picks."""
    if dh == 64 and L <= (40 if dt == F32 else 56):
        return "self_reg"
    return "self_fast" if dh in (32, 64, 128) else "self_generic"


def cross_route(dh, s):
    if dh == 64 and s <= 64:
        return "cross_lds"
    return "cross_fast" if dh in (32, 64, 128) else "cross_generic"


class SelfCase:
    """One dh_attn_self_decode call.  ``n_img * rows_per_img`` compact rows; compact row rc is logical row rl = rc * row_mult of
    ``rows_total = n_img * rows_per_img * row_mult``.  The cache and the ancestor table are drawn once per shape (``cache``),
    the new rows and the tokens per ``t``: about 20 % of the tokens are <pad>, and on the even compact rows the tokens that
    decide keys t - 1 and t are not, so the top slots of the top iteration carry weight."""

    def __init__(self, dt, n_img, rows_per_img, row_mult, d, n_heads, t, tmax, pad_index, scale, cache=None):
        self.dt, self.n_img, self.rows_per_img, self.row_mult, self.d, self.n_heads = dt, n_img, rows_per_img, row_mult, d, n_heads
        self.t, self.pad_index, self.scale = t, pad_index, scale
        self.rows = n_img * rows_per_img
        self.rows_total = rt = self.rows * row_mult
        self.dh = d // n_heads
        per_img = rows_per_img * row_mult
        if cache is None or "kc" not in cache:
            g = torch.Generator().manual_seed(17 * rt + d + tmax)
            kc = torch.randn(tmax + 1, rt, d, generator=g).to(dt)
            vc = torch.randn(tmax + 1, rt, d, generator=g).to(dt)
            base = torch.arange(rt)[:, None] // per_img * per_img
            # any logical row of the image: a random sibling beam, and a second row block reads ancestors in the first
            src = base + torch.randint(0, per_img, (rt, tmax + 3), generator=g)
            new = dict(kc=kc, vc=vc, src=src.int())           # src row stride tmax + 3
            if cache is None:
                cache = new
            else:
                cache.update(new)
        self.cache = cache
        self.kc, self.vc, self.src = cache["kc"], cache["vc"], cache["src"]
        g = torch.Generator().manual_seed(1000 * t + rt + d)
        self.qkv = torch.randn(self.rows, 3 * d, generator=g).to(dt)
        pad_value = pad_index if pad_index >= 0 else 0
        tok = torch.randint(1, 5, (rt, tmax + 2), generator=g, dtype=torch.int32)
        tok[torch.rand(rt, tmax + 2, generator=g) < 0.2] = pad_value
        even = torch.arange(0, self.rows, 2) * row_mult
        for j in (t - 1, t - 2):
            if j >= 0:
                tok[even, j] = 7
        self.tokens = tok                                     # row stride tmax + 2
        self._ops = None

    @property
    def route(self):
        return self_route(self.dt, self.dh, self.t + 1)

    def what(self):
        return dict(t=self.t, rows_per_img=self.rows_per_img, row_mult=self.row_mult, dh=self.dh, pad_index=self.pad_index)

    def operands(self):
        """q [R, H, 1, dh], keys / values [R, H, L, dh] gathered through ``src``, masked [R, 1, 1, L]."""
        d, h, dh, t = self.d, self.n_heads, self.dh, self.t
        rl = torch.arange(self.rows) * self.row_mult
        idx = self.src[rl, :t].long()                                                        # [R, t]
        pos = torch.arange(t)[None, :]
        k = torch.cat([self.kc[pos, idx], self.qkv[:, None, d:2 * d]], 1)                    # [R, L, D]
        v = torch.cat([self.vc[pos, idx], self.qkv[:, None, 2 * d:]], 1)
        masked = torch.zeros(self.rows, t + 1, dtype=torch.bool)
        if self.pad_index >= 0:
            masked[:, 1:] = self.tokens[rl, :t] == self.pad_index                           # key 0 is never masked
        split = lambda x: x.reshape(self.rows, -1, h, dh).transpose(1, 2)                   # noqa: E731
        return split(self.qkv[:, None, :d]), split(k), split(v), masked[:, None, None, :]

    def want(self, drop=None):
        """fp64 result [R, D]; ``drop``: that key is left out altogether (the sensitivity condition)."""
        if self._ops is None:
            self._ops = self.operands()
        q, k, v, masked = self._ops
        dead = None
        if drop is not None:
            dead = torch.zeros(1, 1, 1, self.t + 1, dtype=torch.bool)
            dead[..., drop] = True
        return attn_ref(q, k, v, masked, self.scale, dead).transpose(1, 2).reshape(self.rows, self.d)


def self_sweep_cases(dt, pad_index):
    """dh 64, beam 4, 3 images, every t from 0 to 127 (L = 1 .. 128: max_len 128 is the position table's limit)."""
    cache = {}
    for t in range(128):
        yield SelfCase(dt, 3, 4, 1, 512, 8, t, 128, pad_index, 8.0, cache)


def self_row_block_cases(dt):
    for rpi in ROW_BLOCKS:
        cache = {}
        for t in BOUNDARY_T:
            yield SelfCase(dt, 2, rpi, 1, 512, 8, t, 101, (0, 5, -1)[t % 3], 8.0, cache)


def self_row_mult_cases(dt):
    for row_mult in (4, 20):                                  # one compact row per image, "before the first draw"
        cache = {}
        for t in BOUNDARY_T:
            yield SelfCase(dt, 3, 1, row_mult, 512, 8, t, 101, (0, 5, -1)[t % 3], 8.0, cache)


def self_head_dim_cases(dt):
    for d, h in HEAD_DIMS:
        for beam in (3, 20):
            cache = {}
            for t in HEAD_DIM_T:
                yield SelfCase(dt, 2, beam, 1, d, h, t, 101, (0, 5, -1)[t % 3], float(d // h) ** 0.5, cache)


SELF_CASE_SETS = {"row_blocks": self_row_block_cases, "row_mult": self_row_mult_cases, "head_dims": self_head_dim_cases}


# ---- decode cross-attention (dh_attn_cross_decode, dh_attn_cross_decode_packed) ---------------------------------------------
CROSS_S = (1, 2, 7, 15, 16, 17, 48, 49, 50, 63, 64, 65, 100, 128)
CROSS_ROWS = (1, 5, 16, 17, 40)
CROSS_OTHER = ((256, 8), (512, 4), (128, 8))                  # (D, H): head dim 32, 128, 16
PACKED_S = (1, 7, 16, 17, 48, 49, 63, 64)


class CrossCase:
    """3 images: image 0 has one masked key (key min(3, S - 1)), image 1 is fully masked (uniform weights), image 2 has only
    its last key live.  q is the column block D:2D of a [rows, 3D] buffer; a test passes it as that slice (ldq = 3D) or as
    a contiguous copy."""

    def __init__(self, dt, rows_per_img, s, d, n_heads, scale):
        self.dt, self.n_img, self.rows_per_img, self.s, self.d, self.n_heads, self.scale = dt, 3, rows_per_img, s, d, n_heads, scale
        self.rows, self.dh = 3 * rows_per_img, d // n_heads
        g = torch.Generator().manual_seed(131 * s + rows_per_img + d)
        self.wide = torch.randn(self.rows, 3 * d, generator=g).to(dt)
        self.kv = torch.randn(3 * s, 2 * d, generator=g).to(dt)
        mask = torch.zeros(3 * s, dtype=torch.uint8)
        mask[min(3, s - 1)] = 1
        mask[s:2 * s] = 1
        mask[2 * s:3 * s - 1] = 1
        self.mask = mask

    @property
    def q(self):
        return self.wide[:, self.d:2 * self.d]

    def what(self):
        return dict(s=self.s, rows_per_img=self.rows_per_img, dh=self.dh)

    def operands(self):
        d, h, dh, s, n = self.d, self.n_heads, self.dh, self.s, self.n_img
        q = self.q.reshape(n, self.rows_per_img, h, dh).transpose(1, 2)
        k = self.kv[:, :d].reshape(n, s, h, dh).transpose(1, 2)
        v = self.kv[:, d:].reshape(n, s, h, dh).transpose(1, 2)
        return q, k, v, self.mask.view(n, 1, 1, s).bool()

    def want(self):
        q, k, v, masked = self.operands()
        return attn_ref(q, k, v, masked, self.scale).transpose(1, 2).reshape(self.rows, self.d)

    def want_weights_rounded(self):
        """The matrix-core kernel's arithmetic (attn_items.h cross_core) restated: the softmax weights are rounded to the
        operand type before the P V product; everything else in fp64.  Not rounded to the output type."""
        q, k, v, masked = self.operands()
        energy = (torch.einsum("bhtd,bhsd->bhts", q.double(), k.double()) / self.scale).masked_fill(masked, -1e8)
        p = torch.softmax(energy, -1).to(self.dt).double()
        return torch.einsum("bhts,bhsd->bhtd", p, v.double()).transpose(1, 2).reshape(self.rows, self.d)


def cross_cases(dt):
    for s in CROSS_S:
        for rpi in CROSS_ROWS:
            yield CrossCase(dt, rpi, s, 512, 8, 8.0)
    for d, h in CROSS_OTHER:
        for s in (7, 49, 100):
            for rpi in (5, 17):
                yield CrossCase(dt, rpi, s, d, h, float(d // h) ** 0.5)


def packed_cases(dt):
    for s in PACKED_S:
        for rpi in range(1, 17):
            yield CrossCase(dt, rpi, s, 512, 8, 8.0)
