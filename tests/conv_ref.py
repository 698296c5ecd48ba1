"""What the general-convolution tests share (test_conv_routes_gpu.py, test_conv_ref_cpu.py): dh_conv2d_nhwc_bn_act,
dh_conv1x1_dual_nhwc, dh_conv2d_nhwc_bn_relu_maxpool (csrc/gemm_bf16.hip) and dh_conv2d_bn_act / dh_stem_conv_nhwc (csrc/conv.hip)
stated plainly in fp64, the restated choices of their launchers, and the cases of every loader, tile route, ring depth, shape edge
and epilogue form with their operands and expected results.  Plain module, no GPU use: the cases are built on the CPU.

Two operand flavours, as in linear_ref.  "int": entries in [-3, 3], shift / residual integers in [-8, 8], scale a power of two:
every partial sum is exact in fp32 in any order, the output must torch.equal the exact value rounded once.  "real": randn operands
with w / sqrt(K), compared with fp64 in ulps (16-bit outputs) or by absolute error (fp32 outputs)."""
import functools

import torch
import torch.nn.functional as F

from attn_ref import BF16, F16, F32, F32_ATOL, ULP_FLOOR, ulps  # noqa: F401  (re-exported for the two test modules)
from linear_ref import EXTRA_ROWS, FLAVOURS, NS, SENTINEL, RouteGates, cdiv, epilogue_ref, ring_route  # noqa: F401
from lstm_ref import DT16, DT16_IDS, AbsGate  # noqa: F401

GUARD = 64                                                    # sentinel elements before and after every tensor (128 / 256 bytes)
FORMS = {"affine": (0, 0), "residual": (1, 0), "relu": (0, 1), "all": (1, 1)}      # (residual, relu); scale and shift always
FORM_NAMES = tuple(FORMS)
SQUARE = ((8, 128, 128), (42, 56, 56))                        # (n, h, w) of two narrow shapes; every other case has H != W


def out_hw(h, w, ks, stride, pad):
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


# ---- the references ---------------------------------------------------------------------------------------------------------
def conv_acc(x_nhwc, w, stride, pad, dtype=torch.float64):
    """The bare convolution of a channels-last input with w [Cout, KS, KS, Cin], channels-last, computed in ``dtype``."""
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2).to(dtype), w.permute(0, 3, 1, 2).to(dtype), stride=stride, padding=pad).permute(0, 2, 3, 1)


def conv_ref(x_nhwc, w, scale, shift, residual=None, relu=False, stride=1, pad=0):
    """act(conv(x, w) * scale + shift + residual) in fp64, channels-last, on the operands as the kernel sees them."""
    return epilogue_ref(conv_acc(x_nhwc, w, stride, pad), None, scale, shift, residual, relu)


def pool_nhwc(y):
    """MaxPool2d(3, 2, 1) of a channels-last tensor."""
    return F.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def conv_pool_ref(x_nhwc, w, scale, shift, stride, pad):
    """Convolution, then affine, then ReLU, then MaxPool2d(3, 2, 1), fp64."""
    return pool_nhwc(conv_ref(x_nhwc, w, scale, shift, None, True, stride, pad))


def dual_operand(y, x, stride):
    """[y | x at the strided pixels] as rows: [N Ho Wo, C1 + C2]."""
    n, ho, wo, c1 = y.shape
    xs = x[:, ::stride, ::stride][:, :ho, :wo]
    return torch.cat([y.reshape(n * ho * wo, c1), xs.reshape(n * ho * wo, x.shape[3])], 1)


def dual_ref(y, x, w_cat, shift, stride, relu):
    """[y | x at the strided pixels] @ w_cat.T + shift in fp64, [N, Ho, Wo, Cout]."""
    n, ho, wo, _ = y.shape
    out = dual_operand(y, x, stride).double() @ w_cat.double().t() + shift.double()
    return (torch.relu(out) if relu else out).view(n, ho, wo, -1)


def conv_nchw_ref(x, w, scale, shift, residual=None, relu=False, stride=1, pad=0):
    """dh_conv2d_bn_act / dh_stem_conv_nhwc: NCHW input, w [Cout, Cin, KS, KS], NCHW output, fp64."""
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


# ---- the launchers' choices, restated -------------------------------------------------------------------------------------------
def loader(cin, ks, stride, pad):
    """csrc/gemm_bf16.hip dh_conv2d_nhwc_bn_act: "if (KS == 1 && stride == 1 && pad == 0) { p.lda = Cin; p.conv = 0; ..." (the
    dense loader), else the CONV kernel, in which "const bool tap_uniform = CONV && (p.Cin & 63) == 0;"."""
    if ks == 1 and stride == 1 and pad == 0:
        return "dense"
    return "tap" if cin % 64 == 0 else "generic"


def tile(m, n, k, conv):
    """csrc/gemm_bf16.hip launch_gemm_bf16: "if (big_tiles >= 192 && p.M >= 96 && p.N >= 96 && !lnx)" (128 x 128),
    "if (p.N <= 64 && p.M >= 256 * 512 && !lnx)" with "if (CONV) { ...<OT, 256, 64, 4, CONV, 2, 8>" / "else { // dense 1x1 ...
    <OT, 128, 64, 2, CONV, 2, 4>", then the ring choice (linear_ref.ring_route) over 64 x 64 workgroups."""
    if cdiv(m, 128) * cdiv(n, 128) >= 192 and m >= 96 and n >= 96:
        return "t128"
    if n <= 64 and m >= 256 * 512:
        return "c256" if conv else "n64"
    return ring_route(cdiv(m, 64) * cdiv(n, 64), k)


def n_fast(m, n, k, cin, conv):
    """launch_gemm_bf16: "w_bytes = 2.0 * p.N * p.K, a_bytes = 2.0 * p.M * (CONV ? p.Cin : p.K)" and
    "p.n_fast = w_bytes <= 8.0 * 1024 * 1024 && a_bytes > w_bytes"."""
    w_bytes, a_bytes = 2.0 * n * k, 2.0 * m * (cin if conv else k)
    return int(w_bytes <= 8.0 * 1024 * 1024 and a_bytes > w_bytes)


def magic(d, limit):
    """dh_conv2d_nhwc_bn_act's host lambda: "mg = ((1u << 20) + d - 1) / d", "if (limit * mg >= (1ull << 32)) return 0", and 0
    unless "(v * mg) >> 20 == v / d" for every v < limit (the product taken in 32 bits, as the kernel does)."""
    mg = ((1 << 20) + d - 1) // d
    if limit * mg >= 1 << 32:
        return 0
    v = torch.arange(limit, dtype=torch.int64)
    return mg if bool(((((v * mg) & 0xFFFFFFFF) >> 20) == v // d).all()) else 0


def accepted(cin, ks):
    """"p.cin_magic = magic(Cin, p.K); p.ks_magic = magic(KS, KS * KS); DH_REQUIRE((Cin % 64) == 0 || (p.cin_magic &&
    p.ks_magic));" together with "DH_REQUIRE((Cin % 8) == 0 && KS >= 1 && ..."."""
    return cin % 8 == 0 and (cin % 64 == 0 or bool(magic(cin, ks * ks * cin) and magic(ks, ks * ks)))


def f32_route(cout, ks, ho, wo, stem=False):
    """csrc/conv.hip: "const bool big = Cout >= 128;" picks launch_conv<128, KS> or <64, KS> (dh_stem_conv_nhwc: "Cout >= 128"
    likewise); in the NCHW epilogue "const bool vec = (HoWo % 4) == 0;".  The stem's channels-last epilogue has one form."""
    assert ks in ((7, 3) if stem else (1, 3, 7))
    name = f"tm{128 if cout >= 128 else 64}_k{ks}"
    return "stem_" + name if stem else name + ("_vec" if ho * wo % 4 == 0 else "_px")


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (1 << 61)
    return torch.Generator().manual_seed(seed)


def _draw(g, fl, shape, lim=3, std=1.0):
    if fl == "int":
        return torch.randint(-lim, lim + 1, shape, generator=g).float()
    return torch.randn(shape, generator=g) * std


def _vectors(g, fl, cout, res_shape, dt):
    """scale, shift (fp32) and a residual (``dt``) of ``res_shape``."""
    if fl == "int":
        scale = 2.0 ** torch.randint(-1, 2, (cout,), generator=g).float()
        shift = torch.randint(-8, 9, (cout,), generator=g).float()
        res = torch.randint(-8, 9, res_shape, generator=g).float()
    else:
        scale, shift = torch.rand(cout, generator=g) + 0.5, 0.3 * torch.randn(cout, generator=g)
        res = torch.randn(res_shape, generator=g)
    return scale, shift, res.to(dt)


@functools.lru_cache(maxsize=2)
def _conv_operands(dt, fl, n, h, w, cin, cout, ks, stride, pad, seed):
    """x [n, h, w, cin], wgt [cout, ks, ks, cin] in ``dt``; scale, shift; residual [n, ho, wo, cout] in ``dt``; the bare
    convolution in fp64 (int flavour: computed in fp32, which is exact there -- test_conv_ref_cpu checks it)."""
    g = _gen(seed, n, h, w, cin, cout, ks, stride, pad)
    k = ks * ks * cin
    x, wgt = _draw(g, fl, (n, h, w, cin)).to(dt), _draw(g, fl, (cout, ks, ks, cin), std=k ** -0.5).to(dt)
    ho, wo = out_hw(h, w, ks, stride, pad)
    scale, shift, res = _vectors(g, fl, cout, (n, ho, wo, cout), dt)
    acc = conv_acc(x, wgt, stride, pad, F32 if fl == "int" else torch.float64).double()
    return x, wgt, scale, shift, res, acc


class ConvCase:
    """One dh_conv2d_nhwc_bn_act call (``pool``: dh_conv2d_nhwc_bn_relu_maxpool).  Operands are drawn on first use, so the
    route tables can be checked without them; the int flavour's do not depend on ``dt``."""

    def __init__(self, dt, flavour, n, h, w, cin, cout, ks, stride=1, pad=0, form="affine", pool=False, seed=0):
        assert flavour in FLAVOURS and form in FORMS
        self.dt, self.flavour, self.n, self.h, self.w, self.cin, self.cout = dt, flavour, n, h, w, cin, cout
        self.ks, self.stride, self.pad, self.form, self.pool, self.seed = ks, stride, pad, form, pool, seed
        self.has_res, self.relu = (bool(v) for v in FORMS[form])
        self.ho, self.wo = out_hw(h, w, ks, stride, pad)
        self.m, self.k = n * self.ho * self.wo, ks * ks * cin
        assert self.ho > 0 and self.wo > 0 and not (pool and (self.has_res or self.ho % 2 or self.wo % 2))
        self.out_dt = dt

    # -- what the launchers see
    @property
    def loader(self):
        return loader(self.cin, self.ks, self.stride, self.pad)

    @property
    def tile(self):
        return tile(self.m, self.cout, self.k, self.loader != "dense")

    @property
    def route(self):
        return "pool" if self.pool else f"{self.loader}_{self.tile}"

    @property
    def blocks(self):
        return cdiv(self.m, 64) * cdiv(self.cout, 64)

    @property
    def n_fast(self):
        return n_fast(self.m, self.cout, self.k, self.cin, self.loader != "dense")

    @property
    def nslab(self):
        return cdiv(self.k, 64)

    @property
    def out_shape(self):
        return (self.n, self.ho // 2, self.wo // 2, self.cout) if self.pool else (self.n, self.ho, self.wo, self.cout)

    def what(self):
        return dict(n=self.n, hw=(self.h, self.w), cin=self.cin, cout=self.cout, ks=self.ks, s=self.stride, p=self.pad,
                    fl=self.flavour, form="pool" if self.pool else self.form)

    # -- operands
    def _ops(self):
        return _conv_operands(F32 if self.flavour == "int" else self.dt, self.flavour, self.n, self.h, self.w, self.cin, self.cout,
                              self.ks, self.stride, self.pad, self.seed)

    x = property(lambda self: self._ops()[0].to(self.dt))
    wgt = property(lambda self: self._ops()[1].to(self.dt))
    scale = property(lambda self: self._ops()[2])
    shift = property(lambda self: self._ops()[3])
    residual = property(lambda self: self._ops()[4].to(self.dt) if self.has_res else None)

    # -- expected
    def want(self, drop=None):
        """fp64, channels-last.  ``drop``: a bool mask [ks, ks, cin] of weight entries taken as zero (the sensitivity condition)."""
        acc = self._ops()[5]
        if drop is not None:
            acc = acc - conv_acc(self.x, self.wgt * drop.to(self.dt), self.stride, self.pad, F32).double()
        y = epilogue_ref(acc, None, self.scale, self.shift, self.residual, self.relu or self.pool)
        return pool_nhwc(y) if self.pool else y

    def want_out(self):
        assert self.flavour == "int"
        return self.want().to(self.out_dt)

    def live(self, drop):
        """Output elements that the dropped weights reach at all (a border tap lies outside the image for some pixels)."""
        ones = torch.ones(self.n, self.h, self.w, self.cin)
        hit = conv_acc(ones, drop.float()[None], self.stride, self.pad, F32) > 0
        if self.pool:
            hit = pool_nhwc(hit.float()) > 0
        return hit.expand(self.out_shape)

    def slab_masks(self):
        """The weights of each 64-wide K slab (k = (kh, kw, ci), ci fastest; the tail last), then those of each filter tap."""
        for k0 in range(0, self.k, 64):
            mask = torch.zeros(self.k, dtype=torch.bool)
            mask[k0:k0 + 64] = True
            yield ("slab", k0), mask.view(self.ks, self.ks, self.cin)
        if self.ks > 1:
            for t in range(self.ks * self.ks):
                mask = torch.zeros(self.ks * self.ks, self.cin, dtype=torch.bool)
                mask[t] = True
                yield ("tap", t), mask.view(self.ks, self.ks, self.cin)


@functools.lru_cache(maxsize=2)
def _dual_operands(dt, fl, n, ho, wo, c1, h, w, c2, stride, cout, seed):
    g = _gen(seed, n, ho, wo, c1, h, w, c2, stride, cout, 1)
    k = c1 + c2
    y, x = _draw(g, fl, (n, ho, wo, c1)).to(dt), _draw(g, fl, (n, h, w, c2)).to(dt)
    w_cat = _draw(g, fl, (cout, k), std=k ** -0.5).to(dt)
    _, shift, _ = _vectors(g, fl, cout, (1,), dt)
    a = dual_operand(y, x, stride)
    acc = (a.float() @ w_cat.float().t()).double() if fl == "int" else a.double() @ w_cat.double().t()
    return y, x, w_cat, shift, acc


class DualCase:
    """One dh_conv1x1_dual_nhwc call: y [n, ho, wo, c1], x [n, h, w, c2], w_cat [cout, c1 + c2], shift."""

    def __init__(self, dt, flavour, n, ho, wo, c1, c2, stride, cout, relu, extra_hw=(0, 0), seed=0):
        assert flavour in FLAVOURS
        self.dt, self.flavour, self.n, self.ho, self.wo, self.c1, self.c2, self.stride = dt, flavour, n, ho, wo, c1, c2, stride
        self.cout, self.relu, self.seed = cout, relu, seed
        self.h, self.w = (ho - 1) * stride + 1 + extra_hw[0], (wo - 1) * stride + 1 + extra_hw[1]
        self.m, self.k, self.out_dt, self.out_shape = n * ho * wo, c1 + c2, dt, (n, ho, wo, cout)

    @property
    def tile(self):
        return tile(self.m, self.cout, self.k, False)

    @property
    def route(self):
        return "dual_" + self.tile

    @property
    def blocks(self):
        return cdiv(self.m, 64) * cdiv(self.cout, 64)

    def what(self):
        return dict(n=self.n, out=(self.ho, self.wo), hw=(self.h, self.w), c1=self.c1, c2=self.c2, s=self.stride, cout=self.cout,
                    relu=self.relu, fl=self.flavour)

    def _ops(self):
        return _dual_operands(F32 if self.flavour == "int" else self.dt, self.flavour, self.n, self.ho, self.wo, self.c1, self.h,
                              self.w, self.c2, self.stride, self.cout, self.seed)

    y = property(lambda self: self._ops()[0].to(self.dt))
    x = property(lambda self: self._ops()[1].to(self.dt))
    w_cat = property(lambda self: self._ops()[2].to(self.dt))
    shift = property(lambda self: self._ops()[3])

    def want(self, drop=None):
        """``drop``: a bool mask [c1 + c2] of operand columns taken as zero."""
        acc = self._ops()[4]
        if drop is not None:
            acc = acc - (dual_operand(self.y, self.x, self.stride)[:, drop].float() @ self.w_cat[:, drop].float().t()).double()
        out = acc + self.shift.double()
        return (torch.relu(out) if self.relu else out).view(self.out_shape)

    def want_out(self):
        assert self.flavour == "int"
        return self.want().to(self.out_dt)

    def live(self, drop):
        return torch.ones(self.out_shape, dtype=torch.bool)

    def slab_masks(self):
        for k0 in range(0, self.k, 64):
            mask = torch.zeros(self.k, dtype=torch.bool)
            mask[k0:k0 + 64] = True
            yield ("slab", k0), mask


@functools.lru_cache(maxsize=2)
def _nchw_operands(fl, n, cin, h, w, cout, ks, stride, pad, seed):
    g = _gen(seed, n, cin, h, w, cout, ks, stride, pad, 2)
    k = ks * ks * cin
    x, wgt = _draw(g, fl, (n, cin, h, w)), _draw(g, fl, (cout, cin, ks, ks), std=k ** -0.5)
    ho, wo = out_hw(h, w, ks, stride, pad)
    scale, shift, res = _vectors(g, fl, cout, (n, cout, ho, wo), F32)
    acc = F.conv2d(x, wgt, stride=stride, padding=pad).double() if fl == "int" else F.conv2d(x.double(), wgt.double(), stride=stride, padding=pad)
    return x, wgt, scale, shift, res, acc


class NchwCase:
    """One dh_conv2d_bn_act call (fp32, NCHW in and out) or, ``stem_dt`` given, one dh_stem_conv_nhwc call (fp32 NCHW in,
    channels-last ``stem_dt`` out, no residual).  w [cout, cin, ks, ks]; K runs over (ci, kh, kw), kw fastest, in slabs of 16."""

    def __init__(self, flavour, n, cin, h, w, cout, ks, stride=1, pad=0, form="affine", stem_dt=None, seed=0):
        assert flavour in FLAVOURS and form in FORMS and not (stem_dt is not None and FORMS[form][0])
        self.flavour, self.n, self.cin, self.h, self.w, self.cout, self.ks = flavour, n, cin, h, w, cout, ks
        self.stride, self.pad, self.form, self.stem_dt, self.seed = stride, pad, form, stem_dt, seed
        self.has_res, self.relu = (bool(v) for v in FORMS[form])
        self.ho, self.wo = out_hw(h, w, ks, stride, pad)
        self.m, self.k = n * self.ho * self.wo, ks * ks * cin
        self.dt, self.out_dt = F32, stem_dt if stem_dt is not None else F32
        self.out_shape = (n, self.ho, self.wo, cout) if stem_dt is not None else (n, cout, self.ho, self.wo)

    @property
    def route(self):
        return f32_route(self.cout, self.ks, self.ho, self.wo, self.stem_dt is not None)

    def what(self):
        return dict(n=self.n, cin=self.cin, hw=(self.h, self.w), cout=self.cout, ks=self.ks, s=self.stride, p=self.pad,
                    fl=self.flavour, form=self.form)

    def _ops(self):
        return _nchw_operands(self.flavour, self.n, self.cin, self.h, self.w, self.cout, self.ks, self.stride, self.pad, self.seed)

    x = property(lambda self: self._ops()[0])
    wgt = property(lambda self: self._ops()[1])
    scale = property(lambda self: self._ops()[2])
    shift = property(lambda self: self._ops()[3])
    residual = property(lambda self: self._ops()[4] if self.has_res else None)

    def want(self, drop=None):
        """fp64 in the output's layout.  ``drop``: a bool mask [cin, ks, ks] of weight entries taken as zero."""
        acc = self._ops()[5]
        if drop is not None:
            acc = acc - F.conv2d(self.x, self.wgt * drop, stride=self.stride, padding=self.pad).double()
        y = acc * self.scale.double()[None, :, None, None] + self.shift.double()[None, :, None, None]
        if self.has_res:
            y = y + self.residual.double()
        y = torch.relu(y) if self.relu else y
        return y.permute(0, 2, 3, 1) if self.stem_dt is not None else y

    def want_out(self):
        assert self.flavour == "int"
        return self.want().to(self.out_dt)

    def live(self, drop):
        hit = F.conv2d(torch.ones(self.n, self.cin, self.h, self.w), drop.float()[None], stride=self.stride, padding=self.pad) > 0
        hit = hit.expand(self.n, self.cout, self.ho, self.wo)
        return hit.permute(0, 2, 3, 1) if self.stem_dt is not None else hit

    def slab_masks(self):
        for k0 in range(0, self.k, 16):
            mask = torch.zeros(self.k, dtype=torch.bool)
            mask[k0:k0 + 16] = True
            yield ("slab", k0), mask.view(self.cin, self.ks, self.ks)
        if self.ks > 1:
            for t in range(self.ks * self.ks):
                mask = torch.zeros(self.cin, self.ks * self.ks, dtype=torch.bool)
                mask[:, t] = True
                yield ("tap", t), mask.view(self.cin, self.ks, self.ks)


def as_rows(c, y):
    """An output of case ``c`` as [pixels, channels] rows, the GEMM's view of it."""
    if isinstance(c, NchwCase) and c.stem_dt is None:
        y = y.permute(0, 2, 3, 1)
    return y.reshape(-1, c.cout)


# ---- A. dh_conv2d_nhwc_bn_act -------------------------------------------------------------------------------------------------
# 1. ring switches on the CONV path: 1x1 stride 2, Cin 192 (K > 128), (n, h, w, cout) -> (workgroups, tile); the last: Cin 64
RING_SWITCH = (
    ((1, 9, 25, 10232), (320, "r8")), ((4, 117, 173, 60), (321, "r4")), ((1, 9, 25, 16376), (512, "r4")),
    ((4, 163, 199, 60), (513, "r3")), ((1, 9, 25, 24568), (768, "r3")), ((1, 13, 17, 49208), (769, "r2")),
    ((1, 9, 25, 40952), (1280, "r2")), ((1, 13, 17, 81976), (1281, "r4")), ((1, 9, 25, 10232), (320, "r4")),
)


def ring_switch_cases(dt, fl):
    for i, ((n, h, w, cout), _) in enumerate(RING_SWITCH):
        yield ConvCase(dt, fl, n, h, w, 64 if i == len(RING_SWITCH) - 1 else 192, cout, 1, 2, 0)


# 2. the tap-uniform loader against ring depth.  Images per ring (by workgroup count, Cout 72: two column tiles, the second
# partial) at 71 x 90 output pixels per image: r4 2 (400 workgroups), r3 3 (600), r2 4 (800); r8: one 9 x 14 map (4).
TAP_IMAGES = {"r8": 1, "r4": 2, "r3": 3, "r2": 4}
TAP_COUT = 72
TAP_MULTI = ((3, 64), (3, 128), (3, 256), (2, 64), (2, 128))    # (KS, Cin): the tap changes every slab / second / fourth slab


def tap_slab_counts(route):
    """1x1 stride 2 with Cin = 64 s: s in NS - 2 .. NS + 1 and 2 NS + 1 (K <= 128 is always r4, so s >= 3 elsewhere)."""
    ns = NS[route]
    return sorted(s for s in {ns - 2, ns - 1, ns, ns + 1, 2 * ns + 1} if s >= (1 if route == "r4" else 3))


def tap_cases(dt, fl):
    for route, n in TAP_IMAGES.items():
        ho, wo = (9, 14) if route == "r8" else (71, 90)
        for ks, cin in TAP_MULTI:
            if ks == 3 and cin == 256 and route in ("r3", "r2"):
                continue                                      # 36 slabs: on the two cheap rings only
            pad = 1 if ks == 3 else 0
            yield ConvCase(dt, fl, n, ho + ks - 1 - 2 * pad, wo + ks - 1 - 2 * pad, cin, TAP_COUT, ks, 1, pad)
        for s in tap_slab_counts(route):
            yield ConvCase(dt, fl, n, 2 * ho - 1, 2 * wo - 1, 64 * s, TAP_COUT, 1, 2, 0)
    yield ConvCase(dt, fl, 2, 7, 9, 512, 72, 3, 1, 1)          # one long reduction: K = 4608, 72 slabs


# 3. the generic loader: Cin x KS, (stride, pad) in turn; K % 64 != 0 (the non-stepping W loader) and == 0 (Cin 16, KS 2)
GENERIC_CIN = (8, 16, 24, 40)
GENERIC_KS = (2, 3, 5, 7)
GENERIC_SP = ((1, 0), (2, 1), (1, 3), (2, 0), (1, 1), (2, 3))   # with KS 2, pad 3 >= KS


def generic_cases(dt, fl):
    i = 0
    for cin in GENERIC_CIN:
        for ks in GENERIC_KS:
            stride, pad = GENERIC_SP[i % len(GENERIC_SP)]
            i += 1
            yield ConvCase(dt, fl, 2, 13, 17, cin, 72, ks, stride, pad)
    yield ConvCase(dt, fl, 2, 13, 17, 16, 72, 2, 1, 3)          # pad >= KS, K % 64 == 0
    yield ConvCase(dt, fl, 3, 11, 15, 8, 136, 7, 2, 3)          # the stem's form, K = 392, stride 2 on odd sizes


# 4. big tiles: 192 of them exactly, in both tile orders; 191 tiles, M = 95 and N = 95 fall back to the rings
def big_tile_cases(dt, fl):
    yield ConvCase(dt, fl, 3, 33, 31, 64, 1024, 3, 1, 1)        # 24 x 8 tiles, tap, n_fast 0
    yield ConvCase(dt, fl, 3, 65, 61, 192, 1016, 1, 2, 0)       # 24 x 8 tiles, tap, n_fast 1
    yield ConvCase(dt, fl, 3, 33, 31, 8, 1016, 3, 1, 1)         # 24 x 8 tiles, generic
    yield ConvCase(dt, fl, 3, 17, 19, 64, 3064, 3, 1, 1)        # 8 x 24 tiles
    yield ConvCase(dt, fl, 2, 13, 17, 192, 24440, 1, 2, 0)      # M = 126, 1 x 191 tiles
    yield ConvCase(dt, fl, 1, 9, 37, 192, 24568, 1, 2, 0)       # M = 95, 1 x 192 tiles
    yield ConvCase(dt, fl, 10, 63, 155, 64, 95, 1, 2, 0)        # N = 95, M = 24960: 195 x 1 tiles


# 5. narrow outputs with very many pixels
def narrow_cases(dt, fl):
    yield ConvCase(dt, fl, 8, 128, 128, 8, 64, 3, 1, 1)         # 131072 pixels, generic: c256
    yield ConvCase(dt, fl, 42, 56, 56, 64, 64, 3, 1, 1)         # 131712 pixels, tap: c256
    yield ConvCase(dt, fl, 8, 129, 127, 8, 64, 3, 1, 1)         # 131064 pixels: a ring
    yield ConvCase(dt, fl, 4, 128, 256, 64, 40, 1, 1, 0)        # dense 1x1, 131072 pixels: n64


# 6. shape edges: M in 1 .. 130 output pixels (1 x 1 maps, maps smaller than the filter reach, images sharing a 64-row tile)
# x Cout (60: the element-wise epilogue; 68: a partial last chunk inside the 16-byte path; 130: scalar scale / shift loads)
EDGE_MAPS = (   # (n, h, w, ks, stride, pad) -> output pixels
    ((1, 3, 5, 3, 3, 0), 1), ((1, 7, 9, 3, 1, 1), 63), ((2, 4, 8, 3, 1, 1), 64), ((1, 5, 13, 3, 1, 1), 65), ((2, 5, 13, 3, 1, 1), 130),
    ((3, 2, 3, 5, 1, 2), 18), ((5, 1, 3, 3, 2, 1), 10), ((2, 9, 25, 1, 2, 0), 130), ((1, 7, 9, 1, 1, 0), 63), ((2, 5, 13, 1, 1, 0), 130),
)
EDGE_COUT = (8, 60, 64, 68, 130)
EDGE_CIN = (64, 16, 136)                                      # tap / generic / generic (dense for the 1x1 stride 1 maps)


def edge_cases(dt, fl):
    for (n, h, w, ks, stride, pad), _ in EDGE_MAPS:
        for cout in EDGE_COUT:
            for cin in EDGE_CIN:
                yield ConvCase(dt, fl, n, h, w, cin, cout, ks, stride, pad)


# 7. epilogue forms on a 16-byte Cout and on Cout = 60
FORM_SHAPES = ((2, 5, 13, 64, 3, 1, 1), (2, 9, 25, 24, 3, 2, 1), (2, 5, 13, 136, 1, 1, 0))    # (n, h, w, cin, ks, stride, pad)
FORM_COUT = (72, 60)


def form_cases(dt, fl):
    for n, h, w, cin, ks, stride, pad in FORM_SHAPES:
        for cout in FORM_COUT:
            for form in FORM_NAMES:
                yield ConvCase(dt, fl, n, h, w, cin, cout, ks, stride, pad, form, seed=1)


# ---- B. dh_conv1x1_dual_nhwc ----------------------------------------------------------------------------------------------------
# images per ring at 71 x 45 output pixels and Cout 72 (two column tiles): r4 4 (400 workgroups), r3 6 (600), r2 8 (800)
DUAL_IMAGES = {"r8": 1, "r4": 4, "r3": 6, "r2": 8}


def dual_c1_slabs(route):
    """C1 / 64: the switch to the second source in the prologue (slab < NS - 1), on its last slab and inside the loop."""
    ns = NS[route]
    return sorted(s for s in {1, ns - 2, ns - 1, ns} if s >= 1)


def dual_cases(dt, fl):
    """The second source is 256 channels wide at stride 1 and 64 wide at stride 2; the two big rings take one width per C1."""
    for route, n in DUAL_IMAGES.items():
        ho, wo = (9, 14) if route == "r8" else (71, 45)
        j = 0
        for s in dual_c1_slabs(route):
            for c2 in (256, 64):
                if route != "r4" and 64 * s + c2 <= 128:
                    continue                                  # K <= 128 is always r4
                if route in ("r3", "r2") and c2 != (256 if s % 2 else 64):
                    continue
                yield DualCase(dt, fl, n, ho, wo, 64 * s, c2, 1 if c2 == 256 else 2, 72, relu=bool(j % 2), extra_hw=(2, 1) if j % 3 == 0 else (0, 0))
                j += 1
    yield DualCase(dt, fl, 1, 9, 14, 64, 64, 2, 72, relu=True)                  # K = 128: r4 by its other reason
    yield DualCase(dt, fl, 3, 33, 31, 64, 64, 2, 1024, relu=True)               # 24 x 8 big tiles: t128
    yield DualCase(dt, fl, 3, 33, 31, 128, 256, 1, 1016, relu=False, extra_hw=(1, 2))


# ---- C. dh_conv2d_nhwc_bn_relu_maxpool ------------------------------------------------------------------------------------------
POOL_MAPS = ((1, 1), (7, 7), (8, 7), (7, 15), (16, 12))       # pooled (Hp, Wp): one block, an exact one, a one-row spill, partial blocks
POOL_COUT = (8, 40, 64)


def pool_cases(dt, fl):
    i = 0
    for hp, wp in POOL_MAPS:
        for cout in POOL_COUT:
            # KS 7 stride 2 pad 3: Ho = (H - 1) // 2 + 1, so H = 4 Hp - 1 and W = 4 Wp give Ho = 2 Hp, Wo = 2 Wp
            yield ConvCase(dt, fl, 2 + i % 2, 4 * hp - 1, 4 * wp, 8, cout, 7, 2, 3, pool=True)
            i += 1
    yield ConvCase(dt, fl, 2, 16, 14, 8, 40, 3, 1, 1, pool=True)                # KS 3 stride 1 pad 1: pooled 8 x 7
    yield ConvCase(dt, fl, 3, 14, 30, 16, 64, 3, 1, 1, pool=True)               # Cin 16, pooled 7 x 15


# ---- D. dh_conv2d_bn_act (fp32, NCHW) -------------------------------------------------------------------------------------------
F32_CIN = {1: 20, 3: 5, 7: 3}                                 # K = 20 / 45 / 147: K % 16 != 0
F32_GEOM = (   # (n, h, w, stride): output maps 7 x 7 (a thread's four pixels straddle two images), 6 x 10 (vec), 10 x 12 x 3 (P > 128)
    (3, 13, 14, 2), (2, 6, 10, 1), (3, 10, 12, 1), (2, 11, 15, 2),
)


def f32_cases(fl):
    i = 0
    for ks in (1, 3, 7):
        for cout in (60, 64, 130):
            for n, h, w, stride in F32_GEOM:
                yield NchwCase(fl, n, F32_CIN[ks], h, w, cout, ks, stride, ks // 2, FORM_NAMES[i % 4], seed=1)
                i += 1
    yield NchwCase(fl, 2, 32, 6, 10, 64, 1, 1, 0, "all")       # K % 16 == 0
    yield NchwCase(fl, 2, 16, 9, 7, 130, 3, 2, 1, "all")       # K = 144, stride 2 on odd sizes


# ---- E. dh_stem_conv_nhwc -------------------------------------------------------------------------------------------------------
def stem_cases(dt, fl):
    i = 0
    for ks in (7, 3):
        for cout in (4, 64, 132):
            yield NchwCase(fl, 2, 3, 17 + 2 * i, 22, cout, ks, 2, ks // 2, "relu" if i % 2 else "affine", stem_dt=dt)
            i += 1
    yield NchwCase(fl, 3, 3, 13, 27, 64, 7, 2, 3, "relu", stem_dt=dt)           # 7 x 14 x 3 = 294 pixels: three pixel blocks


# ---- refusals ---------------------------------------------------------------------------------------------------------------
REFUSED = ((1000, 3),)                                        # (Cin, KS): magic() has no exact multiplier for k / 1000, k < 9000


def refusal_cases(dt):
    for cin, ks in REFUSED:
        yield ConvCase(dt, "int", 1, 5, 6, cin, 8, ks, 1, 1)


ROUTES_A = {                                                  # name: (cases(dt, fl), the routes they must reach)
    "ring_switch": (ring_switch_cases, {"tap_r8", "tap_r4", "tap_r3", "tap_r2"}),
    "tap": (tap_cases, {"tap_r8", "tap_r4", "tap_r3", "tap_r2"}),
    "generic": (generic_cases, {"generic_r8", "generic_r4"}),
    "big_tiles": (big_tile_cases, {"tap_t128", "generic_t128", "tap_r3", "tap_r4"}),
    "narrow": (narrow_cases, {"generic_c256", "tap_c256", "generic_r4", "dense_n64"}),
    "edges": (edge_cases, {"tap_r8", "generic_r8", "dense_r8", "tap_r4", "generic_r4", "dense_r4"}),
    "forms": (form_cases, {"tap_r8", "generic_r8", "dense_r8"}),
}
ROUTES_DUAL = {"dual_r8", "dual_r4", "dual_r3", "dual_r2", "dual_t128"}
ROUTES_F32 = {f"tm{tm}_k{ks}_{e}" for tm in (64, 128) for ks in (1, 3, 7) for e in ("vec", "px")}
ROUTES_STEM = {f"stem_tm{tm}_k{ks}" for tm in (64, 128) for ks in (7, 3)}
