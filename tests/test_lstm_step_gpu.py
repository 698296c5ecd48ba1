"""The LSTM layer time step (what ``generate()`` of the LSTM decoder runs) on every kernel route, shape edge and type, against
the plain fp64 statement of the step (lstm_ref.lstm_layer_ref) on the same operands -- rounded to the 16-bit type first for
bf16 / fp16.  The cases and their reference are in lstm_ref.py; tests/test_lstm_ref_cpu.py checks the reference against
torch.nn.LSTM and, from the reference alone, that in every case a dropped operand chunk, an ignored beam parent or the
neighbouring token position moves every row's c' by more than 100 x the gate.

  fused    dh_lstm_layer_fused (csrc/lstm_fused.hip): 64 x 64 tiles, an LDS ring of 4 / 3 / 2 slabs by workgroup count
  wreg     dh_lstm_layer_wreg (csrc/lstm_wreg.hip): gate weights in registers, K = 768 | 1024, two block-index mappings;
           promised bit-identical to ``fused``
  unfused  dh_lstm_prepare -> dh_linear -> dh_lstm_cell (csrc/lstm.hip), fp32 and 16 bits; dh_lstm_prepare_f32x /
           dh_lstm_cell_f32x are the same two kernels with the fp16 planes of the split-operand GEMM as a second output

Every call writes into sentinel-filled buffers with spare rows and a row stride wider than Hh; whatever a logical row / column
does not address must keep the sentinel, and h_out must equal h_next at the logical rows bit for bit.

Gates.  h in 16 bits: ulps at max(|want|, 2^-6) (attn_ref.ulps), one entry per (route, type); c, and every fp32 output: absolute
error, never above F32_ATOL = 2e-5.  Both tables hold 1.25 x the worst error measured on an MI355X over every case of the route
(the 1.25 covers another, equally valid accumulation order); every route measures a little over half an ulp, an fp32 result
rounded once, and c within 1.9e-6 of fp64.  Every test prints its worst error per (route, type).  Gathers and
wreg-against-fused: torch.equal.  A stack of layers is compared
layer by layer: the reference of layer l takes the rows the layer below stored (themselves just compared), since a reference
that rounded its own h would differ from the kernel's by a whole ulp of the type wherever the two round apart."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import lstm_ref as L  # noqa: E402
from lstm_ref import BF16, DT16, DT16_IDS, F16, F32  # noqa: E402

# 1.25 x the worst error measured on an MI355X over every case of the route; check() prints it.  h' in 16 bits: ulps at
# max(|want|, 2^-6).  c' and every fp32 output: absolute, and never above F32_ATOL (AbsGate.check asserts that too).
ULP_GATE = {
    "fused": {BF16: 1.25 * 0.5005, F16: 1.25 * 0.5056},
    "wreg": {BF16: 1.25 * 0.5005, F16: 1.25 * 0.5071},
    "unfused": {BF16: 1.25 * 0.5006, F16: 1.25 * 0.5103},
}
ABS_GATE = {
    "fused": {BF16: 1.25 * 9.105e-07, F16: 1.25 * 8.209e-07},
    "wreg": {BF16: 1.25 * 8.866e-07, F16: 1.25 * 7.434e-07},
    "unfused": {F32: 1.25 * 1.820e-06, BF16: 1.25 * 1.031e-06, F16: 1.25 * 1.027e-06},
    "unfused_h": {F32: 1.25 * 9.582e-07},
}
SENTINEL = 768.0                                              # exact in every type, never a state value


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
    print(f"[test_lstm_step_gpu] module wall time {time.time() - t0:.1f} s")


def full(shape, dt):
    return torch.full(shape, SENTINEL, dtype=dt, device="cuda")


def kept(t):
    return bool((t == SENTINEL).all())


def dev(x):
    return None if x is None else x.cuda()


class RouteGates:
    """The h gate (ulps) and the c gate (absolute) of one (route, type)."""

    def __init__(self, route, dt):
        self.h = L.Gate(route, dt, ULP_GATE) if dt != F32 else L.AbsGate(route + "_h", dt, ABS_GATE, "h")
        self.c = L.AbsGate(route, dt, ABS_GATE)

    def add(self, h, c, want, what):
        self.h.add(h, want[0], what)
        self.c.add(c, want[1], what)

    def check(self):
        failed = []
        for g in (self.h, self.c):
            try:
                g.check()
            except AssertionError as e:
                failed.append(e)
        assert not failed, failed


def run_layer(hip, c, route, weights):
    """One call of ``route`` on case ``c``: (h', c') at the compact rows, after the sentinel and h_out checks."""
    fn = hip.lstm_layer_fused if route == "fused" else hip.lstm_layer_wreg
    h_next, c_next = full((c.n_state, c.hh), c.dt), full((c.n_state, c.hh), F32)
    h_out = full((c.rows + L.EXTRA_ROWS, c.ld_out), c.dt)
    wide = dev(c.wide)
    x_rows = None if wide is None else wide[:, L.X_OFF:L.X_OFF + c.e]
    assert x_rows is None or (x_rows.stride(0) == c.ldx and x_rows.data_ptr() % 16 == 0)
    fn(x_rows, c.x_div, dev(c.emb), dev(c.tokens), c.tok_pos, dev(c.h_prev), dev(c.c_prev), dev(c.hparent), h_next, c_next,
       h_out[:c.rows, :c.hh], weights, dev(c.b_il), c.rows, c.row_mult, c.e, c.hh)
    rl = c.rl.cuda()
    other = torch.ones(c.n_state, dtype=torch.bool, device="cuda")
    other[rl] = False
    assert kept(h_next[other]) and kept(c_next[other]), c.what()
    assert kept(h_out[c.rows:]) and kept(h_out[:c.rows, c.hh:]), c.what()
    assert torch.equal(h_out[:c.rows, :c.hh], h_next[rl]), c.what()
    return h_next[rl], c_next[rl]


_weights = {}


def fused_weights(c):
    """The gate-interleaved weights on the device, once per shape and type."""
    key = (c.dt, c.e, c.hh)
    if key not in _weights:
        _weights[key] = c.w_il.cuda()
    return _weights[key]


def wreg_weights(hip, c):
    key = (c.dt, c.e, c.hh, "packed")
    if key not in _weights:
        _weights[key] = hip.pack_mfma_fragments(fused_weights(c))
    return _weights[key]


# ---- a, b, c: the tile kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_fused_every_ring_depth(hip, dt):
    """E 64 / Hh 128 (8 column tiles) at the row counts on both sides of each switch of the ring depth, the last row tile
    partial; and the benchmark's own two points (640 workgroups: 3 slabs)."""
    gates, reached = RouteGates("fused", dt), set()
    for c in L.fused_depth_cases(dt):
        reached.add((L.fused_workgroups(c.rows, c.hh), L.fused_slabs(c.rows, c.hh)))
        h, cc = run_layer(hip, c, "fused", fused_weights(c))
        gates.add(h, cc, c.want(), c.what())
    assert reached == {(512, 4), (520, 3), (768, 3), (776, 2), (1280, 2), (1288, 4), (640, 3)}, sorted(reached)
    gates.check()


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_fused_shape_edges(hip, dt):
    """K 32 (one partial slab) / 64 (exactly one) / 128 (two against a 4-deep ring) / 208 (a slab straddling x | h, K tail 16),
    N 96 / 544 (a partial last column tile), and the decode shape; 1 .. 130 rows."""
    gates, seen = RouteGates("fused", dt), set()
    for c in L.fused_edge_cases(dt):
        seen.add((c.e + c.hh, 4 * c.hh % 64 != 0))
        h, cc = run_layer(hip, c, "fused", fused_weights(c))
        gates.add(h, cc, c.want(), c.what())
    assert seen == {(32, True), (64, True), (208, True), (128, False), (768, False)}
    gates.check()


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_fused_gather_forms(hip, dt):
    """Tokens at the first, a middle and the last position; x rows out of a wider buffer, one per row or one per 5 rows;
    row_mult 1 and 5; no state, state through hparent, state without hparent."""
    gates, forms = RouteGates("fused", dt), set()
    for c in L.gather_cases(dt):
        forms.add((c.x_src, c.tok_pos if c.x_src == "tokens" else c.x_div, c.row_mult, c.state))
        h, cc = run_layer(hip, c, "fused", fused_weights(c))
        gates.add(h, cc, c.want(), c.what())
    assert len(forms) == 30
    gates.check()


# ---- d: the register-stationary kernel --------------------------------------------------------------------------------------------
def test_wreg_supported(hip):
    for e, hh in L.WREG_SHAPES:
        assert hip.lstm_layer_wreg_supported(e, hh) and L.wreg_supported(e, hh), (e, hh)
    for e, hh in L.WREG_UNSUPPORTED:
        assert not hip.lstm_layer_wreg_supported(e, hh) and not L.wreg_supported(e, hh), (e, hh)


@pytest.mark.parametrize("cases", ["rows", "gather"])
@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_wreg(hip, dt, cases):
    """K 768 and 1024 under both block-index mappings (tiles_n 8 / 16: XCD remap; 20: plain), against fp64 and bit for bit
    against the tile kernel.  ``rows``: 1 .. 161 rows (80-row blocks, mostly clamped rows at 1) x row_mult 1 / 3; ``gather``:
    the forms of test_fused_gather_forms at every shape."""
    gates, reached = RouteGates("wreg", dt), set()
    for c in (L.wreg_row_cases if cases == "rows" else L.wreg_gather_cases)(dt):
        reached.add((c.e + c.hh, L.wreg_mapping(c.hh)))
        h, cc = run_layer(hip, c, "wreg", wreg_weights(hip, c))
        gates.add(h, cc, c.want(), c.what())
        h_f, c_f = run_layer(hip, c, "fused", fused_weights(c))
        assert torch.equal(h, h_f) and torch.equal(cc, c_f), c.what()
    assert reached == {(768, "remap"), (1024, "remap"), (768, "plain"), (1024, "plain")}
    gates.check()


# ---- e, f: prepare -> gate product -> cell ---------------------------------------------------------------------------------------
class StepBuffers:
    """The sentinel-filled outputs of one StepCase, each with two spare rows (the state: the case's own 4) behind it."""

    def __init__(self, c):
        dt, rows, nl, e, hh = c.dt, c.rows, c.n_layers, c.e, c.hh
        self.xcat0 = full((rows + 2, e + hh), dt)
        self.xcatl = full(((nl - 1) * rows + 2, 2 * hh), dt)
        self.c_cur = full((nl * rows + 2, hh), F32)
        self.h_new, self.c_new = full((nl, c.rows_total, hh), dt), full((nl, c.rows_total, hh), F32)
        self.top = full((rows + 2, c.ld_out), dt)

    def below(self, c, l):
        """Layer l >= 1's operand rows [rows, 2 Hh]: x half from the cell below, h half from prepare."""
        return self.xcatl[(l - 1) * c.rows:l * c.rows]

    def dst(self, c, l):
        """Where layer l's cell stores the compact h rows, and its row stride."""
        if l + 1 < c.n_layers:
            return self.below(c, l + 1)[:, :c.hh], 2 * c.hh
        return self.top[:c.rows, :c.hh], c.ld_out


def check_prepared(c, b):
    """The gathers, bit for bit; everything prepare does not address keeps the sentinel."""
    rows, nl, e, hh = c.rows, c.n_layers, c.e, c.hh
    par = c.parent()
    assert torch.equal(b.xcat0[:rows, :e].cpu(), c.x0()), c.what()
    zero = torch.zeros(rows, hh)
    for l in range(nl):
        h_part = b.xcat0[:rows, e:] if l == 0 else b.below(c, l)[:, hh:]
        assert torch.equal(h_part.cpu(), c.h_prev[l][par] if par is not None else zero.to(c.dt)), (c.what(), l)
        assert torch.equal(b.c_cur[l * rows:(l + 1) * rows].cpu(), c.c_prev[l][par] if par is not None else zero), (c.what(), l)
        assert l == 0 or kept(b.below(c, l)[:, :hh]), (c.what(), l)
    assert kept(b.xcat0[rows:]) and kept(b.xcatl[(nl - 1) * rows:]) and kept(b.c_cur[nl * rows:]), c.what()


def check_cell(c, b, l, gates):
    """Layer l's cell outputs against fp64 for the operand rows it was given; stray writes; h_out == h_new."""
    rows, hh = c.rows, c.hh
    x = c.x0() if l == 0 else b.below(c, l)[:, :hh].cpu()
    dst, _ = b.dst(c, l)
    rl = c.rl.cuda()
    other = torch.ones(c.rows_total, dtype=torch.bool, device="cuda")
    other[rl] = False
    assert kept(b.h_new[l][other]) and kept(b.c_new[l][other]), (c.what(), l)
    assert torch.equal(dst, b.h_new[l][rl]), (c.what(), l)
    gates.add(b.h_new[l][rl], b.c_new[l][rl], c.want_layer(l, x), dict(c.what(), layer=l))


_step_weights = {}


def step_weights(c, l):
    key = (c.dt, c.e if l == 0 else c.hh, c.hh, l)
    if key not in _step_weights:
        _step_weights[key] = tuple(t.cuda() for t in c.layers[l])
    return _step_weights[key]


def step_operands(c):
    return dict(emb=dev(c.emb), img=dev(c.img), tokens=dev(c.tokens), hparent=dev(c.hparent), h_prev=dev(c.h_prev), c_prev=dev(c.c_prev))


@pytest.mark.parametrize("dt", L.DTYPES, ids=L.DT_IDS)
def test_unfused_step(hip, dt):
    """1 and 3 layers; E / Hh from one vector per block (8) to a second trip of the 256-thread vector loops (1032 in fp32,
    2056 in 16 bits); token steps with the state gathered through hparent and image steps (x row = img_emb[rc // rows_per_img],
    zero state) at 1 and 4 rows per image, row_mult 1 and 3."""
    gates, seen = RouteGates("unfused", dt), set()
    for c in L.unfused_cases(dt):
        seen.add((c.src, c.rows_per_img, c.row_mult))
        b, d = StepBuffers(c), step_operands(c)
        hip.lstm_prepare(d["emb"], d["img"], d["tokens"], c.tok_pos, d["hparent"], d["h_prev"], d["c_prev"], b.xcat0, b.xcatl, b.c_cur,
                         c.rows, c.rows_per_img, c.row_mult, c.rows_total, c.n_layers, c.e, c.hh)
        check_prepared(c, b)
        for l in range(c.n_layers):
            w, bias = step_weights(c, l)
            g = hip.linear(b.xcat0[:c.rows] if l == 0 else b.below(c, l), w, bias, out_dtype=torch.float32)
            dst, ld = b.dst(c, l)
            hip.lstm_cell(g, b.c_cur[l * c.rows:(l + 1) * c.rows], b.h_new[l], b.c_new[l], dst, ld, c.rows, c.row_mult, c.hh)
            check_cell(c, b, l, gates)
        assert kept(b.top[c.rows:]) and kept(b.top[:c.rows, c.hh:]) and kept(b.xcatl[(c.n_layers - 1) * c.rows:]), c.what()
    assert seen == {(s, r, m) for s in ("tokens", "image") for r in (1, 4) for m in (1, 3)}
    gates.check()


GUARD = 64                                                    # sentinel elements before and behind each planes array


def xcatl_planes_at(c, l):
    """Element offset in xcatl_planes [n_layers - 1][2][rows][2 Hh] of the planes of layer l's (l >= 1) operand rows."""
    return (l - 1) * 2 * c.rows * 2 * c.hh


@pytest.mark.parametrize("src", ["tokens", "image"])
@pytest.mark.parametrize("e,hh,n_layers", L.F32X_SHAPES)
def test_f32x_producers(hip, e, hh, n_layers, src):
    """dh_lstm_prepare_f32x / dh_lstm_cell_f32x: the fp32 outputs equal dh_lstm_prepare / dh_lstm_cell bit for bit, every plane
    equals split_act of the fp32 rows at the documented offsets (xcat0 planes [2][rows][E + Hh], xcatl planes
    [n_layers - 1][2][rows][2 Hh], top planes [2][rows][Hh]; lo one plane behind hi), the memory around the planes is
    untouched and the range flag stays down."""
    from deephumor_amd import f32xp
    c = L.StepCase(F32, n_layers, e, hh, src, 4, 3 if src == "image" else 1)
    rows, nl = c.rows, n_layers
    d = step_operands(c)
    plain, x = StepBuffers(c), StepBuffers(c)
    n0, nl_, nt = 2 * rows * (e + hh), (nl - 1) * 2 * rows * 2 * hh, 2 * rows * hh
    p0, pl, pt = (torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float16, device="cuda") for n in (n0, nl_, nt))
    hip.f32x_take_overflow()                                  # lowers a flag an earlier test may have left up
    hip.lstm_prepare(d["emb"], d["img"], d["tokens"], c.tok_pos, d["hparent"], d["h_prev"], d["c_prev"], plain.xcat0, plain.xcatl,
                     plain.c_cur, rows, c.rows_per_img, c.row_mult, c.rows_total, nl, e, hh)
    f32xp.lstm_prepare_f32x(d["emb"], d["img"], d["tokens"], c.tok_pos, d["hparent"], d["h_prev"], d["c_prev"], x.xcat0, x.xcatl,
                            x.c_cur, p0[GUARD:], pl[GUARD:] if nl > 1 else None, rows, c.rows_per_img, c.row_mult, c.rows_total, nl, e, hh)
    check_prepared(c, x)
    for name in ("xcat0", "xcatl", "c_cur"):
        assert torch.equal(getattr(x, name), getattr(plain, name)), name
    for l in range(nl):
        w, bias = step_weights(c, l)
        g = hip.linear(plain.xcat0[:rows] if l == 0 else plain.below(c, l), w, bias, out_dtype=torch.float32)
        dst, ld = plain.dst(c, l)
        hip.lstm_cell(g, plain.c_cur[l * rows:(l + 1) * rows], plain.h_new[l], plain.c_new[l], dst, ld, rows, c.row_mult, hh)
        last = l + 1 == nl
        dst, ld = x.dst(c, l)
        planes = pt[GUARD:] if last else pl[GUARD + xcatl_planes_at(c, l + 1):]       # the x half of the layer above
        f32xp.lstm_cell_f32x(g, x.c_cur[l * rows:(l + 1) * rows], x.h_new[l], x.c_new[l], dst, ld, planes, rows * (hh if last else 2 * hh),
                             hh if last else 2 * hh, rows, c.row_mult, hh)
    for name in ("xcatl", "h_new", "c_new", "top"):
        assert torch.equal(getattr(x, name), getattr(plain, name)), name
    assert torch.equal(p0[GUARD:GUARD + n0].view(2, rows, e + hh), f32xp.split_act(x.xcat0[:rows]))
    for l in range(1, nl):
        got = pl[GUARD + xcatl_planes_at(c, l):GUARD + xcatl_planes_at(c, l + 1)].view(2, rows, 2 * hh)
        assert torch.equal(got, f32xp.split_act(x.below(c, l))), l
    assert torch.equal(pt[GUARD:GUARD + nt].view(2, rows, hh), f32xp.split_act(x.top[:rows, :hh]))
    for p, n in ((p0, n0), (pl, nl_), (pt, nt)):
        assert kept(p[:GUARD]) and kept(p[GUARD + n:])
    assert hip.f32x_take_overflow() is False


def test_f32x_prepare_raises_the_range_flag(hip):
    """One embedding element beyond the fp16 range: the call returns normally and the range flag is up afterwards (the guard the
    caller repeats the step on the exact path for)."""
    from deephumor_amd import f32xp
    c = L.StepCase(F32, 1, 64, 96, "tokens", 4, 1)
    emb = c.emb.clone()
    emb[int(c.tokens[int(c.rl[5]), c.tok_pos]), 17] = 70000.0
    b, d = StepBuffers(c), step_operands(c)
    p0 = torch.full((2 * c.rows * (c.e + c.hh),), SENTINEL, dtype=torch.float16, device="cuda")
    hip.f32x_take_overflow()
    f32xp.lstm_prepare_f32x(emb.cuda(), None, d["tokens"], c.tok_pos, d["hparent"], d["h_prev"], d["c_prev"], b.xcat0, None, b.c_cur, p0,
                            None, c.rows, c.rows_per_img, c.row_mult, c.rows_total, 1, c.e, c.hh)
    assert float(b.xcat0[5, 17]) == 70000.0
    assert hip.f32x_take_overflow() is True
    assert hip.f32x_take_overflow() is False                  # taken: down again
