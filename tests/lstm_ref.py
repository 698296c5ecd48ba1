"""What the LSTM step tests share (test_lstm_step_gpu.py, test_lstm_ref_cpu.py): one layer time step of nn.LSTM stated plainly in
fp64 (rnn_models.py:23-24, one step of :80 / :108), the cases of the three kernel routes with their operands and expected
results, and the restated route rules of the entry points.  Plain module, no GPU use: the cases are built on the CPU."""
import functools

import torch

from attn_ref import BF16, DT_IDS, DTYPES, F16, F32, F32_ATOL, Gate, err_ulps, ulps  # noqa: F401  (re-exported for the two test modules)

DT16 = [BF16, F16]
DT16_IDS = ["bf16", "f16"]
EXTRA_ROWS = 16                                               # sentinel rows behind every state / output array
VOCAB = 50
TOK_LD = 6                                                    # token columns: tok_pos 5 is the last one
X_OFF = 32                                                    # x_rows = wide[:, X_OFF:X_OFF + E] of a [rows, E + 64] buffer


def lstm_layer_ref(x, h_prev, c_prev, w, b, parent=None):
    """One layer step in fp64.  x [R, E]; h_prev / c_prev [S, Hh] or None (zero state); w [4 Hh, E + Hh] = [W_ih | W_hh] and
    b [4 Hh] = b_ih + b_hh in PyTorch's gate order i, f, g, o; parent [R] rows of the state arrays (None: row r reads row r).
    Returns (h', c'), each [R, Hh]."""
    x, w, b = x.double(), w.double(), b.double()
    rows, hh = x.shape[0], w.shape[0] // 4
    if h_prev is None:
        h0 = c0 = torch.zeros(rows, hh, dtype=torch.float64)
    else:
        idx = torch.arange(rows) if parent is None else parent.long()
        h0, c0 = h_prev.double()[idx], c_prev.double()[idx]
    gates = torch.cat([x, h0], 1) @ w.t() + b
    i, f, g, o = gates.split(hh, dim=1)
    c1 = torch.sigmoid(f) * c0 + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c1), c1


def interleave(w, b):
    """The layout lstm_layer_fused takes: row 4 u + g = gate g of hidden unit u."""
    hh = w.shape[0] // 4
    return w.view(4, hh, -1).permute(1, 0, 2).reshape(4 * hh, -1).contiguous(), b.view(4, hh).t().reshape(-1).contiguous()


def fused_workgroups(rows, hh):
    return -(-rows // 64) * -(-4 * hh // 64)


def fused_slabs(rows, hh):
    """The LDS ring depth dh_lstm_layer_fused (csrc/lstm_fused.hip) picks from its workgroup count."""
    blocks = fused_workgroups(rows, hh)
    return 2 if 768 < blocks <= 1280 else 3 if 512 < blocks <= 768 else 4


def wreg_supported(e, hh):
    return e % 64 == 0 and hh % 32 == 0 and e + hh in (768, 1024)


def wreg_mapping(hh):
    """lstm_wreg_kernel's block-index mapping: the XCD remap when tiles_n = 4 Hh / 128 is a multiple of 8."""
    return "remap" if (4 * hh // 128) % 8 == 0 else "plain"


@functools.lru_cache(maxsize=None)
def layer_weights(dt, e, hh, seed=0):
    """w [4 Hh, E + Hh] rounded to ``dt`` and b fp32, drawn so that no gate saturates."""
    g = torch.Generator().manual_seed(1000003 * seed + 131 * e + hh + (0 if dt == BF16 else 1 if dt == F16 else 2))
    w = (torch.randn(4 * hh, e + hh, generator=g) / (e + hh) ** 0.5).to(dt)
    b = 0.1 * torch.randn(4 * hh, generator=g)
    return w, b


@functools.lru_cache(maxsize=None)
def layer_weights_interleaved(dt, e, hh):
    return interleave(*layer_weights(dt, e, hh))


def draw_tokens(n, g):
    """[n, TOK_LD] token ids in range whose neighbouring columns differ on every row."""
    cols = [torch.randint(0, VOCAB, (n,), generator=g)]
    for _ in range(TOK_LD - 1):
        cols.append((cols[-1] + torch.randint(1, VOCAB, (n,), generator=g)) % VOCAB)
    return torch.stack(cols, 1).int()


def draw_parents(n, n_state, g):
    """[n] rows of an ``n_state``-row state array, none of them the row itself."""
    return ((torch.arange(n) + torch.randint(1, n_state, (n,), generator=g)) % n_state).int()


class LayerCase:
    """One dh_lstm_layer_fused / dh_lstm_layer_wreg call.  Compact row m is logical row rl = m * row_mult; the state arrays
    (h_prev, c_prev, h_next, c_next) hold ``rows * row_mult + EXTRA_ROWS`` rows and a parent may be any of them but rl itself.
    ``x_src``: "tokens" (x row = emb[tokens[rl, tok_pos]]) or "x_rows" (x row = x_rows[m // x_div], x_rows being columns
    X_OFF : X_OFF + E of a ``[rows, E + 64]`` buffer whose every row is drawn, so a kernel that ignored x_div would read other
    numbers, not other memory).  ``state``: "none" (zero state), "parent" (gathered through hparent) or "identity" (state
    given, hparent = None: row rl reads row rl)."""

    def __init__(self, dt, rows, row_mult, e, hh, x_src="tokens", state="parent", x_div=1, tok_pos=3):
        assert x_src in ("tokens", "x_rows") and state in ("none", "parent", "identity")
        self.dt, self.rows, self.row_mult, self.e, self.hh = dt, rows, row_mult, e, hh
        self.x_src, self.state, self.x_div, self.tok_pos = x_src, state, x_div, tok_pos
        self.rows_total = rows * row_mult
        self.n_state = self.rows_total + EXTRA_ROWS
        self.ldx, self.ld_out = e + 64, hh + 8
        self.w, self.b = layer_weights(dt, e, hh)
        self.w_il, self.b_il = layer_weights_interleaved(dt, e, hh)
        g = torch.Generator().manual_seed(7919 * rows + 31 * row_mult + e + 3 * hh + x_div + 17 * tok_pos)
        self.rl = torch.arange(rows) * row_mult
        self.emb = self.tokens = self.wide = self.h_prev = self.c_prev = self.hparent = None
        if x_src == "tokens":
            self.emb = torch.randn(VOCAB, e, generator=g).to(dt)
            self.tokens = draw_tokens(self.rows_total, g)
        else:
            self.wide = torch.randn(rows, self.ldx, generator=g).to(dt)
        if state != "none":
            self.h_prev = (0.5 * torch.randn(self.n_state, hh, generator=g)).to(dt)
            self.c_prev = torch.randn(self.n_state, hh, generator=g)
        if state == "parent":
            self.hparent = draw_parents(self.rows_total, self.n_state, g)
        self._want = None

    @property
    def x_rows(self):
        return None if self.wide is None else self.wide[:, X_OFF:X_OFF + self.e]

    def what(self):
        d = dict(rows=self.rows, row_mult=self.row_mult, e=self.e, hh=self.hh, x=self.x_src, state=self.state)
        d.update(dict(tok_pos=self.tok_pos) if self.x_src == "tokens" else dict(x_div=self.x_div))
        return d

    def perturbations(self):
        """The wrong readings this case can tell from the right one."""
        p = ["x_cols"]
        if self.state != "none":
            p.append("h_cols")
        if self.state == "parent":
            p.append("identity")
        if self.x_src == "tokens" and self.tok_pos > 0:
            p.append("tok_prev")
        return p

    def want(self, wrong=None):
        """(h', c') in fp64 at the compact rows.  ``wrong``: "x_cols" / "h_cols" zero the last 8 columns of that part of the
        operand, "identity" reads the state at rl instead of hparent[rl], "tok_prev" the token at tok_pos - 1."""
        if wrong is None and self._want is not None:
            return self._want
        if self.x_src == "tokens":
            x = self.emb[self.tokens[self.rl, self.tok_pos - (wrong == "tok_prev")].long()]
        else:
            x = self.x_rows[torch.arange(self.rows) // self.x_div]
        x, h_prev = x.double(), self.h_prev
        if wrong == "x_cols":
            x = x.clone()
            x[:, -8:] = 0
        if wrong == "h_cols":
            h_prev = h_prev.double().clone()
            h_prev[:, -8:] = 0
        parent = self.hparent[self.rl] if self.state == "parent" and wrong != "identity" else self.rl
        out = lstm_layer_ref(x, h_prev, self.c_prev, self.w, self.b, parent)
        if wrong is None:
            self._want = out
        return out


# ---- the cases of test_lstm_step_gpu.py ------------------------------------------------------------------------------------
DEPTH_TILES = ((64, 4), (65, 3), (96, 3), (97, 2), (160, 2), (161, 4))     # (row tiles, slabs) at E 64 / Hh 128: 8 column tiles
BENCH_POINTS = ((256, 512), (512, 512))                                     # 1,280 rows: 640 workgroups, 3 slabs
EDGE_ROWS = (1, 63, 64, 65, 130)
EDGE_SHAPES = ((8, 24), (8, 56), (72, 136), (64, 64), (256, 512))
GATHER_SHAPES = ((72, 136), (256, 512))
GATHER_ROWS = 37
WREG_SHAPES = ((256, 512), (512, 512), (512, 256), (768, 256), (128, 640), (384, 640))
WREG_ROWS = (1, 79, 80, 81, 161)
WREG_UNSUPPORTED = ((72, 696), (256, 496), (256, 256))


def fused_depth_cases(dt):
    for tiles, _ in DEPTH_TILES:
        yield LayerCase(dt, 64 * tiles - 7, 1, 64, 128)
    yield LayerCase(dt, 1280, 1, 256, 512, "tokens")
    yield LayerCase(dt, 1280, 1, 512, 512, "x_rows")


def fused_edge_cases(dt):
    for e, hh in EDGE_SHAPES:
        for rows in EDGE_ROWS:
            yield LayerCase(dt, rows, 1, e, hh, "x_rows" if rows % 2 else "tokens")


def gather_cases(dt, shapes=GATHER_SHAPES):
    for e, hh in shapes:
        for row_mult in (1, 5):
            for state in ("none", "parent", "identity"):
                for tok_pos in (0, 3, TOK_LD - 1):
                    yield LayerCase(dt, GATHER_ROWS, row_mult, e, hh, "tokens", state, tok_pos=tok_pos)
                for x_div in (1, 5):
                    yield LayerCase(dt, GATHER_ROWS, row_mult, e, hh, "x_rows", state, x_div=x_div)


def wreg_row_cases(dt):
    for e, hh in WREG_SHAPES:
        for rows in WREG_ROWS:
            for row_mult in (1, 3):
                yield LayerCase(dt, rows, row_mult, e, hh, "x_rows" if rows % 2 else "tokens")


def wreg_gather_cases(dt):
    return gather_cases(dt, WREG_SHAPES)


LAYER_CASE_SETS = {"fused_depth": fused_depth_cases, "fused_edges": fused_edge_cases, "fused_gather": gather_cases,
                   "wreg_rows": wreg_row_cases, "wreg_gather": wreg_gather_cases}


# ---- the unfused route: dh_lstm_prepare -> dh_linear -> dh_lstm_cell over a stack of layers ------------------------------------
UNFUSED_SHAPES = ((8, 8), (256, 512), (1032, 1032))           # fp32: 1032 > 1024 = 256 threads x 4 gives the second loop trip
UNFUSED_SHAPES_16 = UNFUSED_SHAPES + ((2056, 2056),)          # 16 bits: 2056 > 2048 = 256 threads x 8
F32X_SHAPES = ((256, 512, 1), (256, 512, 3), (64, 96, 3))     # (E, Hh, layers): E % 32 == 0 and Hh % 32 == 0
N_IMG = 3


class StepCase:
    """One dh_lstm_prepare call and the n_layers gate products and dh_lstm_cell calls behind it.  ``src`` "tokens": the step of a
    started sequence (state gathered through hparent); "image": the first step (x row = img_emb[rc // rows_per_img], zero
    state).  The state arrays hold ``rows_total = rows * row_mult + 4`` rows per layer, the last 4 never written."""

    def __init__(self, dt, n_layers, e, hh, src, rows_per_img, row_mult, tok_pos=2):
        assert src in ("tokens", "image")
        self.dt, self.n_layers, self.e, self.hh, self.src = dt, n_layers, e, hh, src
        self.rows_per_img, self.row_mult, self.tok_pos = rows_per_img, row_mult, tok_pos
        self.rows = N_IMG * rows_per_img
        self.rows_total = self.rows * row_mult + 4
        self.ld_out = hh + 8
        g = torch.Generator().manual_seed(104729 * n_layers + 7919 * rows_per_img + 31 * row_mult + e + 3 * hh)
        self.rl = torch.arange(self.rows) * row_mult
        self.emb = self.tokens = self.img = self.h_prev = self.c_prev = self.hparent = None
        if src == "tokens":
            self.emb = torch.randn(VOCAB, e, generator=g).to(dt)
            self.tokens = draw_tokens(self.rows_total, g)
            self.h_prev = (0.5 * torch.randn(n_layers, self.rows_total, hh, generator=g)).to(dt)
            self.c_prev = torch.randn(n_layers, self.rows_total, hh, generator=g)
            self.hparent = draw_parents(self.rows_total, self.rows_total, g)
        else:
            self.img = torch.randn(N_IMG, e, generator=g).to(dt)

    @property
    def layers(self):
        """(w, b) per layer: [4 Hh, E + Hh], then [4 Hh, 2 Hh]."""
        return [layer_weights(self.dt, self.e if l == 0 else self.hh, self.hh, seed=l + 1) for l in range(self.n_layers)]

    def what(self):
        return dict(layers=self.n_layers, e=self.e, hh=self.hh, src=self.src, rows_per_img=self.rows_per_img, row_mult=self.row_mult)

    def x0(self):
        """Layer 0's x rows [rows, E], in the case's type."""
        if self.src == "tokens":
            return self.emb[self.tokens[self.rl, self.tok_pos].long()]
        return self.img[torch.arange(self.rows) // self.rows_per_img]

    def parent(self):
        return None if self.hparent is None else self.hparent[self.rl].long()

    def want_layer(self, l, x):
        """(h', c') of layer l in fp64 for the x rows it was given (layer >= 1: the rows the layer below stored, in its type)."""
        w, b = self.layers[l]
        started = self.h_prev is not None
        return lstm_layer_ref(x, self.h_prev[l] if started else None, self.c_prev[l] if started else None, w, b, self.parent())


def unfused_cases(dt):
    for e, hh in (UNFUSED_SHAPES if dt == F32 else UNFUSED_SHAPES_16):
        for n_layers in (1, 3):
            for src in ("tokens", "image"):
                for rows_per_img, row_mult in ((1, 3), (4, 1)) if n_layers == 3 else ((1, 1), (4, 3)):
                    yield StepCase(dt, n_layers, e, hh, src, rows_per_img, row_mult)


class AbsGate:
    """The fp32 outputs' gate: worst |got - want| over a test's cases against ``table[name][dt]``, which itself may not exceed
    F32_ATOL; ``check`` prints the worst (the numbers behind the ``ABS_GATE`` tables)."""

    def __init__(self, name, dt, table, kind="c"):
        self.name, self.dt, self.table, self.kind, self.worst, self.where, self.n = name, dt, table, kind, 0.0, None, 0

    def add(self, got, want, what):
        self.n += 1
        e = float((got.double().cpu() - want.double()).abs().max())
        if not e <= self.worst:                               # a NaN is the worst
            self.worst, self.where = e, what

    def check(self):
        bound = self.table[self.name][self.dt]
        print(f"[{self.name}] {self.dt} {self.kind}: worst {self.worst:.3e} abs at {self.where} ({self.n} cases)")
        assert bound <= F32_ATOL, (self.name, self.dt, bound)
        assert self.worst <= bound, (self.name, self.dt, self.kind, self.worst, self.where)
