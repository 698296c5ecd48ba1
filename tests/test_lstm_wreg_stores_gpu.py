"""dh_lstm_layer_wreg (csrc/lstm_wreg.hip) stores its 80-row x 32-unit output tile through LDS as whole row segments: 128-byte
rows of c_next, 64-byte rows of h_next and h_out, 16 bytes per lane.  Every case here runs the step on the tile kernel
(dh_lstm_layer_fused, the other side of the existing LSTM route tests) and on the register-stationary kernel into
sentinel-filled buffers and compares the three WHOLE buffers byte for byte -- no tolerance -- and then checks on the
register-stationary side that the sentinel is intact wherever the step addresses nothing: state rows that are no logical row
(rows >= rows * row_mult, and with row_mult 5 the four rows between two logical ones), h_out rows >= rows and h_out columns
Hh .. ld_out.

Cases: the full cross product of
  (E, Hh)    (256, 512) and (512, 512): K = 768 (tile behind the operand slabs, one barrier) and 1,024 (tile over them, two)
  type       bf16, fp16
  rows       1, 5 (one partial 16-row tile), 79, 80, 81 (one 80-row block and one row either side), 165 (three blocks, 5 rows
             in the last)
  row_mult   1, 5
  ld_out     Hh, 3 Hh
  state      none (zero state), identity (hparent = NULL), a random permutation of the state rows, every row the same parent
  input      tokens + embedding table; x_rows (columns of a wider buffer) with x_div 1 and 5
one test per (shape, type): 288 cases of two launches each, operands drawn once per test on the device.

A model-level decode (8 images x beam 5; option lstm_wreg_min_rows = 1 so that 40 rows take the register-stationary step)
returns the same captions with option decode_wreg = 0 and with the tile kernel (option lstm_wreg = 0)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 768.0                                              # exact in every type, never a state value
SHAPES = ((256, 512), (512, 512))
DTYPES = (torch.bfloat16, torch.float16)
ROWS = (1, 5, 79, 80, 81, 165)
ROW_MULTS = (1, 5)
STATES = ("none", "identity", "permutation", "same")
INPUTS = (("tokens", 1), ("x_rows", 1), ("x_rows", 5))
EXTRA_ROWS = 16                                               # sentinel rows behind every state / output array
VOCAB, TOK_LD, TOK_POS, X_OFF = 50, 6, 3, 32
N_STATE = max(ROWS) * max(ROW_MULTS) + EXTRA_ROWS


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def kept(t):
    return bool((t == SENTINEL).all())


class Operands:
    """What every case of one (shape, type) reads: drawn once, on the device."""

    def __init__(self, hip, e, hh, dt):
        g = torch.Generator(device="cuda").manual_seed(131 * e + hh + (dt == torch.float16))
        rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
        self.e, self.hh, self.dt = e, hh, dt
        self.w_il = (rnd(4 * hh, e + hh) / (e + hh) ** 0.5).to(dt)
        self.w_pk = hip.pack_mfma_fragments(self.w_il)
        self.b_il = 0.1 * rnd(4 * hh)
        self.emb = rnd(VOCAB, e).to(dt)
        self.tokens = torch.randint(0, VOCAB, (N_STATE, TOK_LD), generator=g, device="cuda", dtype=torch.int32)
        self.wide = rnd(max(ROWS), e + 64).to(dt)             # x_rows = columns X_OFF : X_OFF + E
        self.h_prev = (0.5 * rnd(N_STATE, hh)).to(dt)
        self.c_prev = rnd(N_STATE, hh)
        self.perm = torch.randperm(N_STATE, generator=g, device="cuda").int()
        self.same = torch.full((N_STATE,), 7, dtype=torch.int32, device="cuda")


def run(fn, weights, o, rows, row_mult, ld_out, state, x_src, x_div):
    n_state = rows * row_mult + EXTRA_ROWS
    h_next = torch.full((n_state, o.hh), SENTINEL, dtype=o.dt, device="cuda")
    c_next = torch.full((n_state, o.hh), SENTINEL, dtype=torch.float32, device="cuda")
    h_out = torch.full((rows + EXTRA_ROWS, ld_out), SENTINEL, dtype=o.dt, device="cuda")
    tok = x_src == "tokens"
    x_rows = None if tok else o.wide[:, X_OFF:X_OFF + o.e]
    started = state != "none"
    # parents are rows of the n_state-row state arrays of THIS case
    hparent = {"none": None, "identity": None, "permutation": o.perm[o.perm < n_state][:rows * row_mult].contiguous(),
               "same": o.same[:rows * row_mult]}[state]
    fn(x_rows, x_div, o.emb if tok else None, o.tokens if tok else None, TOK_POS, o.h_prev[:n_state] if started else None,
       o.c_prev[:n_state] if started else None, hparent, h_next, c_next, h_out[:rows, :o.hh], weights, o.b_il, rows, row_mult, o.e, o.hh)
    return h_next, c_next, h_out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("e,hh", SHAPES)
def test_wreg_row_segment_stores(hip, e, hh, dt):
    assert hip.lstm_layer_wreg_supported(e, hh)
    o = Operands(hip, e, hh, dt)
    n = 0
    for rows, row_mult, ld_mult, state, (x_src, x_div) in itertools.product(ROWS, ROW_MULTS, (1, 3), STATES, INPUTS):
        what = dict(e=e, hh=hh, rows=rows, row_mult=row_mult, ld_out=ld_mult * hh, state=state, x=x_src, x_div=x_div)
        args = (o, rows, row_mult, ld_mult * hh, state, x_src, x_div)
        want = run(hip.lstm_layer_fused, o.w_il, *args)
        got = run(hip.lstm_layer_wreg, o.w_pk, *args)
        for name, g_, w_ in zip(("h_next", "c_next", "h_out"), got, want):
            assert torch.equal(bits(g_), bits(w_)), (name, what)
        h_next, c_next, h_out = got
        other = torch.ones(h_next.shape[0], dtype=torch.bool, device="cuda")
        other[torch.arange(rows, device="cuda") * row_mult] = False
        assert int(other.sum()) == rows * (row_mult - 1) + EXTRA_ROWS
        assert kept(h_next[other]) and kept(c_next[other]), what
        assert kept(h_out[rows:]) and kept(h_out[:rows, hh:]), what
        assert not bool((h_out[:rows, :hh] == SENTINEL).any()) and not bool((c_next[~other] == SENTINEL).any()), what
        assert torch.equal(bits(h_out[:rows, :hh]), bits(h_next[~other])), what
        n += 1
    assert n == 288


@pytest.mark.parametrize("settings", [dict(search="beam"), dict(top_k=5, seed=3)], ids=["greedy", "sampled"])
def test_decode_same_captions_on_both_lstm_steps(hip, settings):
    """CaptioningLSTM (E 256, Hh 512, 3 layers: K = 768 for the first layer, 1,024 above it), 8 images x beam 5.  ``greedy``: the
    deterministic search (generate_batch takes no top_k below beam_size, so top_k = 1 is not available at beam 5: search="beam" keeps
    the 5 most likely continuations, no noise); ``sampled``: the seeded stochastic search at the smallest top_k."""
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    model = M.CaptioningLSTM(1000, hidden_size=512).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=2468))
    model = model.bfloat16().cuda()
    imgs = synth_images(8, seed=13).cuda()
    with torch.no_grad(), hip.option_scope(lstm_wreg_min_rows=1):
        t1, l1 = model.generate_batch(imgs, max_len=10, beam_size=5, **settings)
        with hip.option_scope(decode_wreg=0):
            t2, l2 = model.generate_batch(imgs, max_len=10, beam_size=5, **settings)
        with hip.option_scope(decode_wreg=0, lstm_wreg=0):
            t3, l3 = model.generate_batch(imgs, max_len=10, beam_size=5, **settings)
    assert torch.equal(t1, t2) and torch.equal(l1, l2)
    assert torch.equal(t1, t3) and torch.equal(l1, l3)
