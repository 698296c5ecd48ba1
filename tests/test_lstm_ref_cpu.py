"""The LSTM step tests' own reference and inputs (lstm_ref.py), checked without a GPU: the fp64 layer step against
torch.nn.LSTM, the gate-interleaved layout, the input rules of every case, and the sensitivity condition of every LayerCase of
test_lstm_step_gpu.py -- a kernel that dropped the last operand chunk of the x or the h part, ignored the beam parent or read
the neighbouring token position would be seen on every row."""
import pytest
import torch

import lstm_ref as L
from lstm_ref import BF16, DT16, DT16_IDS

SENSITIVITY = 100                                             # x F32_ATOL, which no c gate of test_lstm_step_gpu.py may exceed


@pytest.mark.parametrize("n_layers", [1, 3])
def test_layer_ref_stacked_equals_nn_lstm(n_layers):
    """3 consecutive steps of nn.LSTM in fp64, the state rows of the middle one permuted by a parent gather."""
    e, hh, rows = 24, 40, 7
    g = torch.Generator().manual_seed(n_layers)
    lstm = torch.nn.LSTM(e, hh, n_layers, batch_first=True).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    weights = [(torch.cat([getattr(lstm, f"weight_ih_l{l}"), getattr(lstm, f"weight_hh_l{l}")], 1).detach(),
                (getattr(lstm, f"bias_ih_l{l}") + getattr(lstm, f"bias_hh_l{l}")).detach()) for l in range(n_layers)]
    h = c = None                                              # [layers, rows, Hh]; None: zero state
    parents = [None, torch.tensor([3, 0, 6, 6, 1, 2, 4]), None]
    for step in range(3):
        x = torch.randn(rows, e, generator=g, dtype=torch.float64)
        parent = parents[step]
        with torch.no_grad():
            state = None if h is None else (h, c) if parent is None else (h[:, parent].contiguous(), c[:, parent].contiguous())
            out, (hn, cn) = lstm(x[:, None], state)
        mine_h, mine_c, below = [], [], x
        for l, (w, b) in enumerate(weights):
            h1, c1 = L.lstm_layer_ref(below, None if h is None else h[l], None if h is None else c[l], w, b, parent)
            mine_h.append(h1)
            mine_c.append(c1)
            below = h1
        assert float((torch.stack(mine_h) - hn).abs().max()) < 1e-13 and float((torch.stack(mine_c) - cn).abs().max()) < 1e-13
        assert float((below - out[:, 0]).abs().max()) < 1e-13
        h, c = hn, cn


def test_interleaved_layout():
    """Row 4 u + g of the interleaved weights is gate g of hidden unit u."""
    w, b = L.layer_weights(BF16, 8, 24)
    w_il, b_il = L.interleave(w, b)
    x = torch.randn(5, 32, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    gates, gates_il = x @ w.double().t() + b.double(), x @ w_il.double().t() + b_il.double()
    assert torch.equal(gates_il.view(5, 24, 4).permute(0, 2, 1).reshape(5, 96), gates)


def all_layer_cases(dt):
    for cases in L.LAYER_CASE_SETS.values():
        yield from cases(dt)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_case_inputs_keep_the_rules(dt):
    """In range, hparent a derangement at the logical rows, neighbouring token positions different, nothing saturated."""
    n = 0
    for c in all_layer_cases(dt):
        n += 1
        if c.hparent is not None:
            hp = c.hparent.long()
            assert int(hp.min()) >= 0 and int(hp.max()) < c.n_state and bool((hp[c.rl] != c.rl).all()), c.what()
        if c.tokens is not None:
            assert int(c.tokens.min()) >= 0 and int(c.tokens.max()) < L.VOCAB and c.tok_pos < c.tokens.shape[1], c.what()
            assert bool((c.tokens[:, 1:] != c.tokens[:, :-1]).all()), c.what()
        else:
            assert c.x_rows.shape == (c.rows, c.e) and c.x_rows.stride(0) == c.ldx > c.e, c.what()
        h, cc = c.want()
        assert float(h.abs().max()) < 0.999 and float(cc.abs().max()) < 8, c.what()
    for c in L.unfused_cases(dt):
        assert int(c.hparent.min() if c.hparent is not None else 0) >= 0 and c.rows <= 12
        if c.hparent is not None:
            assert int(c.hparent.max()) < c.rows_total and bool((c.hparent[c.rl].long() != c.rl).all())
    assert n == 8 + 25 + 60 + 60 + 180


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_a_wrong_reading_is_visible(dt):
    """Each wrong reading a case can tell apart moves c' of EVERY logical row (maximum over the hidden units) by more than
    100 x F32_ATOL, the ceiling of every route's c gate (AbsGate.check asserts the ceiling)."""
    least = {}
    bound = SENSITIVITY * L.F32_ATOL
    for cases in L.LAYER_CASE_SETS.values():
        for c in cases(dt):
            want = c.want()[1]
            for wrong in c.perturbations():
                per_row = (c.want(wrong)[1] - want).abs().max(1).values
                assert float(per_row.min()) > bound, (c.what(), wrong, float(per_row.min()), bound)
                least[wrong] = min(least.get(wrong, float("inf")), float(per_row.min()))
    print(f"[sensitivity] {dt}: least movement of a row's c' per wrong reading {least}")
    assert set(least) == {"x_cols", "h_cols", "identity", "tok_prev"}


def test_route_rules():
    assert [L.fused_slabs(64 * t - 7, 128) for t, _ in L.DEPTH_TILES] == [s for _, s in L.DEPTH_TILES]
    assert [L.fused_workgroups(64 * t - 7, 128) for t, _ in L.DEPTH_TILES] == [512, 520, 768, 776, 1280, 1288]
    assert [L.fused_slabs(1280, hh) for _, hh in L.BENCH_POINTS] == [3, 3]
    assert [L.wreg_mapping(hh) for _, hh in L.WREG_SHAPES] == ["remap"] * 4 + ["plain"] * 2
    assert all(L.wreg_supported(e, hh) for e, hh in L.WREG_SHAPES) and not any(L.wreg_supported(e, hh) for e, hh in L.WREG_UNSUPPORTED)
