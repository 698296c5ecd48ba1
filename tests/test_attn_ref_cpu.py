"""The decode attention tests' own reference and inputs (attn_ref.py), checked without a GPU: the vectorised fp64 reference
against the per-row loop of test_kernels_gpu._attn_ref, and the sensitivity condition of every self-attention case of
test_attn_decode_gpu.py -- a kernel that dropped key t or key t - 1 would be seen."""
import pytest
import torch

import attn_ref as A
from attn_ref import BF16, DT_IDS, DTYPES, F16, F32
from test_attn_decode_gpu import ULP_GATE
from test_kernels_gpu import _attn_ref


def naive_self(c):
    """test_attn_self_decode's reference, row by row."""
    d, h, dh, t = c.d, c.n_heads, c.dh, c.t
    qkv, kc, vc = c.qkv.double(), c.kc.double(), c.vc.double()
    ref = torch.empty(c.rows, d, dtype=torch.float64)
    for rc in range(c.rows):
        rl = rc * c.row_mult
        keys = torch.stack([kc[j, c.src[rl, j]] for j in range(t)] + [qkv[rc, d:2 * d]]).view(t + 1, h, dh)
        vals = torch.stack([vc[j, c.src[rl, j]] for j in range(t)] + [qkv[rc, 2 * d:]]).view(t + 1, h, dh)
        masked = torch.tensor([False] + [c.pad_index >= 0 and bool(c.tokens[rl, j - 1] == c.pad_index) for j in range(1, t + 1)])
        ref[rc] = _attn_ref(qkv[rc, :d].view(h, dh), keys, vals, masked, c.scale)
    return ref


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_vectorised_reference_equals_the_row_loop(dt):
    cases = [A.SelfCase(dt, 3, 4, 1, 512, 8, t, 20, pad, 8.0) for t, pad in ((0, 0), (1, 5), (9, 0), (17, -1))]
    cases += [A.SelfCase(dt, 2, 1, 4, 128, 8, 9, 12, 0, 4.0), A.SelfCase(dt, 2, 17, 1, 384, 4, 6, 12, 5, 96 ** 0.5)]
    for c in cases:
        assert float((c.want() - naive_self(c)).abs().max()) < 1e-12, c.what()
        if c.pad_index >= 0 and c.t >= 9:
            assert bool((c.tokens[:, :c.t] == c.pad_index).any())            # the mask is exercised
    for c in (A.CrossCase(dt, 5, 7, 512, 8, 8.0), A.CrossCase(dt, 2, 1, 128, 8, 4.0), A.CrossCase(dt, 17, 65, 256, 8, 32 ** 0.5)):
        want = c.want()
        for row in range(c.rows):
            i, s = row // c.rows_per_img, c.s
            keys = c.kv[i * s:(i + 1) * s, :c.d].double().reshape(s, c.n_heads, c.dh)
            vals = c.kv[i * s:(i + 1) * s, c.d:].double().reshape(s, c.n_heads, c.dh)
            ref = _attn_ref(c.q[row].double().view(c.n_heads, c.dh), keys, vals, c.mask[i * s:(i + 1) * s].bool(), c.scale)
            assert float((want[row] - ref).abs().max()) < 1e-12, (c.what(), row)
        live = (c.mask.view(3, s) == 0).sum(1).tolist()
        assert live[1] == 0 and live[2] == 1                                   # fully masked; only the last key live
        assert c.mask[3 * s - 1] == 0


def all_self_cases(dt):
    for pad_index in (0, 5, -1):
        yield from A.self_sweep_cases(dt, pad_index)
    for cases in A.SELF_CASE_SETS.values():
        yield from cases(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_a_dropped_key_is_visible(dt):
    """Leaving key t or key t - 1 out of the fp64 reference moves every even row, in at least one element, by more than
    8 x the gate of the case's route (fp32: 8 x the atol)."""
    least = {}
    n = 0
    for c in all_self_cases(dt):
        if c.t == 0:
            continue                                           # a single key: nothing can be dropped
        want = c.want()
        for drop in (c.t, c.t - 1):
            moved = c.want(drop=drop)
            if dt == F32:
                move, bound = (moved - want).abs(), 8 * A.F32_ATOL
            else:
                move, bound = A.ulps(moved, want, dt), 8 * ULP_GATE[c.route][dt]
            per_row = move.max(1).values[0::2]
            assert float(per_row.min()) > bound, (c.what(), drop, float(per_row.min()), bound)
            least[c.route] = min(least.get(c.route, float("inf")), float(per_row.min()))
            n += 1
    print(f"[sensitivity] {dt}: {n} (case, key) pairs; least movement of an even row per route {least}")
    assert set(least) == set(A.SELF_ROUTES)


def test_gate_table_is_complete():
    assert set(ULP_GATE) == set(A.SELF_ROUTES) | set(A.CROSS_ROUTES) | {"cross_packed"}
    for name, row in ULP_GATE.items():
        assert set(row) == {BF16, F16}
        if not name.startswith("cross_packed"):                # the kernels that compute in fp32 and round once
            assert max(row.values()) <= 1.25, name
