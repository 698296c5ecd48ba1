"""The vocabulary-classifier tests' own reference and case tables (vocab_ref.py), checked without a GPU: the fp64 references
against F.linear / torch.log_softmax, the restated launch plan against values worked out by hand from csrc/gemm_bf16.hip, every
case table against the route set its GPU test asserts (from the restated launcher rules alone, so a typo in a shape is found
here), the integer flavour's premise, and its sensitivity: zeroing any one 64-deep K slab of the operands (the tail included)
changes at least one logit of every 16-row x 64-column block -- where no logits are written, at least one of the block's 16
group maxima -- so a kernel that dropped, doubled or mixed up a slab in any MFMA block cannot pass torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import vocab_ref as R
from vocab_ref import BF16, DT16, F16


def test_references_equal_f_linear_and_log_softmax():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)    # noqa: E731
    a, w, bias = rnd(7, 24), rnd(150, 24), rnd(150)
    want = F.linear(a, w, bias)
    assert torch.allclose(R.logits_ref(a, w, bias), want, atol=1e-12, rtol=0)
    assert torch.allclose(R.logits_ref(a, w), F.linear(a, w), atol=1e-12, rtol=0)
    gm = R.group_max_ref(want, 4)                             # 150 columns: groups 0, 1, 22 columns of group 2, group 3 past V
    assert gm.shape == (7, 4) and torch.equal(gm[:, 0], want[:, :64].max(1).values) and torch.equal(gm[:, 2], want[:, 128:].max(1).values)
    assert bool((gm[:, 3] == R.NEG_INF).all()) and torch.equal(R.group_max_ref(want), gm[:, :3])
    targets = torch.tensor([0, 149, -1, 150, 75, 3, 1000])
    lp = R.logprob_ref(want, targets)
    ref = torch.log_softmax(want, -1)
    assert lp.dtype == torch.float64 and lp[[2, 3, 6]].tolist() == [0.0, 0.0, 0.0]
    assert torch.allclose(lp[[0, 1, 4, 5]], ref[[0, 1, 4, 5], [0, 149, 75, 3]], atol=1e-12, rtol=0)
    assert R.n_groups(150) == 4 and R.n_groups(128) == 2 and R.n_groups(36541) == 572


PLANS = {
    (1280, 8192): [5], (768, 36541): [3], (2048, 4000): [8], (2816, 10150): [8, 3], (6656, 3000): [16, 10],
    (2304, 16300): [7, 2], (512, 5000): None, (3072, 10150): None, (2048, 3968): None,
}


def test_areg256_plan():
    for (m, v), plan in PLANS.items():
        assert R.areg256_plan(m, v) == plan, (m, v)
    for shape, plan in R.A256_SINGLE + R.A256_MULTI:
        assert R.areg256_plan(*shape) == plan and PLANS.get(shape, plan) == plan, shape
    assert R.areg256_plan(1280, 8192, 8191) is None and R.areg256_plan(1280, 8100, 8128) is None and R.areg256_plan(1280, 8100, 8192) == [5]
    assert R.areg256_plan(1281, 8192) is None and R.areg256_plan(256, 36541) is None and R.areg256_plan(512, 16384) == [2]
    # every launch of a plan has a size that fits, the sizes add up, and no launch is a single tile
    for tiles in range(2, 130):
        plan = R.areg256_plan(256 * tiles, 36541)
        assert plan is not None and sum(plan) == tiles and min(plan) >= 2, tiles
        assert all((32 // t) * t >= 28 for t in plan)
    assert [len(R.areg256_plan(256 * t, 36541)) for t in (8, 9, 10, 11, 13, 16, 17, 27, 32, 33)] == [1, 2, 1, 2, 2, 1, 2, 3, 1, 2]


def test_route_mirrors():
    """The rules at their thresholds."""
    r = R.route
    assert r(1280, 8192, 512, True, 8192) == "a256" and r(1280, 8192, 512, True, 8192, vocab_areg=128) == "a128"
    assert r(1280, 8192, 512, True, 8192, vocab_areg=0) == "pers" and r(1280, 8192, 256, True, 8192) == "pers"
    assert r(1280, 8192, 512, True, 8190) == "tile" and r(1280, 8192, 512, True, 8192, aligned=False) == "tile"
    assert r(1280, 8192, 64, True, 8192) == "tile" and r(1280, 8192, 520, True, 8192) == "tile" and r(1280, 8192, 128, True, 8192) == "pers"
    assert r(1280, 8192, 512, False) == "g256" and r(511, 8192, 512, False) == "pers" and r(512, 8192, 128, False) == "g256"
    assert r(512, 5000, 512, True, 5120) == "pers" and r(512, 8192, 512, True, 8192) == "a128" and r(512, 8191 - 127, 512, True, 8192) == "pers"
    assert r(128, 36541, 512, True, 36544) == "a128" and r(128, 255 * 128, 512, True, 36544) == "pers"
    assert r(129, 36541, 512, True, 36544) == "a128" and r(2176, 36541, 512, True, 36544) == "pers"      # 17 row tiles: 17 < 28
    assert r(3500, 36541, 512, True, 36544) == "a128" and r(4097, 36541, 512, True, 36544) == "pers"     # 28 tiles; 33 tiles
    w = R.wreg_supported
    assert w(640, 1000, 512, 1024, 16) and not w(641, 1000, 512, 1024, 16) and w(1280, 1000, 512, 1024, 16) and not w(720, 1000, 512, 1024, 16)
    assert w(2560, 1000, 512, 0, 16) and not w(5120, 1000, 512, 0, 16) and not w(80, 1000, 256, 1024, 16)
    assert not w(80, 1000, 512, 1020, 16) and not w(80, 1000, 512, 1026, 16) and not w(80, 1000, 512, 1024, 15)
    assert R.logprob_route(511) == "lse128" and R.logprob_route(512) == "lse256"


@pytest.mark.parametrize("fl", R.FLAVOURS)
def test_case_sets_reach_their_routes(fl):
    """What every GPU test asserts with ``==``, from the mirrors alone."""
    for dt in DT16:
        for name, (cases, routes) in R.CASE_SETS.items():
            assert {c.route for c in cases(dt, fl)} == routes, name
    assert [R.areg256_plan(c.m, c.v, c.ldl) for c in R.a256_single_cases(BF16, fl)] == [p for _, p in R.A256_SINGLE]
    assert [R.areg256_plan(c.m, c.v, c.ldl) for c in R.a256_multi_cases(BF16, fl)] == [p for _, p in R.A256_MULTI]
    assert [c.route for c in R.abandoned_cases(F16, fl)] == [r for _, r in R.ABANDONED] + ["a128"]
    assert all(R.route(c.m, c.v, c.k, True, c.ldl) == "a256" for c in R.areg128_cases(BF16, fl))
    c, parts = R.sliced_parts(BF16, fl)
    assert {R.route(rows, c.v, c.k, True, c.ldl) for _, rows in parts} == R.SLICED_ROUTES and sum(rows for _, rows in parts) == c.m
    # every case: operand strides the launchers take, a logits stride wider than its route writes, rows of 16 bytes unless the
    # case is there for the other path
    for name, (cases, _) in R.CASE_SETS.items():
        for c in cases(BF16, fl):
            assert c.lda % 8 == 0 and c.ldw % 8 == 0 and c.k % 8 == 0, (name, c.what())
            if c.logits:
                assert c.ldl >= c.l_off + c.pad_to and (c.ldl > c.l_off + c.pad_to or name == "abandoned"), (name, c.what())
                assert (c.ldl % 4 == 0 and c.aligned) or c.route == "tile", (name, c.what())
            else:
                assert c.k >= 128 and c.k % 64 == 0, (name, c.what())
            if c.entry == "wreg":
                assert R.wreg_supported(c.m, c.v, c.k, c.ldl, c.groups + R.GM_SPARE), c.what()
    assert {c.pad_to > c.v for c in R.a256_single_cases(BF16, fl)} == {False, True}
    assert {c.v % 64 == 0 for c in R.wreg_cases(BF16, fl)} == {False, True} and {c.v % 256 == 0 for c in R.wreg_cases(BF16, fl)} == {False, True}
    assert {(c.lda > c.k, c.ldw > c.k) for c in R.stride_cases(BF16, fl)} == {(True, True)}
    assert {R.logprob_route(m) for m, _, _ in R.LOGPROB} == {"lse128", "lse256"} == {R.logprob_route(m) for m, _, _ in R.LOGPROB_SPIKE}
    assert {(R.logprob_route(m), k) for m, _, k in R.LOGPROB} == {(r, k) for r in ("lse128", "lse256") for k in (128, 512, 1024)}
    assert {m for m, _, _ in R.LOGPROB} == {37, 300, 512, 600} and sorted(v for _, v, _ in R.LOGPROB).count(36541) == 1


def test_logprob_cases():
    c = R.LogprobCase(F16, 37, 1000, 128, spike=True)
    assert c.targets[:6].tolist() == [0, 999, -1, 1000, 998, 500] and int((c.targets == 500).sum()) == 1
    assert bool(torch.isfinite(c.w.float()).all()) and float(c.w[500, 0]) == 15.0 and c.a.dtype == F16
    want = c.want()
    assert want[2:4].tolist() == [0.0, 0.0] and float(want[5]) > -1e-6 and float(want[6:].max()) < -(R.SPIKE - 15)
    # without the rescale across groups the result is off by about log(V)
    lg = c.logits()
    no_rescale = lg[:, 0] - lg.max(-1).values - torch.log(torch.exp(lg.view(37, -1, 8) - lg.view(37, -1, 8).max(-1, keepdim=True).values).sum((1, 2)))
    assert float((no_rescale - R.logprob_ref(lg, torch.zeros(37, dtype=torch.long))).abs().min()) > 3.0


def int_cases():
    """Every integer case once per (operands, bias, logits): its operands do not depend on the 16-bit type."""
    seen = set()
    for name, (cases, _) in R.CASE_SETS.items():
        for c in cases(BF16, "int"):
            key = c._key + (c.logits, c.has_bias and not c.logits)
            if key not in seen:
                seen.add(key)
                yield name, c
    yield "sliced", R.sliced_parts(BF16, "int")[0]


def test_integer_cases_keep_their_premise():
    """Entries are integers exactly representable in every type and 9 K + |bias| stays below 2^24: every partial result is exact
    in fp32."""
    n_cases = 0
    for name, c in int_cases():
        n_cases += 1
        assert 9 * c.k + 8 < 2 ** 24 and c.flavour == "int"
        for x, lim in ((c.a_buf, 3), (c.w_buf, 3), (c.bias, 8)):
            if x is None:
                continue
            assert float(x.double().abs().max()) <= lim and torch.equal(x.double(), x.double().round()), (name, c.what())
            for dt in (BF16, F16):
                assert torch.equal(x.double(), x.to(dt).double())
        if c.m * c.v <= 1 << 22:
            want = c.want()
            assert float(want.abs().max()) <= 9 * c.k + 8 and torch.equal(want, want.round()) and torch.equal(want.float().double(), want)
    assert n_cases >= 45


def test_a_dropped_slab_is_visible():
    """For every integer case and every 64-deep K slab (the tail included): dropping the slab changes at least one logit of
    every 16-row x 64-column block (a logit changes exactly when the slab's own partial product is not zero); for the cases
    without logits, at least one of the block's 16 group maxima."""
    n_cases = n_slabs = 0
    for name, c in int_cases():
        n_cases += 1
        mb, nb = R.cdiv(c.m, 16), c.real_groups
        a, w = c.a.float(), c.w.float()
        gm = None if c.logits else R.group_max_ref(c.want())
        for k0, k1 in c.slabs():
            n_slabs += 1
            if c.logits:
                changed = torch.zeros(mb * 16, nb * 64, dtype=torch.bool)
                changed[:c.m, :c.v] = (a[:, k0:k1] @ w[:, k0:k1].t()) != 0
                per_block = changed.view(mb, 16, nb, 64).any(3).any(1)
            else:
                changed = torch.zeros(mb * 16, nb, dtype=torch.bool)
                changed[:c.m] = R.group_max_ref(c.want(drop=(k0, k1))) != gm
                per_block = changed.view(mb, 16, nb).any(1)
            assert bool(per_block.all()), (name, c.what(), (k0, k1), int((~per_block).sum()))
    print(f"[sensitivity] {n_cases} integer cases, {n_slabs} slabs")
    assert n_cases >= 45
