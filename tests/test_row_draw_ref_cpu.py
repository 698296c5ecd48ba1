"""``tests/row_draw_ref.py`` on the CPU: the Philox restatement against known answers, the row draw against the oracle's
``BeamBook.keep_top_k`` + ``torch.multinomial``'s race and against ``nucleus_ref``, the sampled select against golden G4 -- and the
tables of ``tests/test_row_draw_routes_gpu.py``: every route reached, both sides of every dispatch boundary, every row's margin,
the candidate counts of the loose-bound rows.  All before a GPU is asked anything.  Last, the argument checks of the row-draw entry
points, which return before any launch."""
import numpy as np
import pytest
import torch

import row_draw_ref as R
import test_row_draw_routes_gpu as G
from beam_search_ref import State
from helpers import golden
from nucleus_ref import nucleus_row_sample


# ---- Philox -----------------------------------------------------------------------------------------------------------------------
def words(o):
    return " ".join("%08x" % int(w) for w in o)


def test_philox_known_answers():
    """The kernel's round function (common.h philox4x32) written out: ten rounds, key bumped after each."""
    assert words(R.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(R.philox4x32((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(R.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised == one by one
    idx = np.arange(5)
    many = R.philox4x32((idx, 7, 2, 0), (3, 4))
    for i in idx:
        assert [int(w[i]) for w in many] == [int(w) for w in R.philox4x32((int(i), 7, 2, 0), (3, 4))]


def test_philox_exp1_layout_and_range():
    u = R.philox_u(np.array([0, 0xFFFFFFFF], dtype=np.uint64))
    assert 0.0 < u[0] < u[1] < 1.0 and u[0] == 0.5 / 2 ** 23 and u[1] == 1.0 - 0.5 / 2 ** 23
    assert float(np.float32(u[1])) == u[1] < 1.0                          # exact in fp32
    x = R.philox_exp1(5, 0, 0, 0, 0, np.arange(100000))
    assert bool((x > 0).all()) and abs(float(x.mean()) - 1.0) < 0.01
    # counter (idx, row, step, kind), key (lo32(seed) ^ img * 0x9E3779B1 mod 2^32, hi32(seed) + img mod 2^32)
    seed, img, step, kind, row, idx = (9 << 32) | 0x1234, 3, 6, 1, 2, 77
    o = R.philox4x32((idx, row, step, kind), (0x1234 ^ ((img * 0x9E3779B1) & 0xFFFFFFFF), 9 + img))
    assert float(R.philox_exp1(seed, img, step, kind, row, idx)) == float(-np.log(R.philox_u(o[0])))
    # the tables: stream kinds 0 / 1 / 2
    t = R.row_noise(seed, 4, 6, 5, 2, 9)
    assert t[3, 7] == R.philox_exp1(seed, 4 + 1, 6, 0, 1, 7) and t.shape == (5, 9)
    assert R.select_noise(seed, 4, 6, 2, 3)[1, 5] == R.philox_exp1(seed, 5, 6, 1, 0, 5)
    assert R.final_noise(seed, 4, 2, 3)[1, 2] == R.philox_exp1(seed, 5, 0xFFFFFFFF, 2, 0, 2)


# ---- the row draw -----------------------------------------------------------------------------------------------------------------
def book_draw(logits, noise, temp, beam, top_k, unk=1):
    from oracle.ref_path import BeamBook
    filt = BeamBook(temp, beam, top_k, unk_index=unk).keep_top_k(logits.clone())
    picks = torch.topk(torch.softmax(filt.double() / temp, -1) / noise.double(), beam, dim=-1).indices
    return picks, torch.gather(filt.double(), 1, picks).log_softmax(-1)


def test_row_draw_is_keep_top_k_and_the_multinomial_race_on_g4():
    logits = torch.from_numpy(golden("g4_beam_helper.npz")["pl_logits"])
    torch.manual_seed(7)
    noise = torch.empty(3, logits.shape[1]).exponential_(1)               # what multinomial consumed inside process_logits
    picks, vals, flags, margins = R.row_draw(logits, noise, 0.7, 3, 5, 1)
    want_p, want_v = book_draw(logits, noise, 0.7, 3, 5)
    assert picks.tolist() == want_p.tolist() and flags == [0, 0, 0] and min(margins) > 0
    assert float((vals - want_v).abs().max()) < 1e-12


@pytest.mark.parametrize("v,top_k,beam,temp", [(71, 50, 7, 1.1), (1000, 20, 3, 1.3), (500, 1, 1, 1.0), (3, 3, 2, 1.0)])
def test_row_draw_is_the_oracle_on_random_rows_with_ties_signed_zeros_and_unk(v, top_k, beam, temp):
    g = torch.Generator().manual_seed(v)
    logits = (torch.randn(6, v, generator=g) * 2.5 * 4).round() / 4       # quarters: ties at the threshold, zeros
    logits[logits == 0] = torch.where(torch.rand(int((logits == 0).sum()), generator=g) < 0.5, 0.0, -0.0)
    if top_k > 2:
        logits[0, 1] = 50.0
    noise = torch.empty(6, v).exponential_(1, generator=g)
    picks, vals, flags, _ = R.row_draw(logits, noise, temp, beam, top_k, 1)
    want_p, want_v = book_draw(logits, noise, temp, beam, top_k)
    assert picks.tolist() == want_p.tolist() and not any(flags)
    assert float((vals - want_v).abs().max()) < 1e-12


def test_row_draw_nucleus_is_nucleus_ref():
    cases = [(60, 20, 3, 1.0, 0.5, 3.0), (71, 50, 7, 1.1, 0.8, 2.5), (1000, 20, 3, 1.3, 0.3, 2.5), (5000, 200, 3, 1.0, 0.97, 0.3),
             (500, 1, 1, 1.0, 0.8, 2.5)]
    for v, top_k, beam, temp, top_p, scale in cases:
        g = torch.Generator().manual_seed(v + top_k)
        logits = torch.randn(6, v, generator=g) * scale
        noise = torch.empty(6, v).exponential_(1, generator=g)
        want_p, want_v, margin, _ = nucleus_row_sample(logits, noise, temp, beam, top_k, top_p)
        picks, vals, flags, margins = R.row_draw(logits, noise, temp, beam, top_k, 1, top_p)
        assert picks.tolist() == want_p.tolist() and not any(flags), (v, top_k)
        assert float((vals - want_v.double()).abs().max()) < 2e-6 and min(margins) <= margin + 1e-12


def test_row_draw_flags():
    ninf, inf, nan = float("-inf"), float("inf"), float("nan")
    x = torch.tensor([[0.0, 9.0, 1.0, 2.0, 3.0, 4.0],            # top-1 is <unk>
                      [0.0, 9.0, 1.0, 2.0, 3.0, 4.0],
                      [ninf, 0.0, ninf, 2.0, ninf, 1.0],         # two live logits
                      [0.0, 1.0, inf, 2.0, 3.0, 4.0],
                      [0.0, nan, 1.0, 2.0, 3.0, 4.0],            # a NaN at <unk>: dropped, but it holds a top-k place
                      [0.0, 1.0, 2.0, 3.0, 4.0, G.BAD["-nan"]]])
    nz = torch.ones(6, 6)
    assert R.row_draw(x[:1], nz[:1], 1.0, 1, 1, 1)[2] == [R.ERR_ALL_FILTERED]
    picks, vals, flags, _ = R.row_draw(x, nz, 1.0, 3, 3, 1)
    assert flags == [R.ERR_TOO_FEW, R.ERR_TOO_FEW, R.ERR_TOO_FEW, R.ERR_NONFINITE, R.ERR_TOO_FEW, R.ERR_NONFINITE]
    assert picks[0].tolist() == [5, 4, -1] and vals[0, 2] == ninf and picks[2].tolist() == [3, 5, -1]
    assert picks[3].tolist() == [0, 0, 0] and vals[3].tolist() == [0.0, 0.0, 0.0] and picks[4].tolist() == [5, 4, -1]
    assert abs(float(vals[0, 0]) - float(torch.tensor([4.0, 3.0]).double().log_softmax(0)[0])) < 1e-12


# ---- the select and the final draw ------------------------------------------------------------------------------------------------
def test_select_sampled_reproduces_g4():
    """What test_beam_select_matches_reference_process_logits expects of the kernels, expected of the restatement."""
    g = golden("g4_beam_helper.npz")
    logits = torch.from_numpy(g["pl_logits"])
    b = 3
    torch.manual_seed(7)
    noise_row = torch.empty(b, logits.shape[1]).exponential_(1)
    pi, pv, _, _ = R.row_draw(logits, noise_row, 0.7, b, 5, 1)
    tokens = torch.zeros(b, 4, dtype=torch.int32)
    tokens[:, :2] = torch.from_numpy(g["pl_seqs"]).int()
    st = State.of(tokens, torch.from_numpy(g["pl_vals"]), torch.tensor([0, 1, 0]), torch.zeros(1), torch.zeros(1), b)
    n_cand = len(g["pl_new_ind"])
    cand_val = torch.from_numpy(g["pl_prev_vals"].reshape(-1) + g["pl_new_val"])
    noise_c = torch.ones(b * b)
    noise_c[:n_cand] = torch.tensor([1.0, 50.0, 60.0, 0.5, 0.1, 70.0, 80.0])
    keep = torch.topk(torch.softmax(cand_val / 0.7, -1) / noise_c[:n_cand], b).indices
    margins = R.select_sampled(st, pi, pv.float(), noise_c.numpy(), 0.7, False, 2, 0, 2, 3, first_sets_ended=False)
    exp_seq = torch.cat([torch.from_numpy(g["pl_prev_seqs"]), torch.from_numpy(g["pl_new_ind"])[:, None]], 1)[keep]
    assert st.tokens[:, :3].tolist() == exp_seq.tolist() and margins[0] > 1e-3
    assert float((st.vals - cand_val[keep]).abs().max()) <= 2e-6
    assert st.ended.bool().tolist() == torch.from_numpy(g["pl_has_ended"])[keep].tolist()
    assert st.parent.tolist() == torch.tensor([0, 0, 0, 1, 2, 2, 2])[keep].tolist()
    assert st.hparent.tolist() == (keep // b).tolist()                       # rnn_models.py:135-137 dense-layout quirk
    assert int(st.done[0]) == int(bool(torch.from_numpy(g["pl_has_ended"])[keep].all()))


def test_final_draw_first_index_on_ties():
    drawn, margins = R.final_draw(torch.tensor([[-1.0, -1.0, -2.0], [float("-inf"), -3.0, -1.0]]), np.array([[2.0, 2.0, 0.1], [1.0, 9.0, 1.0]]), 1.0)
    assert drawn == [2, 2] and margins[0] > 0
    assert R.final_draw(torch.tensor([[-1.0, -1.0]]), np.ones((1, 2)), 0.7)[0] == [0]


# ---- the GPU module's tables ------------------------------------------------------------------------------------------------------
def test_route_restates_the_dispatch():
    for v, want in ((1, "f8"), (4096, "f8"), (4097, "f16"), (16384, "f16"), (16385, "f36"), (36864, "f36"), (36865, "f64"),
                    (65536, "f64"), (65537, "general")):
        assert R.route(v, 256) == want and R.route(v, 1) == want
        assert R.route(v, 257) == "general" and R.route(v, 50, exact=True) == "general"
        assert R.route(v, 50, groups=True) == "groups" and R.route(v, 50, exact=True, groups=True) == "general"
    assert R.groups_allowed(65536, 256) and not R.groups_allowed(65537, 50) and not R.groups_allowed(71, 3) and R.groups_allowed(71, 2)
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deephumor_amd", "csrc", "beam.hip")).read()
    for line in ("if (!exact && top_k <= 256 && V <= 512 * 8) DH_FAST(8, 512, 4);", "else if (!exact && top_k <= 256 && V <= 1024 * 16) DH_FAST(16, 1024, 8);",
                 "else if (!exact && top_k <= 256 && V <= 1024 * 36) DH_FAST(36, 1024, 8);", "else if (!exact && top_k <= 256 && V <= 1024 * 64) DH_FAST(64, 1024, 4);",
                 "if (group_max && !exact) {", "n_groups > 0 && n_groups <= 1024 && top_k <= n_groups"):
        assert line in src, line                                             # the quoted lines are still the source's


def test_case_table_reaches_every_route_and_both_sides_of_every_boundary():
    reached = {G.route_of(v, k, e) for v, k, _, _ in G.CASES for e in G.entries(v, k)}
    assert reached == set(R.ROUTES)
    vs = {c[0] for c in G.CASES}
    assert vs >= {3, 71, 4096, 4097, 16384, 16385, 36864, 36865, 65536, 65537}
    for v in (4096, 16384, 36864, 65536):                                    # the two sides run different kernels through the plain entry
        lo = {R.route(v, k) for vv, k, _, _ in G.CASES if vv == v and k <= 256}
        hi = {R.route(v + 1, k) for vv, k, _, _ in G.CASES if vv == v + 1 and k <= 256}
        assert len(lo) == 1 and len(hi) == 1 and lo != hi, v
    ks = {(c[0], c[1]) for c in G.CASES}
    assert any((v, 256) in ks and (v, 257) in ks for v in vs)               # top_k = 256 / 257 at one V
    assert {c[1] for c in G.CASES} >= {1, 50, 256, 257} and {c[2] for c in G.CASES} >= {1, 5, 64} and {c[3] for c in G.CASES} == {0.7, 1.0, 1.3}
    assert {G.route_of(*c[:2], e) for c, e in G.ROUTE_CASE.values()} == set(R.ROUTES) == set(G.ROUTE_CASE)
    assert all(G.route_of(c[0], c[1], e) == rt for rt, (c, e) in G.ROUTE_CASE.items())
    assert {("general" if rt == "exact" else rt) for rt in G.ROUTE_V} == set(R.ROUTES)
    assert all(G.route_of(v, 50, e) == ("general" if rt == "exact" else rt) for rt, (v, e) in G.ROUTE_V.items())
    print("routes reached:", sorted(reached))


@pytest.mark.parametrize("v,top_k,beam,temp", G.CASES, ids=lambda x: str(x))
def test_every_case_row_has_its_margin(v, top_k, beam, temp):
    logits, noise, want = G.case_inputs(v, top_k, beam, temp)
    low = min(min(w[3]) for w in want.values())
    print(f"V {v} top_k {top_k} beam {beam} T {temp}: smallest margin {low:.3e}")
    assert low >= R.MARGIN and all(f == 0 for w in want.values() for f in w[2]) and logits.shape == (G.ROWS, v)
    if top_k > 2:
        assert int(logits[0].argmax()) == 1 and not bool((want[None][0] == 1).any())            # <unk> as the arg-max, never picked
    if top_k > 2 and v >= top_k + 16:
        assert bool((logits[2, 10:10 + top_k + 3] == 30.0).all()) and int((logits[2] > 30.0).sum()) == 1   # ties straddle the threshold


def test_loose_bound_rows_pass_the_bound_in_thousands():
    low = float("inf")
    for table, lo, hi in ((G.HOT_OVER, R.MAX_SURVIVORS + 1, 1 << 30), (G.HOT_MID, 500, R.MAX_SURVIVORS)):
        for rt, v, top_k, hot in table:
            logits, noise, want = G.hot_inputs(rt, v, top_k, hot)
            count = [R.group_candidates(x, top_k) if rt == "groups" else R.fast_candidates(x, top_k, rt) for x in logits.numpy()]
            print(rt, v, top_k, hot, "candidates past the bound:", count)
            assert all(lo <= c <= hi for c in count), (rt, count)
            assert G.route_of(v, top_k, "groups" if rt == "groups" else "plain") == rt and not any(want[2])
            low = min(low, min(want[3]))
            for r in range(G.ROWS):                                          # the true threshold is sharp: top_k survivors, <unk> aside
                assert int((logits[r] >= torch.topk(logits[r], top_k).values[-1]).sum()) == top_k
    assert low >= R.MARGIN


def test_the_other_inputs_have_their_margins():
    low = float("inf")
    for rt, (v, entry) in G.ROUTE_V.items():
        for n in (1024, 1025):
            logits, _, want = G.tied_inputs(v, n)
            assert int((logits[0] == 9.0).sum()) == n and float(logits.max()) == 9.0 and not any(want[2])
            low = min(low, min(want[3]))
    for args, flag in (((71, 10, 50, 5), 0), ((5000, 10, 50, 5), 0), ((71, 3, 50, 5), R.ERR_TOO_FEW)):
        want = G.sparse_inputs(*args)[2]
        assert want[2] == [flag] * G.ROWS
        low = min(low, min(want[3]))
    logits, noise, _ = G.case_inputs(4096, 50, 5, 1.0)
    low = min(low, min(R.row_draw(logits, noise, 1.0, 5, 5, 1)[3]), min(R.row_draw(logits, noise, 1.0, 1, 1, 1)[3]))
    for rt in list(G.ROUTE_CASE) + ["exact"]:
        for bad in G.BAD:
            want = G.nonfinite_inputs(rt, bad)[2]
            assert want[2] == [0, R.ERR_NONFINITE, 0, 0, 0, 0]
            low = min(low, min(want[3]))
    for name in G.FLAT_VARIANTS:
        assert G.flat_inputs(*G.flat_variant(name))[1] >= 1e-5
    for beam in (1, 3, 5, 17, 64):
        for with_src in (False, True):
            for case in range(len(G.SELECT_STEPS)):
                for philox in (False, True):
                    low = min(low, min(G.select_inputs(beam, with_src, case, philox)[6]))
    for beam in (1, 5, 64):
        for philox in (False, True):
            low = min(low, min(G.final_inputs(beam, philox)[4]))
    print(f"smallest margin of the other tables: {low:.3e}")
    assert low >= R.MARGIN


@pytest.mark.parametrize("rt", list(G.ROUTE_CASE))
def test_philox_cases_have_their_margins(rt):
    (v, top_k, beam, temp), _ = G.ROUTE_CASE[rt]
    for top_p, pstep in ((None, None), (0.8, None), (None, 0), (None, 2), (None, 3), (0.8, 2)):
        seed, _, want, drawn, _, _ = G.philox_inputs(v, top_k, beam, temp, top_p, pstep, 900, 3, 4, 3)
        assert min(want[3][r] for r in drawn) >= R.MARGIN and not any(want[2][r] for r in drawn)


# ---- the entry points' argument checks --------------------------------------------------------------------------------------------
def test_bad_arguments_return_bad_arg_without_a_launch():
    from deephumor_amd import hip
    lib = hip.load()
    p, bad = 1 << 20, 1                                   # (never dereferenced: every call fails its argument check first) DH_ERR_BAD_ARG

    def plain(name, v=100, beam=3, top_k=5, rpi=1, rows=6):
        tail = (p,) if "prompted" in name else ()
        return getattr(lib, name)(p, 128, v, rows, rpi, beam, top_k, 1.0, 1, None, 0, None, 0, 0, *tail, p, p, p, None)

    def groups(name, v=100, ng=2, beam=1, top_k=2, rpi=1, rows=6):
        tail = (p,) if "prompted" in name else ()
        return getattr(lib, name)(p, 128, v, p, 1024, ng, 64, rows, rpi, beam, top_k, 1.0, 1, None, 0, None, 0, 0, *tail, p, p, p, None)

    def nucleus(top_p=0.5, v=100, beam=3, top_k=5, rpi=1, rows=6, fp=None, gmax=None, ng=2):
        return lib.dh_beam_row_sample_nucleus(p, 128, v, gmax, 1024, ng, 64, rows, rpi, beam, top_k, top_p, 1.0, 1, None, 0, None, 0, 0, fp, 0,
                                              p, p, p, None)
    for name in ("dh_beam_row_sample", "dh_beam_row_sample_exact", "dh_beam_row_sample_prompted", "dh_beam_row_sample_exact_prompted"):
        pr = dict(rpi=3) if "prompted" in name else {}
        assert plain(name, top_k=101, **pr) == bad, name              # top_k > V
        assert plain(name, beam=6, **(dict(rpi=6) if pr else {})) == bad, name      # beam > top_k
        assert plain(name, beam=65, top_k=70, rows=65, **(dict(rpi=65) if pr else {})) == bad, name     # beam > 64
    for name in ("dh_beam_row_sample_groups", "dh_beam_row_sample_groups_prompted"):
        pr = dict(rpi=1) if "prompted" in name else {}
        assert groups(name, top_k=3, **pr) == bad, name               # top_k > n_groups
        assert groups(name, top_k=101, ng=128, **pr) == bad, name     # top_k > V
        assert groups(name, beam=3, **(dict(rpi=3) if pr else {})) == bad, name     # beam > top_k
    for top_p in (0.0, 1.0, 1.5, -0.5, float("nan")):
        assert nucleus(top_p) == bad, top_p                            # top_p outside (0, 1)
    assert nucleus(top_k=101) == bad and nucleus(beam=6) == bad and nucleus(beam=65, top_k=70) == bad
    assert nucleus(gmax=p, top_k=3, beam=1) == bad                     # top_k > n_groups on the groups route
    # first_pos with rows_per_img != beam (and rows that are not whole images)
    assert plain("dh_beam_row_sample_prompted", rpi=1) == bad and plain("dh_beam_row_sample_exact_prompted", rpi=2) == bad
    assert plain("dh_beam_row_sample_prompted", rpi=3, rows=7) == bad
    assert groups("dh_beam_row_sample_groups_prompted", beam=2, rpi=1) == bad
    assert nucleus(fp=p, rpi=1) == bad and nucleus(fp=p, rpi=3, rows=7) == bad
