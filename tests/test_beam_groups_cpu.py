"""``num_beam_groups`` / ``diversity_penalty`` without a GPU: the two CPU statements of a group step against each other (the containment
claim: a row's picks suffice), hand-worked cases for every rule, the checks, the settings record, the helper's launches through recorded
``hip`` wrappers, the keyword through the layers and the C-ABI addition."""
import copy
import ctypes
import dataclasses
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import torch

import beam_groups_ref as GR
import beam_search_ref as R
import length_penalty_ref as LP
from helpers import DECODE_FIELDS, KINDS, synthetic_sd

from deephumor_amd import _abi, _build, hip
from deephumor_amd.models import beam
from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings, check_beam_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
EOS = 3
f32 = np.float32


def ones(n):
    return torch.ones(n + 1)


# ---- the two statements agree: a row's `beam` picks hold every candidate a group can keep ---------------------------------------------
def divisors(b):
    return [g for g in range(2, b + 1) if b % g == 0]


def test_the_picks_hold_what_a_ranking_over_the_whole_vocabulary_keeps():
    """A few hundred random steps, beams 2-12, every divisor ``G > 1``, ``V`` from ``beam + 3`` up, first and later steps: the select on
    the row step's picks and a ranking of every (row, token) of the vocabulary keep the same candidates with the same bits.  Quarter
    values make equal keys common, so the tie rule is exercised too."""
    g = torch.Generator().manual_seed(11)
    cases = 0
    for beam_size in range(2, 13):
        for groups in divisors(beam_size):
            for trial in range(10):
                v = beam_size + 3 + int(torch.randint(0, 12, (), generator=g))
                lam = (0.25, 1.0, 5.0, 50.0)[(cases + trial) % 4]
                first = trial % 5 == 0
                rows = 1 if first else beam_size
                logp = torch.randint(-20, 0, (rows, v), generator=g).float() * 0.25
                logp[torch.rand(rows, v, generator=g) < 0.1] = NEG
                logp[:, :beam_size] = torch.where(torch.isinf(logp[:, :beam_size]), torch.full((), -6.0), logp[:, :beam_size])
                st = GR.new_state(1, beam_size, 6)
                if not first:
                    st.vals = torch.randint(-12, 0, (beam_size,), generator=g).float() * 0.25
                    st.ended = (torch.rand(beam_size, generator=g) < 0.25).to(torch.uint8)
                    st.keys = st.vals.clone()
                picks, vals, _ = R.row_best(logp, 1.0, beam_size, -1)
                pick_val = torch.gather(logp, 1, picks)                          # the log-probabilities themselves, as given
                pi = torch.zeros(beam_size, beam_size, dtype=torch.int64)
                pv = torch.zeros(beam_size, beam_size)
                pi[:rows], pv[:rows] = picks, pick_val
                want = GR.group_step_whole_vocab(logp.numpy(), st.vals.numpy(), st.keys.numpy(), st.ended.tolist(), first, beam_size, groups,
                                                 lam, f32(1.0))
                GR.select_groups(st, pi, pv, first, 2, 0, 2, EOS, ones(6), groups, lam)
                for slot, (par, tok, score, key) in enumerate(want):
                    assert int(st.parent[slot]) == par, (beam_size, groups, trial, slot)
                    assert int(st.tokens[slot, 2]) == (0 if tok is None else tok)
                    assert f32(st.vals[slot]).tobytes() == f32(score).tobytes() and f32(st.keys[slot]).tobytes() == f32(key).tobytes()
                    assert bool(st.ended[slot]) == (tok is None or tok == EOS)
                    if not first:
                        assert par // (beam_size // groups) == slot // (beam_size // groups)      # a beam never changes group
                cases += 1
    assert cases >= 200


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------------
def first_step(beam_size, picks, vals, groups, lam, max_len=4):
    st = GR.new_state(1, beam_size, max_len)
    pi = torch.zeros(beam_size, beam_size, dtype=torch.int64)
    pv = torch.zeros(beam_size, beam_size)
    pi[0], pv[0] = torch.tensor(picks), torch.tensor(vals)
    return GR.select_groups(st, pi, pv, True, 0, 0, 0, EOS, ones(max_len), groups, lam)


def test_a_first_step_with_a_huge_penalty_takes_the_picks_in_pick_order():
    st = first_step(6, [9, 8, 7, 6, 5, 4], [-0.5, -1.0, -1.5, -2.0, -2.5, -3.0], 3, 1e6)
    assert st.tokens[:, 0].tolist() == [9, 8, 7, 6, 5, 4]
    # stored unpenalised: vals and keys are the picks' own values
    assert st.vals.tolist() == [-0.5, -1.0, -1.5, -2.0, -2.5, -3.0] and st.keys.tolist() == st.vals.tolist()
    assert st.parent.tolist() == [0] * 6 and not st.ended.any() and not st.done.any()


def test_a_penalty_that_rounds_away_makes_every_group_repeat_group_zero():
    st = first_step(6, [9, 8, 7, 6, 5, 4], [-0.5, -1.0, -1.5, -2.0, -2.5, -3.0], 3, 1e-9)        # -0.5 - 1e-9 is -0.5 in fp32
    assert st.tokens[:, 0].tolist() == [9, 8, 9, 8, 9, 8] and st.vals.tolist() == [-0.5, -1.0] * 3


def test_the_penalty_is_two_rounded_operations_and_counts_every_earlier_use():
    assert GR.penalised(f32(-1.0), 0.5, 2).tobytes() == f32(-2.0).tobytes()
    lam, q, n = f32(0.1), f32(-0.3), 3                                           # fused, the product would not be rounded to fp32 first
    fused = f32(np.float64(q) - np.float64(lam) * np.float64(n))
    two = GR.penalised(q, lam, n)
    assert two.tobytes() == f32(q - f32(lam * f32(n))).tobytes()
    print("fused", fused, "two roundings", two)
    # G == B: every group holds one beam; group 1 avoids 9 once, group 2 sees 9 and 8 taken once each, ...
    st = first_step(3, [9, 8, 7], [-1.0, -1.25, -2.0], 3, 0.5)
    #   g0: 9.  g1: 9 at -1.5, 8 at -1.25 -> 8.  g2: 9 at -1.5, 8 at -1.75, 7 at -2.0 -> 9
    assert st.tokens[:, 0].tolist() == [9, 8, 9] and st.vals.tolist() == [-1.0, -1.25, -1.0]
    # an equal penalised key goes to the lower candidate index: 9 at -1.0 - 0.25 ties with 8 at -1.25
    st = first_step(2, [9, 8], [-1.0, -1.25], 2, 0.25)
    assert st.tokens[:, 0].tolist() == [9, 9]


def later_state(beam_size, vals, ended, keys=None, max_len=4):
    st = GR.new_state(1, beam_size, max_len)
    st.vals, st.ended = torch.tensor(vals), torch.tensor(ended, dtype=torch.uint8)
    st.keys = st.vals.clone() if keys is None else torch.tensor(keys)
    st.tokens[:, 0] = torch.arange(10, 10 + beam_size, dtype=torch.int32)
    return st


def test_groups_rank_their_own_rows_and_a_beam_never_changes_group():
    st = later_state(4, [-1.0, -1.5, -5.0, -6.0], [0, 0, 0, 0])
    pi = torch.tensor([[9, 8, 7, 6]] * 4)
    pv = torch.tensor([[-0.25, -0.5, -0.75, -1.0]] * 4)
    GR.select_groups(st, pi, pv, False, 1, 0, 1, EOS, ones(4), 2, 0.5)
    # group 0 (rows 0, 1): -1.25 (r0, 9), -1.5 (r0, 8); group 1 (rows 2, 3): its rows are far worse and still fill its slots;
    # 9 and 8 were taken once each: r2: 9 -5.25 - 0.5 = -5.75, 8 -5.5 - 0.5 = -6.0, 7 -5.75, 6 -6.0 -> (r2, 9) by index, then (r2, 7)
    assert st.parent.tolist() == [0, 0, 2, 2] and st.tokens[:, 1].tolist() == [9, 8, 9, 7]
    assert st.vals.tolist() == [-1.25, -1.5, -5.25, -5.75] and st.keys.tolist() == st.vals.tolist()          # unpenalised
    assert st.tokens[:, 0].tolist() == [10, 10, 12, 12]


def test_an_ended_beam_competes_unpenalised_and_uncounted():
    # group 0 = rows 0, 1: row 0 has ended (one candidate, token 0, its key carried); group 1 = rows 2, 3
    st = later_state(4, [-1.0, -1.5, -1.0, -9.0], [1, 0, 0, 0], keys=[-0.5, -1.5, -1.0, -9.0])
    pi = torch.tensor([[0, 5, 6, 7]] * 4)
    pv = torch.tensor([[-0.25, -0.5, -0.75, -1.0]] * 4)
    GR.select_groups(st, pi, pv, False, 1, 0, 1, EOS, ones(4), 2, 100.0)
    # g0: the ended beam (key -0.5, token 0: NOT said), then (r1, 0) at -1.75 -- token 0 is said once, by the live candidate only
    # g1: (r2, 0) -1.25 - 100, (r2, 5) -1.5, (r2, 6) -1.75 -> tokens 5, 6
    assert st.parent.tolist() == [0, 1, 2, 2] and st.tokens[:, 1].tolist() == [0, 0, 5, 6]
    assert st.ended.tolist() == [1, 0, 0, 0] and st.keys.tolist() == [-0.5, -1.75, -1.5, -1.75] and st.vals[0] == -1.0
    # the same with the ended beam in the LATER group: it is not penalised for the token 0 that group 0 took
    st = later_state(4, [-1.0, -9.0, -1.0, -1.5], [0, 0, 1, 0], keys=[-1.0, -9.0, -0.5, -1.5])
    GR.select_groups(st, pi, pv, False, 1, 0, 1, EOS, ones(4), 2, 100.0)
    # g0: (r0, 0), (r0, 5).  g1: the ended beam at -0.5 in front, then r3: 0 and 5 a hundred down, 6 at -2.25
    assert st.tokens[:, 1].tolist() == [0, 5, 0, 6] and st.keys.tolist() == [-1.25, -1.5, -0.5, -2.25] and st.ended.tolist() == [0, 0, 1, 0]


def test_minus_infinity_picks_come_last_and_are_not_counted():
    st = first_step(4, [9, 8, 0, 0], [-1.0, -2.0, NEG, NEG], 2, 1e6)            # a TOO_FEW row: two real picks
    # g0: 9, 8.  g1: both penalised far below, and still above -inf: 9, 8 again -- a -inf pick never wins against a finite one
    assert st.tokens[:, 0].tolist() == [9, 8, 9, 8] and st.vals.tolist() == [-1.0, -2.0, -1.0, -2.0]
    st = first_step(4, [9, 0, 0, 0], [-1.0, NEG, NEG, NEG], 2, 1.0)
    assert st.tokens[:, 0].tolist() == [9, 0, 9, 0] and st.vals.tolist() == [-1.0, NEG, -1.0, NEG]
    # token 0 at -inf was kept by group 0 and NOT said: a live 0 in group 1 is not penalised for it
    st = later_state(2, [-1.0, -1.0], [0, 0])
    GR.select_groups(st, torch.tensor([[0, 0], [0, 5]]), torch.tensor([[NEG, NEG], [-1.0, -1.5]]), False, 1, 0, 1, EOS, ones(4), 2, 1.0)
    assert st.tokens[:, 1].tolist() == [0, 0] and st.vals.tolist() == [NEG, -2.0]


def test_a_done_image_is_untouched_and_all_ended_finishes_the_image():
    st = GR.new_state(2, 2, 4)
    st.done[0], st.end_step[0] = 1, 1
    st.vals = torch.tensor([-1.0, -2.0, -1.0, -2.0])
    before = copy.deepcopy(st)
    pi = torch.tensor([[EOS, 5]] * 4)
    pv = torch.tensor([[-0.25, -3.0]] * 4)
    GR.select_groups(st, pi, pv, False, 2, 0, 2, EOS, ones(4), 2, 0.5)
    for k in ("tokens", "vals", "keys", "ended", "parent"):
        assert torch.equal(getattr(st, k)[:2], getattr(before, k)[:2]), k
    # image 1: group 0 keeps (r2, eos); group 1 (r3, eos) -2.25 - 0.5 against (r3, 5) at -5: eos -> every beam ended: done
    assert st.tokens[2:, 2].tolist() == [EOS, EOS] and st.ended[2:].tolist() == [1, 1] and st.done.tolist() == [1, 1] and st.end_step[1] == 2


def test_the_prompted_phases():
    st = GR.new_state(3, 2, 6)
    st.vals[4:] = torch.tensor([-1.0, -2.0])
    pi = torch.tensor([[9, 8]] * 6)
    pv = torch.tensor([[-0.5, -1.0]] * 6)
    before = copy.deepcopy(st)
    GR.select_groups(st, pi, pv, False, 2, 1, 2, EOS, LP.weights(1.0, 6), 2, 1e6, first_pos=[3, 2, 0])
    # image 0 is forced: nothing but the parents
    assert torch.equal(st.tokens[:2], before.tokens[:2]) and st.parent[:2].tolist() == [0, 0] and st.vals[:2].tolist() == [0.0, 0.0]
    # image 1 makes its first step (L = 1): both groups from the base row's picks
    assert st.tokens[2:4, 2].tolist() == [9, 8] and st.keys[2:4].tolist() == [-0.5, -1.0] and st.parent[2:4].tolist() == [2, 2]
    # image 2 is at L = 3: keys are vals / 3, the groups stay on their own rows
    assert st.parent[4:].tolist() == [4, 5] and st.tokens[4:, 2].tolist() == [9, 8] and st.vals[4:].tolist() == [-1.5, -3.0]
    assert st.keys[4].item() == float(LP.key_of(-1.5, LP.weights(1.0, 6)[3]))


def test_one_group_is_select_best_norm():
    g = torch.Generator().manual_seed(3)
    for lp in (0.0, 1.0):
        st = GR.new_state(2, 4, 6)
        st.vals = torch.randint(-12, 0, (8,), generator=g).float() * 0.25
        st.keys = st.vals.clone()
        st.ended[1] = 1
        pi = torch.randint(3, 9, (8, 4), generator=g)
        pv = torch.sort(torch.randint(-8, 0, (8, 4), generator=g).float() * 0.25, dim=1, descending=True).values
        a = LP.select_best_norm(copy.deepcopy(st), pi, pv, False, 3, 0, 3, EOS, LP.weights(lp, 6))
        b = GR.select_groups(copy.deepcopy(st), pi, pv, False, 3, 0, 3, EOS, LP.weights(lp, 6), 1, 7.0)
        for k in ("tokens", "vals", "keys", "ended", "parent", "hparent", "done"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_the_driver_returns_groups_that_differ_and_scores_that_are_log_probabilities():
    gen = torch.Generator().manual_seed(5)
    table = torch.randn(50, 40, generator=gen) * 2

    def logits_fn(rows, pos, rpi):
        prev = rows[:, pos - 1].long() if pos else torch.zeros(rows.shape[0], dtype=torch.long)
        return table[(prev + 7 * pos) % 50].clone()
    plain, _, _ = GR.beam_search_groups(logits_fn, 2, 6, 6, 1, 0.0)
    out, err, st = GR.beam_search_groups(logits_fn, 2, 6, 6, 3, 50.0)
    assert err == 0 and torch.equal(plain["scores"], LP.beam_search_norm(logits_fn, 2, 6, 6, 0.0)[0]["scores"])
    best = GR.group_best(out, 3)
    for i in range(2):
        firsts = [int(out["tokens"][i, int(best[i, g]), 0]) for g in range(3)]
        assert len(set(firsts)) == 3                                             # three groups, three different openings
        assert len(set(plain["tokens"][i, :, 0].tolist())) < 3                    # the plain beam's rows share theirs
        for slot in range(6):                                                    # scores are the rows' own log-probabilities
            row, acc = out["tokens"][i, slot], f32(0.0)
            toks = torch.zeros(1, 6, dtype=torch.int32)
            for pos in range(6):
                lg = logits_fn(toks, pos, 1)[0].double()
                acc = f32(acc + f32(float(lg[int(row[pos])] - torch.logsumexp(lg, 0))))
                toks[0, pos] = int(row[pos])
            assert abs(float(acc) - float(out["scores"][i, slot])) < 1e-4


# ---- the check, the record, the helper ---------------------------------------------------------------------------------------------
def test_check_beam_groups():
    assert check_beam_groups() == (1, 0.0) and check_beam_groups(1, 0) == (1, 0.0) and check_beam_groups(1, 0.0, "sample", 5) == (1, 0.0)
    assert check_beam_groups(2, 1, "beam", 6) == (2, 1.0) and check_beam_groups(np.int64(3), np.float32(0.5), "beam", 6) == (3, 0.5)
    assert check_beam_groups(6, 1e6, "beam", 6) == (6, 1e6)
    for bad in (True, False, 2.0, "2", None, [2]):
        with pytest.raises(TypeError, match="num_beam_groups must be an int"):
            check_beam_groups(bad, 1.0)
    for bad in (True, "1", None, [1.0], 1j):
        with pytest.raises(TypeError, match="diversity_penalty must be a real number"):
            check_beam_groups(2, bad)
    for g in (0, -1):
        with pytest.raises(ValueError, match="num_beam_groups must be >= 1"):
            check_beam_groups(g, 1.0)
    for g, b in ((4, 6), (7, 6), (12, 6), (2, 1)):
        with pytest.raises(ValueError, match="must divide beam_size"):
            check_beam_groups(g, 1.0, "beam", b)
    with pytest.raises(ValueError, match='belongs to search="beam"'):
        check_beam_groups(2, 1.0, "sample", 6)
    for lam in (0.0, -1.0, 1e6 + 1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="0 < diversity_penalty <= 1e\\+06"):
            check_beam_groups(2, lam, "beam", 6)
    for lam in (0.5, -0.5, float("nan")):
        with pytest.raises(ValueError, match="needs num_beam_groups > 1"):
            check_beam_groups(1, lam)
    for es in (True, False):
        with pytest.raises(NotImplementedError, match="pool.*follow-up"):
            check_beam_groups(2, 1.0, "beam", 6, es)
    assert check_beam_groups(1, 0.0, "beam", 6, True) == (1, 0.0)
    assert np.isfinite(f32(beam.MAX_DIVERSITY_PENALTY) * f32(hip.MAX_BEAMS))


def test_the_record_key_hash_and_pickle():
    names = [f.name for f in dataclasses.fields(DecodeSettings)]
    assert names == DECODE_FIELDS
    mk = lambda **kw: DecodeSettings.from_kw(dict(search="beam", **kw), 25, 100)
    plain, one, two, three = mk(), mk(num_beam_groups=1, diversity_penalty=0.0), mk(num_beam_groups=2, diversity_penalty=0.5), \
        mk(num_beam_groups=3, diversity_penalty=0.5)
    assert plain == one and hash(plain) == hash(one) and type(one.search) is str and one.num_beam_groups == 1 and one.diversity_penalty == 0.0
    assert len({plain, two, three, mk(num_beam_groups=2, diversity_penalty=0.75)}) == 4
    assert len({hash(plain), hash(two), hash(three)}) == 3
    assert DecodeSettings().num_beam_groups == 1 and DecodeSettings().diversity_penalty == 0.0
    tail = lambda s: (s.early_stopping, s.length_penalty, s.return_logprobs, s.search)
    assert tail(plain) == (None, 0.0, False, "beam") and (plain.num_beam_groups, plain.diversity_penalty) == (1, 0.0)
    assert (two.num_beam_groups, two.diversity_penalty) == (2, 0.5) and dataclasses.replace(two, num_beam_groups=1, diversity_penalty=0.0) == plain
    both = mk(num_beam_groups=3, diversity_penalty=2, length_penalty=1.5, min_len=2)
    assert (both.num_beam_groups, both.diversity_penalty) == (3, 2.0) and tail(both) == (None, 1.5, False, "beam")
    for clone in (copy.copy(both), copy.deepcopy(both), pickle.loads(pickle.dumps(both)), both.compiled("cpu"), dataclasses.replace(both, min_len=2)):
        assert clone == both and hash(clone) == hash(both) and clone.num_beam_groups == 3 and clone.diversity_penalty == 2.0
        assert clone.length_penalty == 1.5 and clone.min_len == 2 and type(clone.search) is str
    same = dataclasses.replace(both, search="beam")                              # every setting is a field of its own: all stay
    assert same == both and same.length_penalty == 1.5 and same.num_beam_groups == 3 and same.diversity_penalty == 2.0
    s = pickle.loads(pickle.dumps(two))
    assert s.search == "beam" and s.num_beam_groups == 2 and s.diversity_penalty == 0.5 and s.length_penalty == 0.0 and s.early_stopping is None
    back = DecodeSettings.from_kw(dict(search=two.search), 25, 100)              # the keywords alone set them
    assert back.num_beam_groups == 1 and type(back.search) is str and type(two.search) is str and back == plain
    with pytest.raises(dataclasses.FrozenInstanceError):
        two.num_beam_groups = 1
    kw = dict(search="beam", num_beam_groups=2, diversity_penalty=1.0)
    DecodeSettings.from_kw(kw, 25, 100)
    assert kw == dict(search="beam", num_beam_groups=2, diversity_penalty=1.0)   # read, not removed


def test_from_kw_checks_them_behind_early_stopping():
    for kw, exc, match in ((dict(num_beam_groups=2.0, search="nope"), ValueError, "search"),
                           (dict(num_beam_groups=2.0, search="beam", early_stopping=1), TypeError, "early_stopping"),
                           (dict(num_beam_groups=2.0, search="beam"), TypeError, "num_beam_groups"),
                           (dict(num_beam_groups=2, diversity_penalty="x", search="beam"), TypeError, "diversity_penalty"),
                           (dict(num_beam_groups=2, diversity_penalty=1.0), ValueError, 'belongs to search="beam"'),
                           (dict(num_beam_groups=2, search="beam"), ValueError, "0 < diversity_penalty"),
                           (dict(diversity_penalty=1.0, search="beam"), ValueError, "needs num_beam_groups > 1"),
                           (dict(num_beam_groups=4, diversity_penalty=1.0, search="beam", beam_size=6), ValueError, "must divide beam_size"),
                           (dict(num_beam_groups=2, diversity_penalty=1.0, search="beam", early_stopping=False), NotImplementedError, "follow-up")):
        with pytest.raises(exc, match=match):
            DecodeSettings.from_kw(kw, 25, 100)


def test_set_beam_groups_and_new_helper(monkeypatch):
    assert list(inspect.signature(BeamSearchHelper.set_beam_groups).parameters) == ["self", "num_beam_groups", "diversity_penalty"]
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    calls = []
    chain = ("set_constraints", "set_search", "set_logprobs", "set_length_penalty", "set_early_stopping", "set_beam_groups")
    for name in chain:
        real = getattr(BeamSearchHelper, name)
        monkeypatch.setattr(BeamSearchHelper, name, lambda self, *a, _n=name, _r=real, **k: (calls.append((_n, a)), _r(self, *a, **k))[1])
    mk = lambda **kw: DecodeSettings.from_kw(dict(search="beam", **kw), 8)
    h = mk(num_beam_groups=2, diversity_penalty=0.5).new_helper(beam_size=4, top_k=5, device="cpu", n_img=3, max_len=8)
    assert [c[0] for c in calls] == list(chain) and calls[-1][1] == (2, 0.5)
    assert h.num_beam_groups == 2 and h.diversity_penalty == 0.5 and h.length_penalty == 0.0 and h.early_stopping is None
    # without a length penalty the table is of ones and the keys exist
    assert torch.equal(h.len_w, torch.ones(9)) and h.len_w is beam.compile_length_weights(0.0, 8, "cpu")
    assert h.keys.shape == (12,) and h.keys.dtype == torch.float32 and not h.keys.any()
    both = mk(num_beam_groups=2, diversity_penalty=0.5, length_penalty=1.0).new_helper(beam_size=4, top_k=5, device="cpu", n_img=3, max_len=8)
    assert torch.equal(both.len_w, LP.weights(1.0, 8)) and both.num_beam_groups == 2
    off = mk().new_helper(beam_size=4, top_k=5, device="cpu", n_img=3, max_len=8)
    assert off.num_beam_groups == 1 and off.diversity_penalty == 0.0 and off.keys is None and off.len_w is None
    with pytest.raises(ValueError, match="must divide beam_size"):               # beam_size is only known here
        mk(num_beam_groups=3, diversity_penalty=0.5).new_helper(beam_size=4, top_k=5, device="cpu", n_img=1, max_len=8)
    with pytest.raises(ValueError, match="must divide beam_size"):
        mk(num_beam_groups=8, diversity_penalty=0.5).new_helper(beam_size=4, top_k=5, device="cpu", n_img=1, max_len=8)
    bare = BeamSearchHelper(1.0, 4, 5, 1, 3, "cpu")
    assert bare.num_beam_groups == 1 and bare.set_beam_groups() is bare and bare.keys is None
    with pytest.raises(ValueError, match='belongs to search="beam"'):
        bare.set_beam_groups(2, 1.0)
    bare.set_search("beam")
    assert bare.set_beam_groups(2, 1.0).keys is not None and bare.set_beam_groups(1).keys is None and bare.len_w is None
    with pytest.raises(NotImplementedError, match="follow-up"):
        BeamSearchHelper(1.0, 4, 5, 1, 3, "cpu").set_search("beam").set_early_stopping(True).set_beam_groups(2, 1.0)
    kept = BeamSearchHelper(1.0, 4, 5, 1, 3, "cpu").set_search("beam").set_length_penalty(1.0).set_beam_groups(2, 1.0).set_beam_groups(1)
    assert kept.keys is not None and torch.equal(kept.len_w, LP.weights(1.0, 25))          # the length penalty keeps its table


# ---- the helper's launches ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_best", "beam_select_best", "beam_select_best_norm", "beam_select_pool",
            "beam_select_groups", "beam_finalize", "beam_finalize_beams", "beam_finalize_pool", "beam_select", "beam_row_sample",
            "beam_pick_logprobs", "beam_record_logprobs", "beam_gather_logprobs")
V, N_IMG, BEAM, MAX_LEN = 100, 2, 4, 8


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    for name in WRAPPERS:
        sig = inspect.signature(getattr(hip, name))

        def recorder(*a, _name=name, _sig=sig, **k):
            bound = _sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append((_name, bound.arguments))
        monkeypatch.setattr(hip, name, recorder)
    return calls


def session(recorded, kw, phase):
    del recorded[:]
    h = DecodeSettings.from_kw(dict(kw, min_len=3), MAX_LEN, V).new_helper(beam_size=BEAM, top_k=5, device="cpu", n_img=N_IMG, max_len=MAX_LEN)
    if phase == "prompted":
        h.set_prompts(torch.zeros(N_IMG, 3, dtype=torch.int64), torch.tensor([1, 3], dtype=torch.int32))
        for s in (1, 2, 3):
            h.step_prompted(torch.zeros(N_IMG * BEAM, V), write_pos=s, t=0, step_index=s, first_sets_ended=True)
        h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=4, t=0, step_index=4)
        pos = 0
    else:
        pos = 2
        h.step(torch.zeros(N_IMG, V), first=True, write_pos=pos, t=0, step_index=pos, first_sets_ended=True)
        for s in (pos + 1, pos + 2):
            h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=s, t=0, step_index=s)
        h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=MAX_LEN, t=0, step_index=MAX_LEN)       # no column: no launch
    h.finalize(1, MAX_LEN, pad_index=7, defer_check=True, beams=True, pos=pos)
    return [n for n, _ in recorded], list(recorded), h


@pytest.mark.parametrize("phase", ("dense", "prompted"))
@pytest.mark.parametrize("extra", ({}, dict(length_penalty=1.0), dict(return_logprobs=True)), ids=("plain", "penalty", "logprobs"))
def test_one_group_is_the_call_without_it_and_more_swap_the_select_only(recorded, phase, extra):
    base = dict(search="beam", **extra)
    select = "beam_select_best_norm" if "length_penalty" in extra else "beam_select_best"
    strip = lambda calls: [(n, {k: v for k, v in a.items() if not torch.is_tensor(v)}) for n, a in calls]
    names0, calls0, _ = session(recorded, base, phase)
    for same_kw in (dict(num_beam_groups=1), dict(num_beam_groups=1, diversity_penalty=0.0)):
        names1, calls1, _ = session(recorded, dict(base, **same_kw), phase)
        assert names1 == names0 and strip(calls1) == strip(calls0) and "beam_select_groups" not in names0
    names2, calls2, h = session(recorded, dict(base, num_beam_groups=2, diversity_penalty=0.75), phase)
    assert names2 == ["beam_select_groups" if n == select else n for n in names0] and select not in names2
    assert names2.count("beam_select_groups") == (4 if phase == "prompted" else 3)
    for (n0, a0), (n2, a2) in zip(calls0, calls2):
        if n2 != "beam_select_groups":
            assert strip([(n2, a2)]) == strip([(n0, a0)])
            continue
        assert a2["n_groups"] == 2 and a2["diversity_penalty"] == 0.75 and a2["first_sets_ended"] is True
        assert a2["keys"] is h.keys and a2["len_w"] is h.len_w and a2["ended"] is h._ended and a2["vals"] is h.vals
        assert torch.equal(a2["len_w"], LP.weights(extra.get("length_penalty", 0.0), MAX_LEN))
        for k in ("n_img", "beam", "first", "write_pos", "t", "step_index", "eos_index"):
            assert a2[k] == a0[k], k
        assert (a2["first_pos"] is h.first_pos) if phase == "prompted" else (a2["first_pos"] is None and a2["first_col"] == 2)
    final = [a for n, a in calls2 if n == "beam_finalize_beams"]
    assert len(final) == 1 and any(v is h.keys for v in final[0].values())       # the order is on the unpenalised keys


# ---- the keyword through the layers -------------------------------------------------------------------------------------------------
def test_keywords_ride_in_kw_and_the_pinned_lists_stay():
    import deephumor_amd.models as M
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder
    fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
    fns += [TransformerDecoder.generate_batch, TransformerDecoder.generate, SelfAttentionTransformerDecoder.generate_batch,
            SelfAttentionTransformerDecoder.generate, LSTMDecoder.generate]
    for fn in fns:
        ps = inspect.signature(fn).parameters
        assert "num_beam_groups" not in ps and "diversity_penalty" not in ps, fn
        assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # (the signatures of every public callable, and the keyword on its way to DecodeSettings.from_kw: test_decode_settings_cpu)
    assert [p.name for p in inspect.signature(LSTMDecoder.generate_batch).parameters.values() if p.kind is not p.VAR_KEYWORD][-1] == "repetition_penalty"
    with pytest.raises(TypeError, match="num_beam_groups"):                    # ... and takes the keyword by name
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="beam", num_beam_groups=2.5, diversity_penalty=1.0)
    with pytest.raises(ValueError, match="must divide beam_size"):
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="beam", beam_size=5, num_beam_groups=2, diversity_penalty=1.0)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_values_fail_before_the_encoder_and_good_ones_reach_the_decoder(kind, monkeypatch):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    monkeypatch.setattr(model, "encode", boom)
    images = torch.zeros(1, 3, 224, 224)
    dec_args = (torch.zeros(1, 256),) if kind == "CaptioningLSTM" else (torch.zeros(1, 512), torch.zeros(1, 49, 512))
    cases = [(dict(search="beam", num_beam_groups=True, diversity_penalty=1.0), TypeError, "num_beam_groups must be an int"),
             (dict(search="beam", num_beam_groups=2, diversity_penalty=None), TypeError, "diversity_penalty must be a real number"),
             (dict(search="beam", num_beam_groups=0), ValueError, "num_beam_groups must be >= 1"),
             (dict(num_beam_groups=2, diversity_penalty=1.0), ValueError, 'belongs to search="beam"'),
             (dict(search="beam", num_beam_groups=2), ValueError, "0 < diversity_penalty"),
             (dict(search="beam", num_beam_groups=2, diversity_penalty=2e6), ValueError, "0 < diversity_penalty"),
             (dict(search="beam", diversity_penalty=0.5), ValueError, "needs num_beam_groups > 1"),
             (dict(search="beam", num_beam_groups=2, diversity_penalty=1.0, early_stopping=True), NotImplementedError, "follow-up")]
    for kw, exc, match in cases:
        for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
            with pytest.raises(exc, match=match):
                call(images, **kw)
        with pytest.raises(exc, match=match):
            model.decode((None,) * len(dec_args), **kw)
        for call in (model.decoder.generate_batch, model.decoder.generate):
            with pytest.raises(exc, match=match):
                call(*dec_args, **kw)
    seen = []

    class Reached(Exception):
        pass

    def from_kw(kw, *a, **k):
        s = real(kw, *a, **k)
        seen.append((s.num_beam_groups, s.diversity_penalty))
        return s
    real = beam.DecodeSettings.from_kw
    monkeypatch.setattr(beam.DecodeSettings, "from_kw", staticmethod(from_kw))
    monkeypatch.setattr(model, "encode", lambda *a: dec_args)
    monkeypatch.setattr(type(model.decoder), "_check_mode", lambda self: (_ for _ in ()).throw(Reached()))
    for call in (model.generate_batch, model.generate):
        for g, lam in ((2, 0.5), (5, 1.0), (1, 0.0)):
            del seen[:]
            with pytest.raises(Reached):
                call(images, search="beam", beam_size=10, num_beam_groups=g, diversity_penalty=lam)
            assert seen and set(seen) == {(g, lam)}


def test_they_are_in_the_graph_key_and_the_table_of_ones_is_uploaded_and_held():
    import deephumor_amd.models as M
    sd, hp = synthetic_sd("CaptioningLSTM")
    model = M.CaptioningLSTM(**hp).eval()

    class Reached(Exception):
        pass

    class Spy(dict):
        def __contains__(self, key):
            raise Reached(key)
    model.__dict__["_graph_overflowed"] = Spy()
    images = torch.zeros(1, 3, 224, 224)

    def key_of(**kw):
        with pytest.raises(Reached) as e:
            model.generate_batch_graphed(images, search="beam", beam_size=6, **kw)
        return e.value.args[0]
    beam._LEN_W_CACHE.clear()
    plain, one = key_of(), key_of(num_beam_groups=1, diversity_penalty=0.0)
    assert plain == one and hash(plain) == hash(one) and "num_beam_groups" not in dict(plain[2]) and "diversity_penalty" not in dict(plain[2])
    assert not beam._LEN_W_CACHE
    two, three, other = key_of(num_beam_groups=2, diversity_penalty=0.5), key_of(num_beam_groups=3, diversity_penalty=0.5), \
        key_of(num_beam_groups=2, diversity_penalty=1)
    assert len({plain, two, three, other}) == 4
    assert ("num_beam_groups", 2) in two[2] and ("num_beam_groups", 3) in three[2] and ("diversity_penalty", 1.0) in other[2]
    ones_t = beam._LEN_W_CACHE[(str(images.device), 0.0, 25)]                     # uploaded in front of the capture
    state = M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None, length_penalty=0.0, device="cpu", num_beam_groups=2)
    assert len(state[8]) == 1 and state[8][0] is ones_t
    assert M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None, length_penalty=0.0, device="cpu")[8] == ()
    assert beam.held_length_weights(0.0, "cpu") == () and beam.held_length_weights(0.0, "cpu", None, 2) == (ones_t,)
    assert "num_beam_groups=settings.num_beam_groups" in inspect.getsource(M.CaptioningLSTM.generate_batch_graphed)


def test_pipeline_and_sharded_callers_carry_the_keywords():
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline

    class Model:
        _hp = {"num_tokens": 50}

        def parameters(self):
            return iter([torch.zeros(1)])
    for kw, exc, match in ((dict(search="beam", num_beam_groups=2.0), TypeError, "num_beam_groups"),
                           (dict(num_beam_groups=2, diversity_penalty=1.0), ValueError, "num_beam_groups"),
                           (dict(search="beam", num_beam_groups=2, diversity_penalty=1.0, early_stopping=True), NotImplementedError, "follow-up")):
        with pytest.raises(exc, match=match):
            CaptionPipeline(Model(), overlap=False, **kw)
    assert "num_beam_groups" in CaptionPipeline.__init__.__doc__ and "num_beam_groups" in dist.generate_sharded.__doc__


def test_group_best_on_a_made_up_result():
    from deephumor_amd.experiments import beams_to_texts, group_best
    idx = torch.tensor([[3, 0, 5, 1, 2, 4], [4, 5, 2, 3, 0, 1]])
    toks = idx[:, :, None].expand(2, 6, 4).clone()
    beams = beam.BeamCaptions(toks, torch.full((2, 6), 4), -torch.arange(6.0).expand(2, 6).clone(), idx, torch.zeros(2, dtype=torch.long),
                              torch.tensor([4, 4]))
    out = group_best(beams, 3)
    assert out.beam_index.tolist() == [[0, 3, 5], [0, 2, 4]] and out.scores.tolist() == [[-1.0, -0.0, -2.0], [-4.0, -2.0, -0.0]]
    assert out.tokens.shape == (2, 3, 4) and out.tokens[:, :, 0].tolist() == out.beam_index.tolist() and out.drawn.tolist() == [1, 2]
    assert torch.equal(GR.group_best(dict(beam_index=idx), 3), torch.tensor([[1, 0, 2], [4, 2, 0]]))

    class Vocab:
        stoi = {"<eos>": 99}
        itos = [str(i) for i in range(10)]
    from deephumor_amd.data import SPECIAL_TOKENS
    Vocab.stoi = {SPECIAL_TOKENS["EOS"]: 99}
    texts = beams_to_texts(out, Vocab)
    assert [t for t, _ in texts[0]] == ["0 0 0 0", "3 3 3 3", "5 5 5 5"]
    for bad in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="num_beam_groups"):
            group_best(beams, bad)


# ---- the C-ABI addition -------------------------------------------------------------------------------------------------------------
ARGS = ["pick_idx", "pick_val", "tokens", "tok_ld", "vals", "keys", "ended", "src", "src_ld", "parent", "hparent", "done", "end_step",
        "n_img", "beam", "first", "first_pos", "first_col", "len_w", "first_sets_ended", "write_pos", "t", "step_index", "eos_index",
        "n_groups", "diversity_penalty", "stream"]


def test_abi_header_table_and_library_agree():
    name = "dh_beam_select_groups"
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[name]
    assert len(args) == len(sig) == len(ARGS)
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    norm = re.search(r"\bint\s+dh_beam_select_best_norm\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    norm_args = [a.strip().split()[-1].lstrip("*") for a in norm.group(1).split(",")]
    assert ARGS == norm_args[:-1] + ["n_groups", "diversity_penalty", "stream"]   # best_norm's arguments plus the two
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    assert _abi.ABI_VERSION == hip.ABI_VERSION == lib.dh_abi_version() == 35       # an entry point was added, no prototype moved
    assert hasattr(lib, name) and hasattr(hip, "beam_select_groups")
    assert len(_abi.SIGNATURES["dh_beam_select_best_norm"]) == 25 and len(_abi.SIGNATURES["dh_beam_select_pool"]) == 30
    ps = list(inspect.signature(hip.beam_select_groups).parameters)
    assert ps == list(inspect.signature(hip.beam_select_best_norm).parameters) + ["n_groups", "diversity_penalty"]


def test_argument_contracts_are_checked_before_any_launch():
    """Pointers are never dereferenced on the host: every case returns DH_ERR_BAD_ARG."""
    lib = hip.load()
    fn = lib.dh_beam_select_groups
    #       pi  pv  tok ld vals keys end src  sld par hpar done estep n  b first fpos col len_w fse wp t step eos G  lam  stream
    good = [64, 64, 64, 8, 64, 64, 64, None, 0, 64, 64, 64, 64, 2, 6, 0, None, 0, 64, 1, 1, 0, 1, 3, 3, 0.5, None]
    assert len(good) == len(ARGS)

    def call(**over):
        a = list(good)
        for k, val in over.items():
            a[ARGS.index(k)] = val
        return fn(*a)
    cases = [{k: None} for k in ("pick_idx", "pick_val", "tokens", "vals", "keys", "ended", "parent", "hparent", "done", "end_step", "len_w")]
    cases += [dict(first_col=-1), dict(n_img=0), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1, n_groups=1), dict(tok_ld=0), dict(t=-1),
              dict(src=64, src_ld=0, t=0), dict(src=64, src_ld=5, t=5), dict(beam=64, n_groups=2, tok_ld=300),
              dict(n_groups=0), dict(n_groups=-1), dict(n_groups=4), dict(n_groups=12), dict(diversity_penalty=0.0),
              dict(diversity_penalty=-1.0), dict(diversity_penalty=float("inf")), dict(diversity_penalty=float("nan"))]
    for over in cases:
        assert call(**over) == 1, over
