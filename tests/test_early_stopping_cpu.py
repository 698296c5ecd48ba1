"""``early_stopping`` on the CPU: the torch-CPU restatement ``tests/early_stopping_ref.py`` on hand-worked cases for every rule, its
invariant against ``length_penalty_ref`` when no candidate is ``<eos>``, the whole-search driver, ``beam.check_early_stopping``, the
settings record, the helper's state and launches, the keyword through the layers and the C-ABI additions."""
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

import beam_search_ref as R
import early_stopping_ref as ES
import length_penalty_ref as LP
from helpers import DECODE_FIELDS, KINDS, synthetic_sd

from deephumor_amd import _abi, _build, hip
from deephumor_amd.models import beam
from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings, check_early_stopping

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 3
NEG = float("-inf")
ONES = LP.weights(0.0, 8)


def step(st, picks, vals, first, pos, mode, len_w=ONES, **kw):
    return ES.select_pool(st, torch.tensor(picks, dtype=torch.int32), torch.tensor(vals, dtype=torch.float32), first, pos, 0, pos, EOS,
                          len_w, mode, **kw)


# ---- the rules, hand-worked ---------------------------------------------------------------------------------------------------------
def test_an_eos_candidate_of_rank_beam_or_more_is_ignored():
    st = ES.new_state(1, 2, 8)
    step(st, [[5, 6], [0, 0]], [[-1.0, -2.0], [0.0, 0.0]], True, 0, False)
    assert st.tokens[:, 0].tolist() == [5, 6] and st.vals.tolist() == [-1.0, -2.0] and st.ended.tolist() == [0, 0] and st.pool_n[0] == 0
    # candidates: 7 at -1.5, <eos> at -4, 8 at -2.25, 9 at -2.5 -- <eos> has rank 3
    step(st, [[7, EOS], [8, 9]], [[-0.5, -3.0], [-0.25, -0.5]], False, 1, False)
    assert st.tokens[:, :2].tolist() == [[5, 7], [6, 8]] and st.vals.tolist() == [-1.5, -2.25] and st.keys.tolist() == [-1.5, -2.25]
    assert st.pool_n[0] == 0 and st.done[0] == 0 and st.parent.tolist() == [0, 1] and st.hparent.tolist() == [0, 1]
    assert bool((st.pool_keys == NEG).all())


def test_a_tie_with_the_worst_key_of_a_full_pool_keeps_the_incumbent():
    st = ES.new_state(1, 2, 8)
    st.tokens[:, 0] = torch.tensor([5, 6])
    st.vals[:], st.keys[:] = torch.tensor([-1.0, -3.0]), torch.tensor([-1.0, -3.0])
    st.pool_tokens[0, 0, :2], st.pool_tokens[0, 1, :3] = torch.tensor([9, EOS]), torch.tensor([9, 9, EOS])
    st.pool_keys[0], st.pool_vals[0], st.pool_len[0], st.pool_n[0] = torch.tensor([-1.0, -2.0]), torch.tensor([-1.0, -2.0]), torch.tensor([2, 3]), 2
    before = {k: v.clone() for k, v in ES.fields(st).items() if k.startswith("pool")}
    # <eos> at -2 has rank 0 and ties with the pool's worst key: not entered
    step(st, [[EOS, 5], [6, 7]], [[-1.0, -1.5], [-0.5, -1.0]], False, 1, False)
    for k, v in before.items():
        assert torch.equal(getattr(st, k), v), k
    assert st.vals.tolist() == [-2.5, -3.5] and st.tokens[:, :2].tolist() == [[5, 5], [6, 6]]
    assert st.done[0] == 1 and st.end_step[0] == 1          # the pool is full and its worst key, -2, is >= the best live key, -2.5
    # ... and strictly above the worst it enters, behind the equal key that stood there first
    st2 = ES.new_state(1, 2, 8)
    for row, key in (([9, EOS], -1.0), ([9, 9, EOS], -2.0)):
        assert ES.pool_insert(st2, 0, torch.tensor(row + [0] * (8 - len(row)), dtype=torch.int32), key, key, len(row))
    assert not ES.pool_insert(st2, 0, torch.zeros(8, dtype=torch.int32), -2.0, -2.0, 1)
    assert ES.pool_insert(st2, 0, torch.tensor([7, 7, 7, EOS, 0, 0, 0, 0], dtype=torch.int32), -1.0, -5.0, 4)
    assert st2.pool_keys[0].tolist() == [-1.0, -1.0] and st2.pool_len[0].tolist() == [2, 4] and st2.pool_vals[0].tolist() == [-1.0, -5.0]
    assert st2.pool_tokens[0, 1, :4].tolist() == [7, 7, 7, EOS] and st2.pool_n[0] == 2


def test_equal_keys_enter_in_the_order_of_the_ranking():
    st = ES.new_state(1, 2, 8)
    step(st, [[5, 6], [0, 0]], [[-1.0, -1.5], [0.0, 0.0]], True, 0, True)
    # both rows offer <eos> at -2: candidate 0 (row 0) ranks in front of candidate 2 (row 1)
    step(st, [[EOS, 7], [EOS, 8]], [[-1.0, -2.0], [-0.5, -2.0]], False, 1, True)
    assert st.pool_n[0] == 2 and st.pool_keys[0].tolist() == [-2.0, -2.0] and st.pool_len[0].tolist() == [2, 2]
    assert st.pool_tokens[0, :, :3].tolist() == [[5, EOS, 0], [6, EOS, 0]]
    assert st.tokens[:, :2].tolist() == [[5, 7], [6, 8]] and st.vals.tolist() == [-3.0, -3.5] and st.ended.tolist() == [0, 0]
    assert st.done[0] == 1 and st.end_step[0] == 1


def test_beam_one_leaves_a_dead_slot_and_is_done_at_once():
    for mode in (True, False):
        st = ES.new_state(2, 1, 4)
        step(st, [[EOS], [5]], [[-0.5], [-0.25]], True, 0, mode)
        assert st.ended.tolist() == [1, 0] and st.vals.tolist() == [NEG, -0.25] and st.keys.tolist() == [NEG, -0.25]
        assert st.tokens[:, 0].tolist() == [0, 5] and st.parent.tolist() == [0, 1] and st.hparent.tolist() == [0, 1]
        assert st.pool_n.tolist() == [1, 0] and st.pool_tokens[0, 0].tolist() == [EOS, 0, 0, 0] and st.pool_len[0, 0] == 1
        assert st.done.tolist() == [1, 0] and st.end_step.tolist() == [0, 0]
        out = ES.finalize_pool(st, 4)
        assert out["tokens"][:, 0].tolist() == [[EOS, 0, 0, 0], [5, 0, 0, 0]] and out["lengths"][:, 0].tolist() == [1, 4]
        assert out["beam_index"][:, 0].tolist() == [-1, 0] and out["scores"][:, 0].tolist() == [-0.5, -0.25]


def test_a_first_step_eos_goes_to_the_pool_and_its_slot_is_dead():
    st = ES.new_state(1, 3, 6, src_len=7)
    st.tokens[:, :2] = torch.tensor([[2, 9]] * 3)              # a prefix of two columns
    step(st, [[5, EOS, 6], [0] * 3, [0] * 3], [[-0.5, -1.0, -1.5], [0.0] * 3, [0.0] * 3], True, 2, False, len_w=LP.weights(1.0, 6), first_col=2)
    assert st.tokens[:, :3].tolist() == [[2, 9, 5], [2, 9, 6], [2, 9, 0]] and st.ended.tolist() == [0, 0, 1]
    assert st.vals.tolist() == [-0.5, -1.5, NEG] and st.keys.tolist() == [-0.5, -1.5, NEG]
    # (the dead slot of a FIRST step points at the base row, the only one with decoder state behind it; later ones at themselves)
    assert st.parent.tolist() == [0, 0, 0] and st.hparent.tolist() == [0, 0, 0] and st.src[:, 0].tolist() == [0, 0, 0]
    assert st.pool_n[0] == 1 and st.pool_tokens[0, 0].tolist() == [2, 9, EOS, 0, 0, 0] and st.pool_len[0, 0] == 3
    assert st.pool_keys[0, 0] == -1.0 and st.pool_vals[0, 0] == -1.0 and st.done[0] == 0
    # the dead slot brings one candidate at -inf, which takes no slot: two live rows fill the three slots
    step(st, [[7, 8, 9], [10, 11, 12], [0, 0, 0]], [[-0.5, -1.0, -4.0], [-0.5, -0.75, -1.0], [0.0] * 3], False, 3, False,
         len_w=LP.weights(1.0, 6), first_col=2)
    assert st.tokens[:, 2:4].tolist() == [[5, 7], [5, 8], [6, 10]] and st.ended.tolist() == [0, 0, 0]
    assert st.vals.tolist() == [-1.0, -1.5, -2.0] and st.keys.tolist() == [-0.5, -0.75, -1.0]          # L = 2: w = 0.5


def test_an_eos_at_minus_infinity_is_neither_pooled_nor_kept():
    """``min_len`` bans ``<eos>``: a TOO_FEW row can still list it, at ``-inf``."""
    st = ES.new_state(1, 2, 4)
    step(st, [[5, EOS], [0, 0]], [[-1.0, NEG], [0.0, 0.0]], True, 0, True)
    assert st.pool_n[0] == 0 and st.ended.tolist() == [0, 1] and st.tokens[:, 0].tolist() == [5, 0] and st.vals.tolist() == [-1.0, NEG]
    assert st.done[0] == 0
    # a token at -inf takes no slot either (dh_beam_row_best's dead picks): the slot is dead
    step(st, [[6, 0], [0, 0]], [[-0.5, NEG], [0.0, 0.0]], False, 1, True)
    assert st.tokens[:, :2].tolist() == [[5, 6], [0, 0]] and st.ended.tolist() == [0, 1] and st.parent.tolist() == [0, 1]


def run_two_beams(mode):
    st = ES.new_state(1, 2, 8)
    steps = [([[5, 6], [0, 0]], [[-0.5, -1.0], [0.0, 0.0]]),
             ([[EOS, 7], [EOS, 8]], [[-0.25, -2.0], [-0.5, -0.25]]),       # <eos> -0.75 (rank 0), 8 -1.25, <eos> -1.5 (rank 2), 7 -2.5
             ([[9, EOS], [10, 11]], [[-0.125, -0.25], [-0.5, -1.0]]),      # 9 -1.375, <eos> -1.5 (rank 1), 10 -3, 11 -3.5
             ([[EOS, 12], [13, 14]], [[-0.0625, -3.0], [-0.125, -0.25]])]  # <eos> -1.4375, 13 -3.125, 14 -3.25, 12 -4.375
    ends = None
    for pos, (picks, vals) in enumerate(steps):
        step(st, picks, vals, pos == 0, pos, mode)
        if st.done[0] and ends is None:
            ends = pos
            break
    return st, ends


def test_true_stops_when_the_pool_is_full_and_false_when_no_live_beam_can_enter():
    st, ends = run_two_beams(True)
    assert ends == 2 and st.end_step[0] == 2 and st.pool_keys[0].tolist() == [-0.75, -1.5] and st.keys[0] == -1.375
    out = ES.finalize_pool(st, 8)
    assert out["tokens"][0, :, :4].tolist() == [[5, EOS, 0, 0], [6, 8, EOS, 0]] and out["lengths"][0].tolist() == [2, 3]
    assert out["beam_index"][0].tolist() == [-1, -1] and out["scores"][0].tolist() == [-0.75, -1.5] and out["row_lengths"].tolist() == [2]
    st, ends = run_two_beams(False)
    assert ends == 3 and st.end_step[0] == 3 and st.pool_keys[0].tolist() == [-0.75, -1.4375] and st.pool_len[0].tolist() == [2, 4]
    out = ES.finalize_pool(st, 8)
    assert out["tokens"][0, :, :5].tolist() == [[5, EOS, 0, 0, 0], [6, 8, 9, EOS, 0]] and out["drawn"].tolist() == [0]


def test_finalize_offers_the_live_slots_of_an_image_that_is_not_done():
    st = ES.new_state(2, 3, 5, pad_index=0)
    st.tokens[:] = torch.arange(30, dtype=torch.int32).view(6, 5) + 10
    st.keys[:] = torch.tensor([-1.0, -2.0, NEG, -1.0, -0.5, -3.0])
    st.ended[2] = 1
    st.pool_tokens[0, 0, :2], st.pool_keys[0, 0], st.pool_len[0, 0], st.pool_n[0] = torch.tensor([7, EOS]), -2.0, 2, 1
    st.pool_tokens[1, :, :3] = torch.tensor([[7, 8, EOS]] * 3)
    st.pool_keys[1], st.pool_len[1], st.pool_n[1] = torch.tensor([-0.5, -1.0, -2.0]), torch.tensor([3, 3, 3]), 3
    out = ES.finalize_pool(st, 5, pad_index=9)
    # image 0: the pool's -2 stands in front of live slot 1's -2 (it arrived first); the dead slot is not offered
    assert out["scores"][0].tolist() == [-1.0, -2.0, -2.0] and out["beam_index"][0].tolist() == [0, -1, 1]
    assert out["tokens"][0].tolist() == [[10, 11, 12, 13, 14], [7, EOS, 9, 9, 9], [15, 16, 17, 18, 19]] and out["lengths"][0].tolist() == [5, 2, 5]
    # image 1: a full pool is entered only strictly above its worst key; equal keys stand behind the pool's
    assert out["scores"][1].tolist() == [-0.5, -0.5, -1.0] and out["beam_index"][1].tolist() == [-1, 1, -1]
    st.done[1] = 1                                       # a done image offers nothing
    assert ES.finalize_pool(st, 5)["beam_index"][1].tolist() == [-1, -1, -1]
    st.pool_n[0], st.ended[:3] = 0, 1                    # nothing at all: the slots follow at -inf
    out = ES.finalize_pool(st, 4)
    assert out["scores"][0].tolist() == [NEG] * 3 and out["beam_index"][0].tolist() == [0, 1, 2] and out["lengths"][0].tolist() == [4] * 3


# ---- the invariant: without <eos> it is the length-penalty select ------------------------------------------------------------------
@pytest.mark.parametrize("beam_size", (1, 2, 5))
@pytest.mark.parametrize("lp", (0.0, 1.0, -1.0))
def test_without_eos_candidates_it_is_select_best_norm(beam_size, lp):
    g = torch.Generator().manual_seed(100 * beam_size + int(lp * 2))
    n, m = 4, 7
    a, b = ES.new_state(n, beam_size, m, src_len=m + 1), LP.new_state(n, beam_size, m, src_len=m + 1)
    w = LP.weights(lp, m)
    fp = None
    for pos in range(m):
        rows = n * beam_size
        picks = torch.stack([torch.randperm(30, generator=g)[:beam_size] + 4 for _ in range(rows)]).to(torch.int32)
        vals = torch.sort(torch.randint(-8, 0, (rows, beam_size), generator=g).float() * 0.25, dim=1, descending=True).values
        for mode in (True,):
            ES.select_pool(a, picks, vals, pos == 0, pos, pos, pos, EOS, w, mode, first_col=0, first_pos=fp)
        LP.select_best_norm(b, picks, vals, pos == 0, pos, pos, pos, EOS, w, first_col=0, first_pos=fp)
        for k, v in b.fields().items():
            assert torch.equal(getattr(a, k), v), (k, pos)
        assert torch.equal(a.keys.view(torch.int32), b.keys.view(torch.int32)) and int(a.pool_n.sum()) == 0
    got, want = ES.finalize_pool(a, m), LP.finalize_norm(b, 1, m, 0, EOS)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def logits_fn(v=40, boost=1.5, seed=5):
    """Logits that depend on the row's history alone (a hash of its tokens seeds them), ``<eos>`` raised by ``boost``."""
    def fn(tokens, pos, rows_per_img):
        out = torch.empty(tokens.shape[0], v)
        for r in range(tokens.shape[0]):
            h = seed
            for tk in tokens[r, :pos].tolist():
                h = (h * 1000003 + tk + 1) % (2 ** 31 - 1)
            out[r] = torch.randn(v, generator=torch.Generator().manual_seed(h + 7919 * (r // rows_per_img if rows_per_img > 1 else r)))
        out[:, EOS] += boost
        return out
    return fn


def test_the_driver_fills_pools_with_mixed_lengths_and_ends_images_at_different_steps():
    n, b, m = 6, 3, 10
    ends = {}
    for lp in (0.0, 1.0):
        for mode in (True, False):
            trace = []
            out, err, st = ES.beam_search_pool(logits_fn(), n, b, m, lp, mode, trace=trace)
            assert err == 0 and out["drawn"].tolist() == [0] * n
            s = out["scores"]
            assert bool((s[:, :-1] >= s[:, 1:]).all()) and torch.equal(out["row_lengths"], out["lengths"][:, 0])
            first_done = [next((pos for pos, d in trace if d[i]), None) for i in range(n)]
            ends[lp, mode] = first_done
            assert any(e is not None and e < m - 1 for e in first_done), (lp, mode)       # some image is done early
            assert len({e for e in first_done}) > 1, (lp, mode)                           # ... and not all at the same step
            pooled = [sorted(set(st.pool_len[i, :int(st.pool_n[i])].tolist())) for i in range(n)]
            assert any(len(p) >= 2 for p in pooled), (lp, mode)                           # a pool holds two lengths
            for i in range(n):                                                            # every pooled row ends in its <eos>
                for j in range(int(st.pool_n[i])):
                    ln = int(st.pool_len[i, j])
                    assert st.pool_tokens[i, j, ln - 1] == EOS and EOS not in st.pool_tokens[i, j, :ln - 1].tolist()
                keys = st.pool_keys[i, :int(st.pool_n[i])]
                assert bool((keys[:-1] >= keys[1:]).all())
                if st.done[i]:
                    assert int(st.pool_n[i]) == b and out["beam_index"][i].tolist() == [-1] * b
    last = lambda e: [m if x is None else x for x in e]
    for lp in (0.0, 1.0):
        assert all(f >= t for t, f in zip(last(ends[lp, True]), last(ends[lp, False])))
    assert any(f > t for t, f in zip(last(ends[1.0, True]), last(ends[1.0, False])))     # False ends later than True under penalty 1
    print("first done step per image:", ends)


# ---- the check, the record, the helper ---------------------------------------------------------------------------------------------
def test_check_early_stopping():
    assert check_early_stopping(None) is None and check_early_stopping(True) is True and check_early_stopping(False) is False
    assert check_early_stopping(None, "sample") is None and check_early_stopping(False, "beam") is False
    for bad in (0, 1, 1.0, "never", "True", [True], np.bool_(True), torch.tensor(True)):
        with pytest.raises(TypeError, match="early_stopping must be None, True or False"):
            check_early_stopping(bad)
    for value in (True, False):
        with pytest.raises(ValueError, match='belongs to search="beam"'):
            check_early_stopping(value, "sample")
        with pytest.raises(NotImplementedError, match="return_attention=True.*follow-up"):
            check_early_stopping(value, "beam", return_attention=True)
        with pytest.raises(NotImplementedError, match="return_logprobs=True.*follow-up"):
            check_early_stopping(value, "beam", return_logprobs=True)
    assert check_early_stopping(None, "sample", True, True) is None


def test_the_record_key_hash_and_pickle():
    names = [f.name for f in dataclasses.fields(DecodeSettings)]
    assert names == DECODE_FIELDS
    plain, none = DecodeSettings.from_kw(dict(search="beam"), 25, 100), DecodeSettings.from_kw(dict(search="beam", early_stopping=None), 25, 100)
    on, off = (DecodeSettings.from_kw(dict(search="beam", early_stopping=v), 25, 100) for v in (True, False))
    assert plain == none and hash(plain) == hash(none) and type(none.search) is str and none.early_stopping is None
    assert len({plain, on, off}) == 3 and on.early_stopping is True and off.early_stopping is False and DecodeSettings().early_stopping is None
    tail = lambda s: (s.early_stopping, s.length_penalty, s.return_logprobs, s.search)
    assert tail(on) == (True, 0.0, False, "beam") and tail(off) == (False, 0.0, False, "beam") and tail(plain) == (None, 0.0, False, "beam")
    assert dataclasses.replace(on, early_stopping=None) == plain == dataclasses.replace(off, early_stopping=None)
    both = DecodeSettings.from_kw(dict(search="beam", early_stopping=False, length_penalty=1.5, min_len=2), 25, 100)
    assert tail(both) == (False, 1.5, False, "beam") and both.length_penalty == 1.5
    for clone in (copy.copy(both), copy.deepcopy(both), pickle.loads(pickle.dumps(both)), both.compiled("cpu"), dataclasses.replace(both, min_len=2)):
        assert clone == both and hash(clone) == hash(both) and clone.early_stopping is False and clone.length_penalty == 1.5
        assert clone.min_len == 2 and type(clone.search) is str
    same = dataclasses.replace(both, search="beam")                              # every setting is a field of its own: all stay
    assert same == both and same.early_stopping is False and same.length_penalty == 1.5
    s = pickle.loads(pickle.dumps(on))
    assert s.search == "beam" and s.early_stopping is True and s.length_penalty == 0.0
    back = DecodeSettings.from_kw(dict(search=on.search), 25, 100)              # the keyword alone sets it
    assert back.early_stopping is None and type(back.search) is str and type(on.search) is str and back == plain
    with pytest.raises(dataclasses.FrozenInstanceError):
        on.early_stopping = None
    kw = dict(search="beam", early_stopping=True)
    DecodeSettings.from_kw(kw, 25, 100)
    assert kw == dict(search="beam", early_stopping=True)                        # read, not removed


def test_from_kw_checks_it_last_and_refuses_the_gathers():
    for kw, exc, match in ((dict(early_stopping=1, search="nope"), ValueError, "search"),
                           (dict(early_stopping=1, return_logprobs=1), TypeError, "return_logprobs"),
                           (dict(early_stopping=1, search="beam", length_penalty="x"), TypeError, "length_penalty"),
                           (dict(early_stopping=1, search="beam"), TypeError, "early_stopping"),
                           (dict(early_stopping=0, search="beam"), TypeError, "early_stopping"),
                           (dict(early_stopping=True), ValueError, 'belongs to search="beam"'),
                           (dict(early_stopping=False, search="sample"), ValueError, 'belongs to search="beam"'),
                           (dict(early_stopping=True, search="beam", return_logprobs=True), NotImplementedError, "return_logprobs"),
                           (dict(early_stopping=False, search="beam", return_attention=True), NotImplementedError, "return_attention")):
        with pytest.raises(exc, match=match):
            DecodeSettings.from_kw(kw, 25, 100)


def test_set_early_stopping_and_new_helper(monkeypatch):
    assert list(inspect.signature(BeamSearchHelper.set_early_stopping).parameters) == ["self", "early_stopping"]
    assert list(inspect.signature(BeamSearchHelper.set_length_penalty).parameters) == ["self", "length_penalty"]
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    calls = []
    for name in ("set_constraints", "set_search", "set_logprobs", "set_length_penalty", "set_early_stopping"):
        real = getattr(BeamSearchHelper, name)
        monkeypatch.setattr(BeamSearchHelper, name, lambda self, *a, _n=name, _r=real, **k: (calls.append((_n, a)), _r(self, *a, **k))[1])
    h = DecodeSettings.from_kw(dict(search="beam", early_stopping=False), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert [c[0] for c in calls] == ["set_constraints", "set_search", "set_logprobs", "set_length_penalty", "set_early_stopping"]
    assert calls[-1][1] == (False,) and h.early_stopping is False and h.length_penalty == 0.0
    assert h.pool_tokens.shape == (3, 2, 8) and h.pool_tokens.dtype == torch.int32 and not h.pool_tokens.any()
    assert h.pool_keys.shape == h.pool_vals.shape == h.pool_len.shape == (3, 2) and h.pool_n.shape == (3,)
    assert bool((h.pool_keys == NEG).all()) and not h.pool_vals.any() and not h.pool_len.any() and not h.pool_n.any()
    assert h.pool_keys.dtype == h.pool_vals.dtype == torch.float32 and h.pool_len.dtype == h.pool_n.dtype == torch.int32
    # one arena: the pieces follow one another
    assert h.pool_keys.data_ptr() == h.pool_tokens.data_ptr() + 4 * 48 and h.pool_n.data_ptr() == h.pool_keys.data_ptr() + 4 * 18
    # without a penalty the table is of ones -- compile_length_weights(0.0, max_len) -- and the keys exist
    assert torch.equal(h.len_w, torch.ones(9)) and h.len_w is beam.compile_length_weights(0.0, 8, "cpu") and h.keys.shape == (6,)
    both = DecodeSettings.from_kw(dict(search="beam", early_stopping=True, length_penalty=1.0), 8).new_helper(beam_size=2, top_k=5, device="cpu",
                                                                                                            n_img=3, max_len=8)
    assert torch.equal(both.len_w, LP.weights(1.0, 8)) and both.early_stopping is True
    off = DecodeSettings.from_kw(dict(search="beam"), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert off.early_stopping is None and off.pool_tokens is None and off.pool_n is None and off.keys is None and off.len_w is None
    bare = BeamSearchHelper(1.0, 2, 5, 1, 3, "cpu")
    assert bare.early_stopping is None and bare.set_early_stopping(None) is bare and bare.pool_keys is None
    with pytest.raises(ValueError, match='belongs to search="beam"'):
        bare.set_early_stopping(True)
    with pytest.raises(TypeError, match="early_stopping"):
        bare.set_search("beam").set_early_stopping(1)
    assert bare.set_early_stopping(True).pool_n is not None and bare.set_early_stopping(None).pool_n is None and bare.keys is None
    with pytest.raises(NotImplementedError, match="return_logprobs"):
        BeamSearchHelper(1.0, 2, 5, 1, 3, "cpu").set_search("beam").set_logprobs(True).set_early_stopping(False)


# ---- the helper's launches ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_best", "beam_select_best", "beam_select_best_norm", "beam_select_pool",
            "beam_finalize", "beam_finalize_beams", "beam_finalize_pool", "beam_select", "beam_row_sample")
V, N_IMG, BEAM, MAX_LEN = 100, 2, 2, 8


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


def session(recorded, kw, phase, beams=True):
    del recorded[:]
    h = DecodeSettings.from_kw(dict(kw, min_len=3), MAX_LEN, V).new_helper(beam_size=BEAM, top_k=3, device="cpu", n_img=N_IMG, max_len=MAX_LEN)
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
    res = h.finalize(1, MAX_LEN, pad_index=7, defer_check=True, beams=beams, pos=pos)
    return [n for n, _ in recorded], list(recorded), h, res


@pytest.mark.parametrize("phase", ("dense", "prompted"))
@pytest.mark.parametrize("lp", (0.0, 1.0))
def test_none_is_the_call_without_it_and_a_value_swaps_the_select_and_the_finalize(recorded, phase, lp):
    base = dict(search="beam", length_penalty=lp)
    select = "beam_select_best_norm" if lp else "beam_select_best"
    names0, calls0, h0, _ = session(recorded, base, phase)
    names_none, calls_none, _, _ = session(recorded, dict(base, early_stopping=None), phase)
    strip = lambda calls: [(n, {k: v for k, v in a.items() if not torch.is_tensor(v)}) for n, a in calls]
    assert names_none == names0 and strip(calls_none) == strip(calls0) and "beam_select_pool" not in names0 and "beam_finalize_pool" not in names0
    for mode in (True, False):
        names1, calls1, h1, res = session(recorded, dict(base, early_stopping=mode), phase)
        swap = {select: "beam_select_pool", "beam_finalize_beams": "beam_finalize_pool"}
        assert names1 == [swap.get(n, n) for n in names0] and names1[-1] == "beam_finalize_pool"
        assert names1.count("beam_select_pool") == (4 if phase == "prompted" else 3)
        for (n0, a0), (n1, a1) in zip(calls0, calls1):
            if n1 == "beam_select_pool":
                assert a1["stop_when_full"] is mode and a1["keys"] is h1.keys and a1["len_w"] is h1.len_w and a1["ended"] is h1._ended
                for k in ("pool_tokens", "pool_keys", "pool_vals", "pool_len", "pool_n", "tokens", "vals", "done", "end_step", "pick_idx"):
                    assert a1[k] is getattr(h1, k), k
                for k in ("n_img", "beam", "first", "write_pos", "t", "step_index", "eos_index"):
                    assert a1[k] == a0[k], k
                assert (a1["first_pos"] is h1.first_pos) if phase == "prompted" else (a1["first_pos"] is None and a1["first_col"] == 2)
            elif n1 == "beam_finalize_pool":
                assert a1["keys"] is h1.keys and a1["ended"] is h1._ended and a1["pool_n"] is h1.pool_n and a1["full_len"] == MAX_LEN
                assert a1["pad_index"] == 7 and a1["out_tokens"].shape == (N_IMG, BEAM, MAX_LEN)
            else:
                assert strip([(n1, a1)]) == strip([(n0, a0)])
        assert isinstance(res.captions, beam.BeamCaptions)
        pair = session(recorded, dict(base, early_stopping=mode), phase, beams=False)[3].captions
        assert isinstance(pair, tuple) and not isinstance(pair, beam.BeamCaptions) and pair[0].shape == (N_IMG, MAX_LEN) and pair[1].shape == (N_IMG,)
    with pytest.raises(NotImplementedError, match="return_attention"):
        h1.finalize(0, MAX_LEN, attn_w=torch.zeros(1, 4, 2))


# ---- the keyword through the layers -------------------------------------------------------------------------------------------------
def test_keyword_rides_in_kw_and_the_pinned_lists_stay():
    import deephumor_amd.models as M
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder
    fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
    fns += [TransformerDecoder.generate_batch, TransformerDecoder.generate, SelfAttentionTransformerDecoder.generate_batch,
            SelfAttentionTransformerDecoder.generate, LSTMDecoder.generate]
    for fn in fns:
        ps = inspect.signature(fn).parameters
        assert "early_stopping" not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # (the signatures of every public callable, and the keyword on its way to DecodeSettings.from_kw: test_decode_settings_cpu)
    assert [p.name for p in inspect.signature(LSTMDecoder.generate_batch).parameters.values() if p.kind is not p.VAR_KEYWORD][-1] == "repetition_penalty"
    assert [f.name for f in dataclasses.fields(DecodeSettings)] == DECODE_FIELDS
    with pytest.raises(TypeError, match="early_stopping"):                     # ... and takes the keyword by name
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="beam", early_stopping=1)


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
    cases = [(dict(search="beam", early_stopping=1), TypeError, "early_stopping must be None, True or False"),
             (dict(search="beam", early_stopping=0), TypeError, "early_stopping must be None, True or False"),
             (dict(search="beam", early_stopping="never"), TypeError, "early_stopping must be None, True or False"),
             (dict(early_stopping=True), ValueError, 'belongs to search="beam"'),
             (dict(search="sample", early_stopping=False), ValueError, 'belongs to search="beam"'),
             (dict(search="beam", early_stopping=True, return_logprobs=True), NotImplementedError, "return_logprobs=True.*follow-up")]
    if kind == "CaptioningTransformer":
        cases.append((dict(search="beam", early_stopping=False, return_attention=True), NotImplementedError, "return_attention=True.*follow-up"))
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
        seen.append(s.early_stopping)
        return s
    real = beam.DecodeSettings.from_kw
    monkeypatch.setattr(beam.DecodeSettings, "from_kw", staticmethod(from_kw))
    monkeypatch.setattr(model, "encode", lambda *a: dec_args)
    monkeypatch.setattr(type(model.decoder), "_check_mode", lambda self: (_ for _ in ()).throw(Reached()))
    for call in (model.generate_batch, model.generate):
        for value in (True, False, None):
            del seen[:]
            with pytest.raises(Reached):
                call(images, search="beam", early_stopping=value)
            assert seen and set(seen) == {value}
    del seen[:]
    with pytest.raises(Reached):
        model.decode(dec_args, search="beam", early_stopping=False, length_penalty=1.0)
    assert seen == [False]


def test_it_is_in_the_graph_key_and_its_table_is_uploaded_and_held(monkeypatch):
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
            model.generate_batch_graphed(images, **kw)
        return e.value.args[0]
    beam._LEN_W_CACHE.clear()
    plain, none, on, off = (key_of(search="beam"), key_of(search="beam", early_stopping=None), key_of(search="beam", early_stopping=True),
                            key_of(search="beam", early_stopping=False))
    assert plain == none and hash(plain) == hash(none) and len({plain, on, off}) == 3 and "early_stopping" not in dict(plain[2])
    assert ("early_stopping", True) in on[2] and ("early_stopping", False) in off[2]
    assert (str(images.device), 0.0, 25) in beam._LEN_W_CACHE               # the table of ones, uploaded in front of the capture
    ones = beam._LEN_W_CACHE[(str(images.device), 0.0, 25)]
    state = M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None, length_penalty=0.0, device="cpu", early_stopping=False)
    assert len(state[8]) == 1 and state[8][0] is ones
    assert M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None, length_penalty=0.0, device="cpu")[8] == ()
    assert beam.held_length_weights(0.0, "cpu") == () and beam.held_length_weights(0.0, "cpu", True) == (ones,)
    src = inspect.getsource(M.CaptioningLSTM.generate_batch_graphed)
    assert "early_stopping=settings.early_stopping" in src


def test_pipeline_and_sharded_callers_carry_the_keyword():
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline

    class Model:
        _hp = {"num_tokens": 50}

        def parameters(self):
            return iter([torch.zeros(1)])
    for kw, exc in ((dict(search="beam", early_stopping=1), TypeError), (dict(early_stopping=True), ValueError),
                    (dict(search="beam", early_stopping=True, return_logprobs=True), NotImplementedError)):
        with pytest.raises(exc, match="early_stopping"):
            CaptionPipeline(Model(), overlap=False, **kw)
    assert 'pop("early_stopping"' not in inspect.getsource(CaptionPipeline.__init__)
    assert "early_stopping" in CaptionPipeline.__init__.__doc__ and "early_stopping" in dist.generate_sharded.__doc__


# ---- the C-ABI additions ------------------------------------------------------------------------------------------------------------
SELECT_ARGS = ["pick_idx", "pick_val", "tokens", "tok_ld", "vals", "keys", "ended", "src", "src_ld", "parent", "hparent", "done", "end_step",
               "pool_tokens", "pool_keys", "pool_vals", "pool_len", "pool_n", "n_img", "beam", "first", "first_pos", "first_col", "len_w",
               "stop_when_full", "write_pos", "t", "step_index", "eos_index", "stream"]
FINAL_ARGS = ["tokens", "tok_ld", "keys", "ended", "done", "pool_tokens", "pool_keys", "pool_len", "pool_n", "out_tokens", "out_ld", "out_len",
              "out_score", "out_index", "out_drawn", "out_row_len", "n_img", "beam", "full_len", "pad_index", "stream"]


@pytest.mark.parametrize("name,names", (("dh_beam_select_pool", SELECT_ARGS), ("dh_beam_finalize_pool", FINAL_ARGS)))
def test_abi_header_table_and_library_agree(name, names):
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[name]
    assert len(args) == len(sig) == len(names)
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == names
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == lib.dh_abi_version() == 35
    assert hasattr(lib, name) and hasattr(hip, name[3:])
    assert len(_abi.SIGNATURES["dh_beam_select_best_norm"]) == 25 and len(_abi.SIGNATURES["dh_beam_finalize_beams"]) == 26      # additive


def call_with(fn, names, good, **over):
    a = list(good)
    for k, val in over.items():
        a[names.index(k)] = val
    return fn(*a)


def test_argument_contracts_are_checked_before_any_launch():
    """Pointers are never dereferenced on the host: every case returns DH_ERR_BAD_ARG."""
    lib = hip.load()
    #       pi  pv  tok ld vals keys end src  sld par hpar done estep ptok pkey pval plen pn  n  b first fpos col len_w stop wp t step eos stream
    good = [64, 64, 64, 8, 64, 64, 64, None, 0, 64, 64, 64, 64, 64, 64, 64, 64, 64, 2, 3, 0, None, 0, 64, 1, 1, 0, 1, 3, None]
    assert len(good) == len(SELECT_ARGS)
    cases = [{k: None} for k in SELECT_ARGS if k.startswith("pool_") or k in ("pick_idx", "pick_val", "tokens", "vals", "keys", "ended", "parent",
                                                                              "hparent", "done", "end_step", "len_w")]
    cases += [dict(first_col=-1), dict(n_img=0), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1), dict(tok_ld=0), dict(t=-1), dict(step_index=-1),
              dict(write_pos=-1), dict(write_pos=8), dict(stop_when_full=2), dict(stop_when_full=-1), dict(src=64, src_ld=0, t=0),
              dict(src=64, src_ld=5, t=5), dict(beam=64, tok_ld=300, write_pos=1), dict(first_pos=64, beam=64, tok_ld=300), dict(len_w=None, first_pos=64)]
    for over in cases:
        assert call_with(lib.dh_beam_select_pool, SELECT_ARGS, good, **over) == 1, over
    #       tok ld keys end done ptok pkey plen pn  out old olen osc oidx odr orow n  b full pad stream
    good = [64, 8, 64, 64, 64, 64, 64, 64, 64, 64, 8, 64, 64, 64, 64, 64, 2, 3, 8, 0, None]
    assert len(good) == len(FINAL_ARGS)
    cases = [{k: None} for k, v in zip(FINAL_ARGS, good) if v == 64]
    cases += [dict(n_img=0), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1), dict(tok_ld=0), dict(out_ld=0), dict(full_len=-1)]
    assert len(cases) == 14 + 6
    for over in cases:
        assert call_with(lib.dh_beam_finalize_pool, FINAL_ARGS, good, **over) == 1, over
