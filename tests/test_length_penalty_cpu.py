"""``length_penalty`` on the CPU: ``beam.check_length_penalty``, the settings record, the helper's launches, the C-ABI addition, the
keyword through the layers -- and the torch-CPU restatement ``tests/length_penalty_ref.py``: equal to ``beam_search_ref`` at 0.0, and
hand-worked cases where the penalty changes the winner and where two keys tie."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beam_search_ref as R
import length_penalty_ref as LP
from helpers import DECODE_FIELDS, KINDS, synthetic_sd

from deephumor_amd import _abi, _build, hip
from deephumor_amd.models import beam
from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings, check_length_penalty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 3


# ---- the check ---------------------------------------------------------------------------------------------------------------------
def test_check_length_penalty():
    assert check_length_penalty(0.0) == 0.0 and check_length_penalty(1) == 1.0 and isinstance(check_length_penalty(1), float)
    assert check_length_penalty(-2.5, 25, "beam") == -2.5 and check_length_penalty(8, 25, "beam") == 8.0
    assert check_length_penalty(np.float32(0.5)) == 0.5
    assert str(check_length_penalty(-0.0)) == "0.0"                          # one key for the two zeros
    for bad in (True, False, None, "1", [1.0], (1.0,), torch.tensor(1.0), 1j):
        with pytest.raises(TypeError, match="length_penalty must be a real number"):
            check_length_penalty(bad)
    for bad in (float("nan"), float("inf"), float("-inf"), 8.5, -9, 1e30):
        with pytest.raises(ValueError, match="length_penalty"):
            check_length_penalty(bad)
    # a weight that is not a normal fp32: 1e5 ** -8 = 1e-40 is subnormal, 1e5 ** 8 = 1e40 is above the largest fp32
    for bad in (8.0, -8.0):
        assert check_length_penalty(bad, 1000, "beam") == bad                # (1000 ** 8 = 1e24 and its inverse are fine)
        with pytest.raises(ValueError, match="normal fp32 range"):
            check_length_penalty(bad, 100000, "beam")
    with pytest.raises(ValueError, match='belongs to search="beam"'):
        check_length_penalty(1.0, 25, "sample")
    assert check_length_penalty(0.0, 25, "sample") == 0.0 and check_length_penalty(0, 10 ** 6, "sample") == 0.0


def test_the_engine_table_is_the_restatement_table():
    for lp in (-8.0, -1.0, -0.3, 0.0, 0.5, 0.7, 1.0, 2.0, 3.3, 8.0):
        for max_len in (1, 12, 300):
            w = beam.length_weights(lp, max_len)
            assert w.dtype == torch.float32 and w.shape == (max_len + 1,) and float(w[0]) == 1.0 and float(w[1]) == 1.0
            assert torch.equal(w, LP.weights(lp, max_len)), (lp, max_len)
    w = beam.length_weights(1.0, 4).tolist()
    assert w == [1.0, 1.0, 0.5, float(np.float32(1.0 / 3.0)), 0.25]
    assert beam.length_weights(-1.0, 4).tolist() == [1.0, 1.0, 2.0, 3.0, 4.0]
    a = beam.compile_length_weights(1.0, 4, "cpu")
    assert a is beam.compile_length_weights(1.0, 4, "cpu") and a is not beam.compile_length_weights(1.0, 5, "cpu")      # one upload


# ---- the settings record -----------------------------------------------------------------------------------------------------------
def test_settings_carry_it_outside_the_field_list():
    names = [f.name for f in DecodeSettings.__dataclass_fields__.values()]
    assert names == DECODE_FIELDS
    plain = DecodeSettings.from_kw({}, 25, 100)
    off = DecodeSettings.from_kw(dict(length_penalty=0.0), 25, 100)
    off_beam, beam_plain = DecodeSettings.from_kw(dict(search="beam", length_penalty=0), 25, 100), DecodeSettings.from_kw(dict(search="beam"), 25, 100)
    on = DecodeSettings.from_kw(dict(search="beam", length_penalty=1.0), 25, 100)
    assert plain.length_penalty == 0.0 and DecodeSettings().length_penalty == 0.0 and on.length_penalty == 1.0
    assert plain == off and hash(plain) == hash(off) and off_beam == beam_plain and hash(off_beam) == hash(beam_plain)
    assert on != beam_plain and on != plain and len({plain, off, beam_plain, off_beam, on}) == 3
    assert on == DecodeSettings.from_kw(dict(search="beam", length_penalty=1), 8, 10)
    assert on != DecodeSettings.from_kw(dict(search="beam", length_penalty=2.0), 25, 100)
    assert on.search == "beam" and type(on.search) is str and on.length_penalty == 1.0 and plain.length_penalty == 0.0
    lp_on = DecodeSettings.from_kw(dict(search="beam", length_penalty=1.0, return_logprobs=True), 25, 100)
    assert dataclasses.replace(lp_on, return_logprobs=False) == on and lp_on != on
    with pytest.raises(dataclasses.FrozenInstanceError):
        on.length_penalty = 0.0
    # it survives compiled() and replace() of another field
    assert on.compiled("cpu").length_penalty == 1.0 and on.compiled("cpu") == on
    moved = dataclasses.replace(on, min_len=2)
    assert moved.length_penalty == 1.0 and moved.min_len == 2 and moved.search == "beam" and moved != on
    assert dataclasses.replace(moved, min_len=0) == on
    kw = dict(search="beam", length_penalty=1.0)
    DecodeSettings.from_kw(kw, 25, 100)
    assert kw == dict(search="beam", length_penalty=1.0)                     # read, not removed


def test_from_kw_checks_it_last():
    for kw, exc, match in ((dict(length_penalty="x", search="nope"), ValueError, "search"),
                           (dict(length_penalty="x", return_logprobs=1), TypeError, "return_logprobs"),
                           (dict(length_penalty="x", top_p=2), ValueError, "top_p"),
                           (dict(length_penalty="x"), TypeError, "length_penalty"),
                           (dict(length_penalty=True, search="beam"), TypeError, "length_penalty"),
                           (dict(length_penalty=9, search="beam"), ValueError, "length_penalty"),
                           (dict(length_penalty=1.0), ValueError, 'belongs to search="beam"'),
                           (dict(length_penalty=1.0, search="sample"), ValueError, 'belongs to search="beam"')):
        with pytest.raises(exc, match=match):
            DecodeSettings.from_kw(kw, 25, 100)
    with pytest.raises(ValueError, match="normal fp32 range"):
        DecodeSettings.from_kw(dict(length_penalty=8.0, search="beam"), 100000, 100)


def test_set_length_penalty_and_new_helper(monkeypatch):
    assert list(inspect.signature(BeamSearchHelper.set_length_penalty).parameters) == ["self", "length_penalty"]
    assert "length_penalty" not in inspect.signature(BeamSearchHelper.__init__).parameters
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    calls = []
    for name in ("set_constraints", "set_search", "set_logprobs", "set_length_penalty"):
        real = getattr(BeamSearchHelper, name)
        monkeypatch.setattr(BeamSearchHelper, name, lambda self, *a, _n=name, _r=real, **k: (calls.append((_n, a)), _r(self, *a, **k))[1])
    h = DecodeSettings.from_kw(dict(search="beam", length_penalty=1.0), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert [c[0] for c in calls] == ["set_constraints", "set_search", "set_logprobs", "set_length_penalty"] and calls[-1][1] == (1.0,)
    assert h.length_penalty == 1.0 and h.keys.shape == (6,) and h.keys.dtype == torch.float32 and bool((h.keys == 0).all())
    assert h.len_w.dtype == torch.float32 and torch.equal(h.len_w, LP.weights(1.0, 8)) and h.keys.data_ptr() != h.vals.data_ptr()
    off = DecodeSettings.from_kw(dict(search="beam"), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert off.length_penalty == 0.0 and off.keys is None and off.len_w is None
    bare = BeamSearchHelper(1.0, 2, 5, 1, 3, "cpu")
    assert bare.length_penalty == 0.0 and bare.keys is None and bare.set_length_penalty(0.0) is bare and bare.keys is None
    with pytest.raises(ValueError, match='belongs to search="beam"'):
        bare.set_length_penalty(1.0)                                         # (the helper's search is still "sample")
    with pytest.raises(TypeError, match="length_penalty"):
        bare.set_search("beam").set_length_penalty(True)
    assert bare.set_length_penalty(0.5).keys is not None and bare.set_length_penalty(0).keys is None      # off again: the state goes
    # the reference-style method surface raises on such a helper, as for search="beam"
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_search("beam").set_length_penalty(1.0)
    logits = torch.zeros(3, 8)
    with pytest.raises(NotImplementedError):
        h.sample_k_indices(logits)
    with pytest.raises(NotImplementedError):
        h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))


# ---- the helper's launches ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_sample_nucleus", "beam_row_sample_prompted", "beam_row_sample_groups",
            "beam_row_sample", "beam_select_prompted", "beam_select", "beam_row_best", "beam_select_best", "beam_select_best_norm",
            "beam_pick_logprobs", "beam_record_logprobs", "beam_finalize", "beam_finalize_beams", "beam_gather_logprobs",
            "beam_gather_attention")
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


def session(recorded, kw, phase):
    """The launches of a short session: a first (or prompted) step, two later steps, the finalize.  Returns (names, calls, helper)."""
    del recorded[:]
    h = DecodeSettings.from_kw(dict(kw, no_repeat_ngram_size=2), MAX_LEN, V).new_helper(beam_size=BEAM, top_k=3, device="cpu", n_img=N_IMG,
                                                                                       max_len=MAX_LEN)
    if phase == "prompted":
        h.set_prompts(torch.zeros(N_IMG, 3, dtype=torch.int64), torch.tensor([1, 3], dtype=torch.int32))
        for s in (1, 2, 3):
            h.step_prompted(torch.zeros(N_IMG * BEAM, V), write_pos=s, t=0, step_index=s, first_sets_ended=True)
        h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=4, t=0, step_index=4)      # behind the longest prompt: dense again
        pos = 0
    else:
        pos = 2
        h.step(torch.zeros(N_IMG, V), first=True, write_pos=pos, t=0, step_index=pos, first_sets_ended=True)
        for s in (pos + 1, pos + 2):
            h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=s, t=0, step_index=s)
        h.step(torch.zeros(N_IMG * BEAM, V), first=False, write_pos=MAX_LEN, t=0, step_index=MAX_LEN)       # no column: no launch
    h.finalize(1, MAX_LEN, defer_check=True, beams=True, pos=pos)
    return [n for n, _ in recorded], list(recorded), h


def strip(calls):
    """A call list without the tensors' identities: names, and every plain argument."""
    return [(n, {k: v for k, v in a.items() if not torch.is_tensor(v)}) for n, a in calls]


@pytest.mark.parametrize("phase", ("dense", "prompted"))
@pytest.mark.parametrize("logprobs", (False, True))
def test_zero_is_the_call_without_it_and_non_zero_swaps_the_select_only(recorded, phase, logprobs):
    base = dict(search="beam", return_logprobs=logprobs)
    names0, calls0, h0 = session(recorded, base, phase)
    names_off, calls_off, h_off = session(recorded, dict(base, length_penalty=0.0), phase)
    assert names_off == names0 and strip(calls_off) == strip(calls0) and "beam_select_best_norm" not in names0
    assert h_off.keys is None and h_off.len_w is None
    fin = calls_off[-2 if logprobs else -1]
    assert fin[0] == "beam_finalize_beams" and fin[1]["vals"] is h_off.vals
    names1, calls1, h1 = session(recorded, dict(base, length_penalty=1.0), phase)
    assert names1 == ["beam_select_best_norm" if n == "beam_select_best" else n for n in names0]
    assert names1.count("beam_select_best_norm") == names0.count("beam_select_best") == (4 if phase == "prompted" else 3)
    steps = []
    for (n0, a0), (n1, a1) in zip(calls0, calls1):
        if n1 == "beam_select_best_norm":
            assert a1["keys"] is h1.keys and a1["len_w"] is h1.len_w and a1["vals"] is h1.vals and a1["tokens"] is h1.tokens
            assert a1["first_sets_ended"] is True and a1["pick_idx"] is h1.pick_idx and a1["hparent"] is h1.hparent
            for k in ("n_img", "beam", "first", "write_pos", "t", "step_index", "eos_index", "first_sets_ended"):
                assert a1[k] == a0[k], k
            if phase == "prompted":
                assert a1["first_pos"] is h1.first_pos                       # also at the dense step behind the longest prompt
            else:
                assert a1["first_pos"] is None and a1["first_col"] == 2      # the dense first step's column, at every later step too
            steps.append(a1["step_index"])
        elif n1 == "beam_finalize_beams":
            assert a1["vals"] is h1.keys and a0["vals"] is h0.vals           # the final order runs on the keys
            assert {k: v for k, v in a1.items() if not torch.is_tensor(v)} == {k: v for k, v in a0.items() if not torch.is_tensor(v)}
        else:                                                                # the row step, the edits, the pick / record / gather launches
            assert strip([(n1, a1)]) == strip([(n0, a0)])
    assert steps == ([1, 2, 3, 4] if phase == "prompted" else [2, 3, 4])
    if logprobs:
        assert names1.count("beam_pick_logprobs") == names1.count("beam_record_logprobs") == len(steps) and names1[-1] == "beam_gather_logprobs"


def test_sampled_default_is_untouched(recorded):
    for kw in ({}, dict(length_penalty=0.0), dict(search="sample", length_penalty=0)):
        del recorded[:]
        h = DecodeSettings.from_kw(kw, 8, V).new_helper(beam_size=BEAM, top_k=3, device="cpu", n_img=N_IMG, max_len=8)
        h.step(torch.zeros(N_IMG, V), first=True, write_pos=0, t=0, step_index=0)
        h.finalize(1, 8, defer_check=True)
        assert [n for n, _ in recorded] == ["beam_row_sample", "beam_select", "beam_finalize"] and h.keys is None


# ---- the restatement reduces to today's at 0.0 -------------------------------------------------------------------------------------
def random_state(n, b, max_len, v, seed, src_len=0):
    """A random mid-search state (live beams, beams ended at different lengths, a done image, -inf scores) and random picks."""
    g = torch.Generator().manual_seed(seed)
    st = LP.new_state(n, b, max_len, src_len)
    r = n * b
    st.tokens[:] = torch.randint(4, v, (r, max_len), generator=g).int()
    st.vals[:] = -torch.rand(r, generator=g) * 8
    st.ended[:] = (torch.rand(r, generator=g) < 0.3).to(torch.uint8)
    st.vals[torch.rand(r, generator=g) < 0.1] = R.NEG
    if n > 1:
        st.done[n - 1] = 1
        st.ended[(n - 1) * b:] = 1
    if src_len:
        st.src[:] = (torch.arange(r)[:, None] // b * b + torch.randint(0, b, (r, src_len), generator=g)).int()
    pick_idx = torch.randint(2, v, (r, b), generator=g).int()
    pick_idx[torch.rand(r, b, generator=g) < 0.2] = EOS
    pick_val = -torch.rand(r, b, generator=g) * 4
    pick_val[torch.rand(r, b, generator=g) < 0.1] = R.NEG
    return st, pick_idx, pick_val


def as_plain(st):
    p = R.State.of(st.tokens, st.vals, st.ended, st.done, st.end_step, st.beam, st.src, st.parent, st.hparent)
    return p


@pytest.mark.parametrize("b", (1, 2, 5))
@pytest.mark.parametrize("mode", ("first", "later", "prompted"))
def test_at_zero_the_select_and_the_final_order_are_beam_search_refs(b, mode):
    n, max_len, v = 4, 7, 30
    w0 = LP.weights(0.0, max_len)
    assert bool((w0 == 1).all())
    for seed in range(8):
        st, pick_idx, pick_val = random_state(n, b, max_len, v, 17 * seed + b, src_len=max_len + 1)
        st.keys[:] = st.vals                                                 # (what a search at 0.0 has carried)
        if mode == "first":
            st.ended[:] = 0
            st.done[:] = 0
        plain = as_plain(st)
        first_pos = [4, 3, 0, 1] if mode == "prompted" else None
        args = (pick_idx, pick_val, mode == "first", 3, 3, 3, EOS)
        R.select_best(plain, *args, first_pos=first_pos)
        LP.select_best_norm(st, *args, w0, first_col=1, first_pos=first_pos)
        for k, t in plain.fields().items():
            assert torch.equal(getattr(st, k).view(torch.int32) if k == "vals" else getattr(st, k), t.view(torch.int32) if k == "vals" else t), (k, seed)
        assert torch.equal(st.keys.view(torch.int32), st.vals.view(torch.int32))       # every weight is 1: the keys ARE the scores
        want, got = R.finalize_best(plain, 1, max_len, 0, EOS, 1, first_pos), LP.finalize_norm(st, 1, max_len, 0, EOS, 1, first_pos)
        for k in want:
            assert torch.equal(want[k], got[k]), k


def table_model(v, seed, scale=2.0, eos_boost=0.0):
    cache = {}

    def row(prefix):
        if prefix not in cache:
            g = torch.Generator().manual_seed(hash((seed,) + prefix) % (1 << 31))
            cache[prefix] = torch.randn(v, generator=g) * scale
            cache[prefix][EOS] += eos_boost
        return cache[prefix]

    def logits_fn(tokens, pos, rows_per_img):
        return torch.stack([row(tuple(int(t) for t in tokens[r, :pos])) for r in range(tokens.shape[0])])
    return logits_fn


@pytest.mark.parametrize("b", (1, 3))
def test_at_zero_the_driver_is_beam_search_refs(b):
    for seed in range(3):
        fn = table_model(11, seed, eos_boost=1.5)
        want, err = R.beam_search(fn, 3, b, 6, temperature=1.3)
        got, err2, st = LP.beam_search_norm(fn, 3, b, 6, 0.0, temperature=1.3)
        assert err == err2 and torch.equal(st.keys.view(torch.int32), st.vals.view(torch.int32))
        for k in want:
            assert torch.equal(want[k], got[k]), (k, seed)
        assert bool((want["lengths"] < 6).any())                             # some beams did end early


def test_the_driver_changes_its_mind_with_the_penalty():
    """Random tables with a likely ``<eos>``: over a few seeds a positive penalty lengthens some winners, and the scores it returns
    are the sorted keys -- a beam's raw score times the weight of its own length, one fp32 multiply."""
    longer = 0
    for seed in range(6):
        fn = table_model(11, seed, eos_boost=2.5)
        zero, _, _ = LP.beam_search_norm(fn, 4, 3, 8, 0.0)
        pos, _, st = LP.beam_search_norm(fn, 4, 3, 8, 2.0)
        longer += int((pos["lengths"][:, 0] > zero["lengths"][:, 0]).sum())
        finite = torch.where(torch.isinf(pos["scores"]), torch.full_like(pos["scores"], -1e30), pos["scores"])
        assert bool((finite[:, :-1] >= finite[:, 1:]).all())
        w = LP.weights(2.0, 8)
        for i in range(4):
            for slot in range(3):
                k = int(pos["beam_index"][i, slot])
                ln = int(pos["lengths"][i, slot])
                if bool(st.ended[i * 3 + k]) or ln == 8:                     # key = vals * w[L], one fp32 multiply
                    assert float(pos["scores"][i, slot]) == float(LP.key_of(st.vals[i * 3 + k].item(), w[ln]))
    assert longer > 0


# ---- the restatement is meaningful: worked by hand ---------------------------------------------------------------------------------
def hand_search(length_penalty):
    """2 images, beam 2, 3 columns, every number a short binary fraction.

    Image 0.  Step 0 keeps the row's picks as they are: beam 0 = [<eos>] at -1 (ended, L = 1: key -1 at any penalty), beam 1 = [5] at
    -1.5.  Step 1 (L = 2): the live beam brings [5, 6] at -1.75 and [5, <eos>] at -2.5, the ended one itself at -1.
      penalty 0: keys -1.75, -2.5 | -1       -> [<eos>] (-1), [5, 6] (-1.75)
      penalty 1: keys -0.875, -1.25 | -1     -> [5, 6] (-0.875), [<eos>] (-1): w[2] = 0.5
    Step 2 (L = 3), both rows pick <eos> at -0.5 and 7 at -2: [5, 6, <eos>] at -2.25, [5, 6, 7] at -3.75, the ended beam at -1.
      penalty 0: -1 | -2.25, -3.75           -> [<eos>] (-1), [5, 6, <eos>] (-2.25): the early <eos> wins
      penalty 1: -2.25 * w[3] = -0.75.., -3.75 * w[3] = -1.25.. | -1 -> [5, 6, <eos>] (-0.75), [<eos>] (-1): the longer beam wins
    Image 1 never meets <eos> before the last column, so every candidate of a step has the same L and the penalty changes nothing:
    [8, 10, <eos>] (-1.25) in front of [8, 10, 14] (-1.5, which ties with [9, 12, <eos>] and has the lower candidate index)."""
    st = LP.new_state(2, 2, 3)
    w = LP.weights(length_penalty, 3)
    LP.select_best_norm(st, torch.tensor([[EOS, 5], [8, 9]]), torch.tensor([[-1.0, -1.5], [-0.5, -0.75]]), True, 0, 0, 0, EOS, w)
    live = torch.tensor([[6, EOS], [6, EOS]])                                # (image 0: whichever row the live beam sits in)
    live_val = torch.tensor([[-0.25, -1.0], [-0.25, -1.0]])
    LP.select_best_norm(st, torch.cat([live, torch.tensor([[10, 11], [12, 13]])]),
                        torch.cat([live_val, torch.tensor([[-0.5, -1.0], [-0.5, -4.0]])]), False, 1, 0, 1, EOS, w)
    mid = {k: getattr(st, k).clone() for k in ("tokens", "vals", "keys", "ended")}
    LP.select_best_norm(st, torch.tensor([[EOS, 7], [EOS, 7], [EOS, 14], [EOS, 14]]),
                        torch.tensor([[-0.5, -2.0], [-0.5, -2.0], [-0.25, -0.5], [-0.25, -0.5]]), False, 2, 0, 2, EOS, w)
    return st, mid, LP.finalize_norm(st, 1, 3, 0, EOS)


def test_by_hand_an_early_eos_wins_at_zero_and_the_longer_beam_at_one():
    st, mid, out = hand_search(0.0)
    assert mid["tokens"][:2, :2].tolist() == [[EOS, 0], [5, 6]] and mid["vals"][:2].tolist() == [-1.0, -1.75] == mid["keys"][:2].tolist()
    assert out["tokens"][0].tolist() == [[EOS, 0, 0], [5, 6, EOS]] and out["lengths"][0].tolist() == [1, 3]
    assert out["scores"][0].tolist() == [-1.0, -2.25] and st.done.tolist() == [1, 0] and st.end_step.tolist() == [2, 0]
    assert out["tokens"][1].tolist() == [[8, 10, EOS], [8, 10, 14]] and out["scores"][1].tolist() == [-1.25, -1.5]

    st, mid, out = hand_search(1.0)
    assert mid["tokens"][:2, :2].tolist() == [[5, 6], [EOS, 0]] and mid["vals"][:2].tolist() == [-1.75, -1.0]
    assert mid["keys"][:2].tolist() == [-0.875, -1.0] and mid["ended"][:2].tolist() == [0, 1]
    third = np.float32(1.0 / 3.0)
    assert out["tokens"][0].tolist() == [[5, 6, EOS], [EOS, 0, 0]] and out["lengths"][0].tolist() == [3, 1]
    assert out["scores"][0].tolist() == [float(np.float32(-2.25) * third), -1.0] and st.vals[:2].tolist() == [-2.25, -1.0]
    assert out["beam_index"][0].tolist() == [0, 1] and st.done.tolist() == [1, 0]
    # image 1: the same beams in the same order, the keys scaled by w[3] -- the ended beam's carried key IS score * w[3] here
    assert out["tokens"][1].tolist() == [[8, 10, EOS], [8, 10, 14]] and st.vals[2:].tolist() == [-1.25, -1.5]
    assert out["scores"][1].tolist() == [float(np.float32(-1.25) * third), float(np.float32(-1.5) * third)]


@pytest.mark.parametrize("ended_first", (False, True))
def test_by_hand_equal_keys_go_to_the_lower_candidate_index(ended_first):
    """Penalty 1, step 1 (L = 2, w = 0.5): the live beam's [5, 6] has score -2 and key -1; the beam that ended at L = 1 has score -1 and
    key -1.  Different raw scores, the same key in fp32: whichever comes first in the candidate list stays in front."""
    st = LP.new_state(1, 2, 3)
    w = LP.weights(1.0, 3)
    first = ([EOS, 5], [-1.0, -1.5]) if ended_first else ([5, EOS], [-1.5, -1.0])
    LP.select_best_norm(st, torch.tensor([first[0]]), torch.tensor([first[1]]), True, 0, 0, 0, EOS, w)
    picks, vals = torch.tensor([[6, 7], [6, 7]]), torch.tensor([[-0.5, -1.0], [-0.5, -1.0]])
    LP.select_best_norm(st, picks, vals, False, 1, 0, 1, EOS, w)
    assert st.keys.tolist() == [-1.0, -1.0]
    if ended_first:
        assert st.tokens[:, :2].tolist() == [[EOS, 0], [5, 6]] and st.vals.tolist() == [-1.0, -2.0] and st.parent.tolist() == [0, 1]
    else:
        assert st.tokens[:, :2].tolist() == [[5, 6], [EOS, 0]] and st.vals.tolist() == [-2.0, -1.0] and st.parent.tolist() == [0, 1]
    out = LP.finalize_norm(st, 1, 3, 0, EOS)
    assert out["beam_index"].tolist() == [[0, 1]] and out["scores"].tolist() == [[-1.0, -1.0]]        # the lower engine index on ties
    # at penalty 0 the raw scores decide: the ended beam (-1) is in front of [5, 6] (-2) wherever it stands
    st0 = LP.new_state(1, 2, 3)
    LP.select_best_norm(st0, torch.tensor([first[0]]), torch.tensor([first[1]]), True, 0, 0, 0, EOS, LP.weights(0.0, 3))
    LP.select_best_norm(st0, picks, vals, False, 1, 0, 1, EOS, LP.weights(0.0, 3))
    assert st0.tokens[:, :2].tolist() == [[EOS, 0], [5, 6]] and st0.vals.tolist() == [-1.0, -2.0]


def test_a_prompted_image_counts_from_its_own_first_column():
    """Two images at absolute step 3: image 0 (prompt of 3) makes its first step there (L = 1), image 1 (no prompt) its fourth
    (L = 4); image 2 (prompt of 5) is still forced and keeps its keys."""
    st = LP.new_state(3, 2, 8)
    w = LP.weights(-1.0, 8)                                                  # w[L] = L: exact
    st.vals[2:4] = torch.tensor([-1.0, -3.0])
    st.keys[2:4] = torch.tensor([-3.0, -9.0])
    st.keys[4:6] = 7.0
    pick_idx = torch.tensor([[5, 6], [9, 9], [7, 8], [7, 8], [9, 9], [9, 9]])
    pick_val = torch.tensor([[-0.5, -1.0], [-9.0, -9.0], [-0.5, -1.0], [-0.25, -0.5], [-9.0, -9.0], [-9.0, -9.0]])
    LP.select_best_norm(st, pick_idx, pick_val, False, 3, 0, 3, EOS, w, first_col=99, first_pos=[3, 0, 5])
    assert st.vals[:2].tolist() == [-0.5, -1.0] and st.keys[:2].tolist() == [-0.5, -1.0]               # w[1] = 1
    assert st.vals[2:4].tolist() == [-1.5, -2.0] and st.keys[2:4].tolist() == [-6.0, -8.0]             # w[4] = 4
    assert st.keys[4:6].tolist() == [7.0, 7.0] and st.vals[4:6].tolist() == [0.0, 0.0]


# ---- the C-ABI addition ------------------------------------------------------------------------------------------------------------
NORM_ARGS = ["pick_idx", "pick_val", "tokens", "tok_ld", "vals", "keys", "ended", "src", "src_ld", "parent", "hparent", "done", "end_step",
             "n_img", "beam", "first", "first_pos", "first_col", "len_w", "first_sets_ended", "write_pos", "t", "step_index", "eos_index",
             "stream"]


def test_abi_header_table_and_library_agree():
    name = "dh_beam_select_best_norm"
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[name]
    assert len(args) == len(sig) == len(NORM_ARGS) == 25
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == NORM_ARGS
    # one version in the header, the table, the binding and the library (additive: no prototype moved, so the number the other
    # modules pin stays)
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == lib.dh_abi_version()
    assert hasattr(lib, name) and hasattr(hip, "beam_select_best_norm")
    assert len(_abi.SIGNATURES["dh_beam_select_best"]) == 22 and len(_abi.SIGNATURES["dh_beam_finalize_beams"]) == 26
    wrapper = list(inspect.signature(hip.beam_select_best_norm).parameters)
    assert wrapper[:6] == ["pick_idx", "pick_val", "tokens", "vals", "keys", "ended"] and wrapper[-3:] == ["len_w", "first_col", "first_pos"]


def call_with(fn, good, **over):
    a = list(good)
    for k, val in over.items():
        a[NORM_ARGS.index(k)] = val
    return fn(*a)


def test_select_best_norm_argument_contract():
    """Checked before any HIP call (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    fn = hip.load().dh_beam_select_best_norm
    #       pi  pv  tok ld vals keys end src sld par hpar done estep n b first first_pos col len_w fse wp t step eos stream
    good = [64, 64, 64, 8, 64, 64, 64, None, 0, 64, 64, 64, 64, 2, 3, 0, None, 0, 64, 1, 1, 0, 1, 3, None]
    for over in (dict(len_w=None), dict(keys=None), dict(first_col=-1), dict(len_w=None, first_pos=64), dict(keys=None, first_pos=64),
                 dict(pick_idx=None), dict(pick_val=None), dict(tokens=None), dict(vals=None), dict(ended=None), dict(parent=None),
                 dict(hparent=None), dict(done=None), dict(end_step=None), dict(n_img=0), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1),
                 dict(tok_ld=0), dict(t=-1), dict(src=64, src_ld=0, t=0), dict(src=64, src_ld=5, t=5),
                 dict(beam=64, tok_ld=300), dict(first_pos=64, beam=64, tok_ld=300)):
        assert call_with(fn, good, **over) == 1, over


# ---- the keyword through the layers, and the refusals ------------------------------------------------------------------------------
def test_keyword_rides_in_kw_and_the_pinned_lists_stay():
    import deephumor_amd.models as M
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder
    fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
    fns += [TransformerDecoder.generate_batch, TransformerDecoder.generate, SelfAttentionTransformerDecoder.generate_batch,
            SelfAttentionTransformerDecoder.generate, LSTMDecoder.generate]
    for fn in fns:
        ps = inspect.signature(fn).parameters
        assert "length_penalty" not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # (the signatures of every public callable, and the keyword on its way to DecodeSettings.from_kw: test_decode_settings_cpu)
    assert [p.name for p in inspect.signature(LSTMDecoder.generate_batch).parameters.values() if p.kind is not p.VAR_KEYWORD][-1] == "repetition_penalty"
    with pytest.raises(ValueError, match="length_penalty"):                  # ... and takes the keyword by name
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="beam", length_penalty=float("nan"))


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
    cases = ((dict(search="beam", length_penalty=True), TypeError, "length_penalty must be a real number"),
             (dict(search="beam", length_penalty="1"), TypeError, "length_penalty must be a real number"),
             (dict(search="beam", length_penalty=float("inf")), ValueError, "length_penalty must be finite"),
             (dict(search="beam", length_penalty=8.5), ValueError, "length_penalty must be finite"),
             (dict(search="beam", length_penalty=8.0, max_len=100000), ValueError, "normal fp32 range"),
             (dict(length_penalty=1.0), ValueError, 'belongs to search="beam"'),
             (dict(search="sample", length_penalty=-1.0), ValueError, 'belongs to search="beam"'))
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
        seen.append(s.length_penalty)
        return s
    real = beam.DecodeSettings.from_kw
    monkeypatch.setattr(beam.DecodeSettings, "from_kw", staticmethod(from_kw))
    monkeypatch.setattr(model, "encode", lambda *a: dec_args)
    monkeypatch.setattr(type(model.decoder), "_check_mode", lambda self: (_ for _ in ()).throw(Reached()))
    for call in (model.generate_batch, model.generate):
        for value in (1.0, 0.0):
            del seen[:]
            with pytest.raises(Reached):
                call(images, search="beam", length_penalty=value)
            assert seen and set(seen) == {value}
    del seen[:]
    with pytest.raises(Reached):
        model.decode(dec_args, search="beam", length_penalty=-0.5)
    assert seen == [-0.5]


def test_it_is_in_the_graph_key(monkeypatch):
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
    plain, zero, one, one_int, two = (key_of(search="beam"), key_of(search="beam", length_penalty=0.0), key_of(search="beam", length_penalty=1.0),
                                      key_of(search="beam", length_penalty=1), key_of(search="beam", length_penalty=2.0))
    assert plain == zero and hash(plain) == hash(zero) and one == one_int and len({plain, one, two}) == 3
    assert ("length_penalty", 1.0) in one[2] and "length_penalty" not in dict(plain[2])
    assert key_of() == key_of(length_penalty=0)                              # the sampled default: the plain graph
    # the table is uploaded in front of the capture
    assert (str(images.device), 2.0, 25) in beam._LEN_W_CACHE


def test_pipeline_and_sharded_callers_carry_the_keyword():
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline

    class Model:
        _hp = {"num_tokens": 50}

        def parameters(self):
            return iter([torch.zeros(1)])
    for kw, exc in ((dict(search="beam", length_penalty=True), TypeError), (dict(search="beam", length_penalty=9.0), ValueError),
                    (dict(length_penalty=1.0), ValueError)):
        with pytest.raises(exc, match="length_penalty"):
            CaptionPipeline(Model(), overlap=False, **kw)
    src = inspect.getsource(CaptionPipeline.__init__)
    assert "DecodeSettings.from_kw(gen_kw" in src and 'pop("length_penalty"' not in src      # validated with the rest, handed on as it is
    assert "length_penalty" in CaptionPipeline.__init__.__doc__ and "length_penalty" in dist.generate_sharded.__doc__
    seen = {}
    got = dist.generate_sharded(lambda lo, hi: seen.update(lo=lo, hi=hi) or (torch.zeros(hi - lo, 4, dtype=torch.int64),
                                                                              torch.ones(hi - lo, dtype=torch.int64)), 3)
    assert seen == dict(lo=0, hi=3) and got[0].shape == (3, 4)


# ---- who owns the table, and the carrier on ``search`` -----------------------------------------------------------------------------
def test_a_graph_state_keeps_its_table_when_the_cache_moves_on():
    """The captured select nodes hold the table's raw pointer: the cached graph state must own the tensor, because the cache evicts."""
    import gc
    import weakref
    import deephumor_amd.models as M
    beam._LEN_W_CACHE.clear()
    table = beam.compile_length_weights(1.5, 9, "cpu")
    other = beam.compile_length_weights(1.5, 12, "cpu")                      # (an LSTM prefix session's wider table: kept as well)
    beam.compile_length_weights(2.5, 9, "cpu")
    state = M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None, length_penalty=1.5, device="cpu")
    assert state[:8] == ("graph", [], None, None, (), "sig", [], None) and len(state[8]) == 2
    assert any(t is table for t in state[8]) and any(t is other for t in state[8])
    assert M.CaptioningLSTM._graph_state("graph", [], None, None, (), "sig", [], None)[8] == ()      # no penalty: nothing to hold
    ref = weakref.ref(table)
    for n in range(beam._LEN_W_CACHE_SIZE + 1):                              # past its size: the first entries are gone
        beam.compile_length_weights(0.25, 20 + n, "cpu")
    assert ("cpu", 1.5, 9) not in beam._LEN_W_CACHE and len(beam._LEN_W_CACHE) == beam._LEN_W_CACHE_SIZE
    del table, other
    gc.collect()
    assert ref() is not None and any(t is ref() for t in state[8])           # the state is what keeps it
    again = beam.compile_length_weights(1.5, 9, "cpu")                       # a new upload, another tensor: the graph's is untouched
    assert again is not ref() and torch.equal(again, ref())
    del state
    gc.collect()
    assert ref() is None
    src = inspect.getsource(M.CaptioningLSTM.generate_batch_graphed)
    assert "self._graph_state(" in src and "length_penalty=settings.length_penalty" in src


def test_the_cache_evicts_the_least_recently_used_table():
    beam._LEN_W_CACHE.clear()
    first = beam.compile_length_weights(1.0, 5, "cpu")
    for n in range(beam._LEN_W_CACHE_SIZE - 1):
        beam.compile_length_weights(1.0, 6 + n, "cpu")
    assert beam.compile_length_weights(1.0, 5, "cpu") is first               # a hit: most recently used now
    beam.compile_length_weights(3.0, 5, "cpu")                               # one more: the oldest goes, not the one just used
    assert ("cpu", 1.0, 5) in beam._LEN_W_CACHE and ("cpu", 1.0, 6) not in beam._LEN_W_CACHE
    assert beam.held_length_weights(0.0, "cpu") == () and len(beam.held_length_weights(3.0, "cpu")) == 1


def test_the_record_copies_pickles_and_takes_the_penalty_from_the_keyword_alone():
    import copy
    import pickle
    on = DecodeSettings.from_kw(dict(search="beam", length_penalty=1.5, min_len=2), 25, 100)
    for clone in (copy.copy(on), copy.deepcopy(on), pickle.loads(pickle.dumps(on)), on.compiled("cpu"), dataclasses.replace(on, min_len=2)):
        assert clone == on and clone.length_penalty == 1.5 and clone.search == "beam" and hash(clone) == hash(on)
        assert clone.min_len == 2 and type(clone.search) is str
    s = pickle.loads(pickle.dumps(on.search))
    assert s == "beam" and type(s) is str and type(on.search) is str
    # the penalty is a field of its own: replace(search=...) keeps it
    same = dataclasses.replace(on, search="beam")
    assert same.length_penalty == 1.5 and same == on and same != DecodeSettings.from_kw(dict(search="beam", min_len=2), 25, 100)
    # a record's `search` handed back in brings no penalty with it: the keyword alone sets one
    back = DecodeSettings.from_kw(dict(search=on.search), 25, 100)
    assert back.length_penalty == 0.0 and type(back.search) is str and back == DecodeSettings.from_kw(dict(search="beam"), 25, 100)
    both = DecodeSettings.from_kw(dict(search=on.search, length_penalty=0.5), 25, 100)
    assert both.length_penalty == 0.5
