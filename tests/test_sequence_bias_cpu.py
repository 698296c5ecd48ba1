"""``sequence_bias`` without a GPU: the restatement (``tests/bias_ref.py``) against its brute-force scan, what the kernel cases hold,
``beam.check_sequence_bias`` on every public entry before the encoder runs, ``SequenceBias`` and the host sort, the settings record,
the helper, the text helper, the signatures, and the ABI of ``dh_beam_bias_logits`` with its argument contract."""
import ctypes
import dataclasses
import inspect
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

from bias_ref import (CASE_VS, NEG_INF, ORDER_BIASES, bias_logits, bits, brute_bias_row, brute_fired, fires, flatten_sorted, kernel_cases,
                      sort_pairs)
from helpers import DECODE_FIELDS, GOLDEN, KINDS, synthetic_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dh_beam_bias_logits"
INF, NAN = float("inf"), float("nan")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_brute_force_scan(seed):
    """Random histories over a small alphabet and random lists of 1 .. 4-id phrases over the same alphabet (so that many fire, and
    several on one column), ids outside ``[0, V)`` among the last ids, duplicates, every ``pos`` from 0 on.  Bit for bit."""
    g = torch.Generator().manual_seed(seed)
    for v, alphabet in ((130, 4), (70, 6), (200, 3)):
        rows, width = 5, 9
        hist = torch.randint(0, alphabet, (rows, width), generator=g)
        pairs = [(torch.randint(0, alphabet, (int(torch.randint(1, 5, (1,), generator=g)),), generator=g).tolist(),
                  float(torch.randn(1, generator=g)) * 5) for _ in range(14)]
        pairs += [([0, v + 2], 1.0), ([1, -3], 1.0), ([1, v - 1], -2.0), pairs[0], ([2], 1e-3), ([2], 7.25), ([2], -3.1)]
        logits = torch.randn(rows, v, generator=g) * 3
        logits[0, :3] = torch.tensor([0.0, -0.0, NEG_INF])
        gm0 = torch.full((rows, (v + 63) // 64 + 1), 777.0)             # poison: one word more than there are groups
        for pos in range(width + 1):
            out, gm, stored = bias_logits(logits, hist, pos, pairs, gm0, 64)
            for r in range(rows):
                bx, bgm, bst = brute_bias_row(logits[r], hist[r, :pos].tolist(), pairs, gm0[r], 64)
                assert torch.equal(bits(out[r]), bits(bx)) and torch.equal(gm[r], bgm), (v, pos, r)
                assert stored[r].nonzero().flatten().tolist() == bst
            assert bool((gm[:, -1] == 777.0).all()) and bool(stored[:, 2].all()) and out[0, 2] == NEG_INF
            assert torch.equal(bits(out[~stored]), bits(logits[~stored]))


def test_the_rules_on_small_examples():
    f32 = np.float32
    # a single id fires at every position, the empty history included
    assert brute_fired([], [([7], 1.0)]) == [0] and brute_fired([1, 2, 3], [([7], 1.0)]) == [0]
    # a phrase fires only when its prefix ENDS the history
    assert brute_fired([5, 6], [([5, 6, 9], 1.0)]) == [0] and brute_fired([5, 6, 1], [([5, 6, 9], 1.0)]) == []
    assert brute_fired([6], [([5, 6, 9], 1.0)]) == [] and brute_fired([], [([5, 9], 1.0)]) == []      # l - 1 > s
    assert brute_fired([5], [([5, 9], 1.0), ([4, 7], 1.0), ([5, 8], 1.0)]) == [0, 2]
    x = torch.arange(8.0)[None, :]
    out, gm, stored = bias_logits(x, torch.tensor([[5]]), 1, [([5, 7], -4.5), ([2], 10.0), ([6, 3], 9.0)], torch.full((1, 1), 777.0), 64)
    assert stored[0].nonzero().flatten().tolist() == [2, 7] and out[0].tolist() == [0, 1, 12, 3, 4, 5, 6, 2.5] and gm[0, 0] == 12.0
    # list order: every addition is rounded on its own, so the order of three pairs on one column shows in the bits
    a, b, c = ORDER_BIASES
    x = torch.full((1, 4), -2.3)
    one = bias_logits(x, torch.zeros(1, 0), 0, [([1], a), ([1], b), ([1], c)])[0][0, 1]
    other = bias_logits(x, torch.zeros(1, 0), 0, [([1], c), ([1], b), ([1], a)])[0][0, 1]
    assert float(one) == float(f32(f32(f32(f32(-2.3) + f32(a)) + f32(b)) + f32(c))) and float(one) != float(other)
    # the same phrase twice counts twice; a zero bias still stores (the group is recomputed, the value stays)
    out, gm, stored = bias_logits(torch.zeros(1, 70), torch.zeros(1, 0), 0, [([3], 1.5), ([3], 1.5), ([65], 0.0)], torch.full((1, 2), 777.0), 64)
    assert out[0, 3] == 3.0 and gm[0].tolist() == [3.0, 0.0] and stored[0].nonzero().flatten().tolist() == [3, 65]
    # -inf stays -inf and is stored; a lowered maximum; an untouched group keeps its word
    x = torch.tensor([[NEG_INF, 5.0, 4.0] + [0.0] * 67])
    out, gm, stored = bias_logits(x, torch.zeros(1, 0), 0, [([0], 100.0), ([1], -3.0)], torch.full((1, 2), 777.0), 64)
    assert out[0, 0] == NEG_INF and bool(stored[0, 0]) and out[0, 1] == 2.0 and gm[0].tolist() == [4.0, 777.0]
    # a last id outside [0, V) is never a column
    out, _, stored = bias_logits(torch.zeros(1, 8), torch.zeros(1, 0), 0, [([8], 1.0), ([-1], 1.0)])
    assert not stored.any() and not out.any()
    # inactive rows keep every word
    out, gm, stored = bias_logits(torch.zeros(2, 8), torch.tensor([[5], [5]]), 1, [([5, 7], 1.0)], torch.full((2, 1), 777.0), 64,
                                  active=torch.tensor([False, True]))
    assert not out[0].any() and gm[0, 0] == 777.0 and not stored[0].any() and out[1, 7] == 1.0 and gm[1, 0] == 1.0


def test_the_host_sort_is_stable_by_last_id():
    pairs = [([9, 4], 1.0), ([2], 2.0), ([4], 3.0), ([7, 2], 4.0), ([1, 1, 4], 5.0), ([2], 6.0)]
    order, run_off = sort_pairs(pairs)
    assert order == [1, 3, 5, 0, 2, 4] and run_off == [0, 3, 6]
    words, offs, bias, runs = flatten_sorted(pairs)
    assert words.tolist() == [2, 7, 2, 2, 9, 4, 4, 1, 1, 4] and offs.tolist() == [0, 1, 3, 4, 6, 7, 10]
    assert bias.tolist() == [2.0, 4.0, 6.0, 1.0, 3.0, 5.0] and runs.tolist() == [0, 3, 6]
    assert words.dtype == offs.dtype == runs.dtype == torch.int32 and bias.dtype == torch.float32
    from deephumor_amd.models.beam import compile_sequence_bias, sort_sequence_bias
    tup = tuple((tuple(w), b) for w, b in pairs)
    assert sort_sequence_bias(tup) == (tuple(order), run_off)
    sb = compile_sequence_bias(pairs, 10, "cpu")
    assert torch.equal(sb.words, words) and torch.equal(sb.offsets, offs) and torch.equal(sb.bias, bias) and torch.equal(sb.run_off, runs)
    assert sb.order == tuple(order) and sb.n_runs == 2 and sb.n_words == len(sb) == 6
    g = torch.Generator().manual_seed(0)
    rnd = [(torch.randint(0, 9, (int(torch.randint(1, 4, (1,), generator=g)),), generator=g).tolist(), float(k)) for k in range(200)]
    sb = compile_sequence_bias(rnd, 9, "cpu")
    for got, want in zip((sb.words, sb.offsets, sb.bias, sb.run_off), flatten_sorted(rnd)):
        assert torch.equal(got, want)
    lasts = [rnd[i][0][-1] for i in sb.order]
    assert lasts == sorted(lasts) and all(a < b for a, b, x, y in zip(sb.order, sb.order[1:], lasts, lasts[1:]) if x == y)


@pytest.mark.parametrize("v", CASE_VS)
def test_kernel_cases_hold_what_they_promise(v):
    cases = kernel_cases(v)
    assert [c["pos"] for c in cases] == [0, 1, 5, 40, 5] and [c["rows"] for c in cases] == [12, 12, 12, 12, 4]
    assert cases[-1]["mult"] == 3 and cases[-1]["table"].shape[0] == 12
    for c in cases:
        pos, pairs, named, x = c["pos"], c["pairs"], c["named"], c["logits"]
        phrases = [w for w, _ in pairs]
        h = c["table"][::c["mult"]]
        assert len(pairs) == 300 and max(len(w) for w in phrases) == 32 and min(len(w) for w in phrases) == 1
        planted = [named[k] for k in ("O1", "O2", "O3", "D", "B", "C")] + named["never"] + [[5, v - 1], [69], [8], [6, 7], [4], [5, v + 3]]
        assert all(phrases.index(w) >= 256 for w in planted)
        assert phrases.count(named["D"]) == 2 and phrases.count([10]) == 2                            # the same phrase twice
        order, run_off = sort_pairs(pairs)
        n_runs = len(run_off) - 1
        if v > 130:                          # the stride loop over the runs takes a second trip, with a column in it
            run_of = lambda t: [q for q in range(n_runs) if phrases[order[run_off[q]]][-1] == t][0]
            assert n_runs > 256 and run_of(v - 1) >= 256 and run_of(v + 3) >= 256
        else:                                # one run of some 280 phrases on one column
            assert max(b - a for a, b in zip(run_off, run_off[1:])) > 256
        out, gm, stored = bias_logits(x, h, pos, pairs, torch.full((c["rows"], (v + 63) // 64), 777.0), 64)
        on10 = [(w, b) for w, b in pairs if w[-1] == 10]
        assert [b for _, b in on10] == list(ORDER_BIASES)
        if pos >= 1:
            r = 0
            assert all(bool(fires(h, pos, w)[r]) for w, _ in on10)                                    # three pairs on one column of row 0
            back = bias_logits(x, h, pos, [p for p in pairs if p[0][-1] != 10] + on10[::-1])[0]
            assert out[r, 10] != back[r, 10] and not torch.equal(bits(out[:, 10]), bits(back[:, 10]))  # another order, another word
            assert bool(fires(h, pos, named["D"])[2 % c["rows"]]) and not bool(fires(h, pos, named["D"]).all())
            assert out[2 % c["rows"], 12] == x[2 % c["rows"], 12] + 0.5 + 0.5
            assert bool(stored[0, v - 1]) and not bool(stored[3, v - 1]) and out[0, v - 1] == x[0, v - 1] + 2.0
            assert gm[0, (v - 1) // 64] == out[0, (v - 1) // 64 * 64:v].max()
            assert out[2 % c["rows"], 7] == x[2 % c["rows"], 7] + 50.0
        else:
            multi = [w for w in phrases if len(w) > 1]
            assert not any(bool(fires(h, pos, w).any()) for w in multi) and all(len(w) > pos + 1 for w in multi)
        # the old row maximum fell below its group's second value; a new group maximum; -inf stays
        assert bool((x.argmax(1) == 69).all()) and bool((out[:, 69] == 2.0).all()) and bool((gm[:, 1] == 9.0).all())
        assert bool((out[:, 8] == x[:, 8] + 40.0).all()) and bool((gm[:, 0] >= out[:, 8]).all()) and bool((out[:, 8] > x[:, :64].max(1).values).all())
        assert bool((out[:, 4] == NEG_INF).all()) and bool(stored[:, 4].all())
        assert not any(bool(fires(h, pos, w).any()) for w in named["never"])
        assert bool(fires(h, pos, [5, v + 3]).any()) == (pos >= 1)                                     # fires, and is no column
        assert bool(fires(h, pos, named["B"]).any()) == (pos >= 4)
        if pos >= 4:                         # the near miss: its last prefix id matches, the one before does not
            assert h[3, pos - 1] == named["B"][3] and h[3, pos - 2] != named["B"][2] and not bool(fires(h, pos, named["B"])[3])
            assert bool(stored[1, 20]) and not bool(stored[3, 20])
        assert bool(fires(h, pos, named["C"]).any()) == (pos == 40)
        if pos < 31:
            assert len(named["C"]) > pos + 1
        assert torch.equal(bits(out[~stored]), bits(x[~stored]))


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_check_sequence_bias():
    from deephumor_amd import hip
    from deephumor_amd.models.beam import MAX_SEQUENCE_BIAS, check_sequence_bias
    assert MAX_SEQUENCE_BIAS == 1e4 and (hip.MAX_BAD_WORDS, hip.MAX_BAD_LEN) == (4096, 32)
    assert check_sequence_bias() is None and check_sequence_bias(None, 10) is None
    assert check_sequence_bias({}, 10) is None and check_sequence_bias([], 10) is None and check_sequence_bias((), 10) is None
    # a mapping in insertion order, a list in list order; numbers become Python numbers
    got = check_sequence_bias({(3, 4): 2, (1,): -1.5, (2,): np.float32(0.5)}, 10)
    assert got == (((3, 4), 2.0), ((1,), -1.5), ((2,), 0.5)) and all(type(b) is float for _, b in got)
    got = check_sequence_bias([([1, 2], 1.0), (np.array([3]), np.float64(2.0)), (torch.tensor([4]), torch.tensor(3.0)), ((7,), 1), ((7,), 1)], 10)
    assert got == (((1, 2), 1.0), ((3,), 2.0), ((4,), 3.0), ((7,), 1.0), ((7,), 1.0))                 # duplicates stay, each one counts
    assert all(type(t) is int for w, _ in got for t in w)
    assert check_sequence_bias([((1,), 1e4), ((2,), -1e4), ((3,), 0.0)], 10) is not None
    check_sequence_bias([([1] * 32, 1.0)], 10)
    check_sequence_bias([([1], 1.0)] * 4096, 10)
    check_sequence_bias({(2, 10): 1.0}, None)                            # no vocabulary size given: only the lower bound
    # a bad bias names the phrase; the message sends bans to bad_words_ids
    for bad in (True, False, NAN, INF, -INF, 1.0001e4, -2e4, "1", None, [1.0], 1 + 0j):
        with pytest.raises(ValueError, match=r"phrase 1 \(5, 6\).*bad_words_ids"):
            check_sequence_bias([((1,), 1.0), ((5, 6), bad)], 10)
    for bad, phrase in (([((1,), 1.0), ((), 1.0)], "phrase 1"), ({(1,): 1.0, (2, 10): 1.0}, "phrase 1"), ({(-1,): 1.0}, "phrase 0"),
                        ([((1, 2.0), 1.0)], "phrase 0"), ([((True,), 1.0)], "phrase 0"), ([([1] * 33, 1.0)], "phrase 0"),
                        ([((1,), 1.0)] * 4097, "phrase 4096"), ({5: 1.0}, "phrase 0"), ([("ab", 1.0)], "phrase 0"), ([((None,), 1.0)], "phrase 0")):
        with pytest.raises(ValueError, match="sequence_bias: " + phrase):
            check_sequence_bias(bad, 10)
    for bad in ([(1,)], [((1,), 1.0, 2.0)], [5], ["ab"]):                 # an entry that is no pair
        with pytest.raises(ValueError, match="entry 0"):
            check_sequence_bias(bad, 10)
    for bad in ("abc", 5, b"ab", 2.5):
        with pytest.raises(TypeError, match="sequence_bias_from_words"):
            check_sequence_bias(bad, 10)

    class Reforward:
        pad_index = 1

    class Incremental:
        pad_index = 0
    assert check_sequence_bias(None, 10, Reforward()) is None and check_sequence_bias({}, 10, Reforward()) is None
    assert check_sequence_bias({(1,): 1.0}, 10, Incremental()) == (((1,), 1.0),)
    with pytest.raises(NotImplementedError, match="pad_index == 1"):
        check_sequence_bias({(1,): 1.0}, 10, Reforward())


def test_sequence_bias_is_immutable_hashable_and_cached():
    from deephumor_amd.models.beam import SequenceBias, check_sequence_bias, compile_sequence_bias
    a = compile_sequence_bias({(1, 2): 1.5, (3,): -2.0}, 10, "cpu")
    b = compile_sequence_bias([([1, 2], 1.5), ((3,), -2)], 10, "cpu")
    c = compile_sequence_bias({(1, 2): 1.5, (3,): -2.5}, 10, "cpu")
    d = compile_sequence_bias([((3,), -2.0), ((1, 2), 1.5)], 10, "cpu")      # another order is another list
    assert isinstance(a, SequenceBias) and a == b and hash(a) == hash(b) and a != c and a != d and len({a, b, c, d}) == 3
    assert a.words is b.words and a.offsets is b.offsets and a.bias is b.bias and a.run_off is b.run_off      # uploaded once
    assert a.pairs == (((1, 2), 1.5), ((3,), -2.0)) and len(a) == a.n_words == 2 and a.n_runs == 2
    assert a.words.tolist() == [1, 2, 3] and a.offsets.tolist() == [0, 2, 3] and a.bias.tolist() == [1.5, -2.0] and a.run_off.tolist() == [0, 1, 2]
    for name in ("pairs", "words", "offsets", "bias", "run_off", "other"):
        with pytest.raises(AttributeError):
            setattr(a, name, None)
    with pytest.raises(AttributeError):
        del a.pairs
    assert compile_sequence_bias(None, 10, "cpu") is None and compile_sequence_bias({}, 10, "cpu") is None
    assert compile_sequence_bias(a, 10, "cpu") is a and check_sequence_bias(a, 10) is a
    with pytest.raises(ValueError, match="phrase 1"):
        check_sequence_bias(a, 3)                                                # compiled for a larger vocabulary
    with pytest.raises(ValueError, match="phrase 0"):
        compile_sequence_bias({(11,): 1.0}, 10, "cpu")
    key = tuple(sorted(dict(top_k=5, sequence_bias=a).items()))               # what generate_batch_graphed keys its cache with
    assert hash(key) == hash(tuple(sorted(dict(top_k=5, sequence_bias=b).items())))


BAD = (dict(sequence_bias={(5,): NAN}), dict(sequence_bias={(5,): INF}), dict(sequence_bias={(5,): True}), dict(sequence_bias={(5,): 1e5}),
       dict(sequence_bias={(1000,): 1.0}), dict(sequence_bias={(-2,): 1.0}), dict(sequence_bias=[((), 1.0)]), dict(sequence_bias=[([1] * 33, 1.0)]),
       dict(sequence_bias=[((1,), 1.0)] * 4097), dict(sequence_bias=[[5]]), dict(sequence_bias={(1.5,): 1.0}))
BAD_TYPE = (dict(sequence_bias="word"), dict(sequence_bias=7))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_values_fail_before_the_encoder(kind):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    model.encode = boom
    images = torch.zeros(1, 3, 224, 224)
    for group, exc in ((BAD, ValueError), (BAD_TYPE, TypeError)):
        for bad in group:
            for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
                with pytest.raises(exc):
                    call(images, **bad)
            with pytest.raises(exc):
                model.decode((None,) if kind == "CaptioningLSTM" else (None, None), **bad)    # (the decoder's own check)
            with pytest.raises(exc):
                if kind == "CaptioningLSTM":
                    model.decoder.generate_batch(torch.zeros(1, 256), **bad)
                else:
                    model.decoder.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), **bad)


def test_reforward_decoder_refuses_it_before_the_encoder():
    import deephumor_amd.models as M
    sd, hp = synthetic_sd("CaptioningTransformer")
    model = M.CaptioningTransformer(**dict(hp, pad_index=1)).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    model.encode = boom
    images = torch.zeros(1, 3, 224, 224)
    for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
        with pytest.raises(NotImplementedError, match="sequence_bias with pad_index == 1"):
            call(images, sequence_bias={(5,): 2.0})
    with pytest.raises(NotImplementedError, match="sequence_bias with pad_index == 1"):
        model.decoder.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), sequence_bias={(5,): 2.0})


def test_keyword_rides_in_kw_and_parameter_lists_stay():
    import deephumor_amd.models as M
    from deephumor_amd.models.beam import BeamSearchHelper
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder
    fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
    fns += [TransformerDecoder.generate_batch, SelfAttentionTransformerDecoder.generate_batch, LSTMDecoder.generate]
    for fn in fns:
        ps = inspect.signature(fn).parameters
        assert "sequence_bias" not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # (the signatures of every public callable, and the keyword on its way to DecodeSettings.from_kw: test_decode_settings_cpu)
    assert "sequence_bias" not in inspect.signature(LSTMDecoder.generate_batch).parameters
    with pytest.raises(TypeError, match="unexpected keyword"):
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), sequence_bias=None, no_such_keyword=1)
    # the helper: a method, the constructor's list ends where it ended
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    assert list(inspect.signature(BeamSearchHelper.set_sequence_bias).parameters) == ["self", "sequence_bias"]


# ---- the settings record ----------------------------------------------------------------------------------------------------------
def test_record_key_hash_pickle_and_replace():
    from deephumor_amd.models.beam import DecodeSettings, SequenceBias
    fields = [f.name for f in dataclasses.fields(DecodeSettings)]
    assert fields == DECODE_FIELDS
    bias = {(17,): 4.0, (230, 45): -2.5}
    pairs = (((17,), 4.0), ((230, 45), -2.5))
    plain = DecodeSettings.from_kw({}, 25, 1000)
    none = DecodeSettings.from_kw(dict(sequence_bias=None), 25, 1000)
    empty = DecodeSettings.from_kw(dict(sequence_bias={}), 25, 1000)
    on = DecodeSettings.from_kw(dict(sequence_bias=bias), 25, 1000)
    assert plain.sequence_bias is None and none == plain == empty and hash(none) == hash(plain) and type(plain.search) is str
    assert on.sequence_bias == pairs and on.search == "sample" and type(on.search) is str and on != plain
    assert dataclasses.replace(on, sequence_bias=None) == plain
    same = DecodeSettings.from_kw(dict(sequence_bias=[((17,), 4), ([230, 45], -2.5)]), 8, 1000)
    assert same == on and hash(same) == hash(on) and len({on, same, plain}) == 2
    for other in ({(17,): 4.5, (230, 45): -2.5}, {(230, 45): -2.5, (17,): 4.0}, {(17,): 4.0}):
        assert DecodeSettings.from_kw(dict(sequence_bias=other), 25, 1000) != on
    # with groups: the bias in front of the groups' pair
    both = DecodeSettings.from_kw(dict(sequence_bias=bias, search="beam", num_beam_groups=2, diversity_penalty=0.5, beam_size=4), 25, 1000)
    assert both.sequence_bias == pairs and (both.num_beam_groups, both.diversity_penalty) == (2, 0.5) and both.search == "beam"
    beam_on = DecodeSettings.from_kw(dict(sequence_bias=bias, search="beam", length_penalty=1.5), 25, 1000)
    assert beam_on.length_penalty == 1.5 and beam_on.sequence_bias == pairs and type(beam_on.search) is str
    # replace / compiled / pickle keep it
    r = dataclasses.replace(on, top_p=0.5)
    assert r.sequence_bias == pairs and r.top_p == 0.5 and r != on
    assert dataclasses.replace(on, search="sample") == on                               # the list is a field of its own: it stays
    assert DecodeSettings.from_kw(dict(search=on.search), 25, 1000) == plain            # ... and only its keyword sets it
    c = on.compiled("cpu")
    assert isinstance(c.sequence_bias, SequenceBias) and c.sequence_bias.pairs == pairs and c == on and hash(c) == hash(on)
    assert c.compiled("cpu").sequence_bias is c.sequence_bias and c.sequence_bias.num_tokens == 1000
    assert DecodeSettings.from_kw(dict(sequence_bias=c.sequence_bias), 25, 1000) == on    # a SequenceBias passes through
    cb = beam_on.compiled("cpu")
    assert cb.length_penalty == 1.5 and cb.search == "beam" and isinstance(cb.sequence_bias, SequenceBias)
    assert plain.compiled("cpu").sequence_bias is None and type(plain.compiled("cpu").search) is str
    p = pickle.loads(pickle.dumps(on))
    assert p == on and hash(p) == hash(on) and p.sequence_bias == pairs and p.search == "sample"
    # the bad value raises behind every older control's
    with pytest.raises(ValueError, match="top_p"):
        DecodeSettings.from_kw(dict(top_p=2, sequence_bias={(5,): NAN}), 25, 1000)
    with pytest.raises(ValueError, match="sequence_bias"):
        DecodeSettings.from_kw(dict(sequence_bias={(1000,): 1.0}), 25, 1000)
    kw = dict(sequence_bias=bias)
    DecodeSettings.from_kw(kw, 25, 1000)
    assert kw == dict(sequence_bias=bias)                                               # read, not removed


def test_helper_set_sequence_bias_and_method_surface():
    from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings, SequenceBias, compile_sequence_bias
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
    assert h.sequence_bias is None
    logits = torch.zeros(3, 8)
    for given in ({(4, 5): 2.0}, [((4,), -1.0)], compile_sequence_bias({(4,): 1.0}, 8, "cpu")):
        h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
        assert h.set_sequence_bias(given) is h and isinstance(h.sequence_bias, SequenceBias)
        with pytest.raises(NotImplementedError, match="sequence_bias"):
            h.sample_k_indices(logits)
        with pytest.raises(NotImplementedError):
            h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))
    for off in (None, {}, []):
        assert BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_sequence_bias(off).sequence_bias is None
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_sequence_bias({(4,): NAN})
    with pytest.raises(TypeError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_sequence_bias("word")
    s = DecodeSettings.from_kw(dict(sequence_bias={(4,): 2.0}), 25, 8).compiled("cpu")
    h = s.new_helper(temperature=1.0, beam_size=3, top_k=5, device="cpu")
    assert h.sequence_bias is s.sequence_bias
    assert DecodeSettings.from_kw({}, 25, 8).new_helper(temperature=1.0, beam_size=3, top_k=5, device="cpu").sequence_bias is None


# ---- the text helper --------------------------------------------------------------------------------------------------------------
def test_sequence_bias_from_words_word_and_character_tokenizer():
    from deephumor_amd.data import SPECIAL_TOKENS, CharTokenizer, Vocab, WordPunctTokenizer
    from deephumor_amd.experiments import bad_words_to_ids, sequence_bias_from_words, text_to_seq
    from deephumor_amd.models.beam import check_sequence_bias
    g = json.load(open(os.path.join(GOLDEN, "g8_text_and_metrics.json")))
    wv, cv, wt, ct = Vocab(g["word_vocab"]), Vocab(g["char_vocab"]), WordPunctTokenizer(), CharTokenizer()
    unk, eos = wv.stoi[SPECIAL_TOKENS["UNK"]], wv.stoi[SPECIAL_TOKENS["EOS"]]
    known = [t for t in wv.tokens if t.isalpha()][:3]
    assert len(known) == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # nothing is skipped: no warning
        pairs = sequence_bias_from_words({known[0].upper(): 4.0, known[1] + " " + known[2]: -2.0, "": 1.0}, wv, wt)
    assert pairs == [((wv.stoi[known[0]],), 4.0), ((wv.stoi[known[1]], wv.stoi[known[2]]), -2.0)]          # lower-cased; a phrase; '' skipped
    assert list(pairs[1][0]) == text_to_seq(known[1] + " " + known[2], wv, wt)[0].tolist()
    assert [list(w) for w, _ in pairs] == bad_words_to_ids([known[0], known[1] + " " + known[2]], wv, wt)  # the same text_to_seq
    assert all(eos not in w and unk not in w for w, _ in pairs)
    with pytest.warns(UserWarning) as rec:
        pairs = sequence_bias_from_words([(known[0], 1.0), ("zzzqqqxxx", 2.0), (known[1] + " zzzqqqxxx", 3.0), ("qqqzzz", 4.0), (known[0], -1.0)], wv, wt)
    assert pairs == [((wv.stoi[known[0]],), 1.0), ((wv.stoi[known[0]],), -1.0)] and len(rec) == 1 and "3 of 5" in str(rec[0].message)
    assert check_sequence_bias(pairs, len(wv)) == tuple(pairs)
    # the character tokenizer: a word is a run of characters; the bias lands on its last one behind the others, inside longer words too
    chars = [t for t in cv.tokens if len(t) == 1 and t.isalpha()]
    word = "".join(chars[:3])
    pairs = sequence_bias_from_words({word: 3.0}, cv, ct)
    assert pairs == [(tuple(cv.stoi[ch] for ch in word), 3.0)]
    longer = text_to_seq(chars[3] + word[:2], cv, ct)[0].tolist()
    assert brute_fired(longer, pairs) == [0] and brute_fired(longer[:-1], pairs) == []
    doc = sequence_bias_from_words.__doc__
    assert "LAST token" in doc and "SUBSTRING" in doc


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
ARGS = ["logits", "ldl", "V", "group_max", "gm_ld", "n_groups", "group_cols", "tokens", "tok_ld", "tok_row_mult", "pos", "rows",
        "rows_per_img", "first_pos", "words", "word_off", "bias", "run_off", "n_words", "n_runs", "stream"]


def test_abi_header_table_and_library_agree():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NAME + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[NAME]
    assert len(args) == len(sig) == 21
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, NAME)
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35
    # one new symbol, no prototype moved
    assert len(_abi.SIGNATURES["dh_beam_history_logits"]) == 17 and len(_abi.SIGNATURES["dh_beam_constrain_logits"]) == 20
    assert len(_abi.SIGNATURES["dh_beam_row_sample_groups"]) == 22 and len(_abi.SIGNATURES["dh_beam_row_best"]) == 18
    readme = open(os.path.join(ROOT, "README.md")).read()
    n_protos = len(re.findall(r"^(?:int|const char\*|void|unsigned long long|double|float)\s+\*?dh_\w+\s*\(", text, flags=re.M))
    assert f"{n_protos} entry points" in readme and n_protos == 129
    assert callable(hip.beam_bias_logits)


def test_entry_point_argument_contract():
    """Checked before any HIP call (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    from deephumor_amd import hip
    fn = getattr(hip.load(), NAME)
    #       logits ldl  V    gmax gm ng gc tokens tok_ld mult pos rows rpi first_pos words off bias runs n_words n_runs stream
    good = [64, 128, 100, None, 0, 0, 0, 64, 12, 1, 5, 2, 1, None, 64, 64, 64, 64, 7, 3, None]

    def call(**over):
        a = list(good)
        for k, val in over.items():
            a[ARGS.index(k)] = val
        return fn(*a)
    for over in (dict(n_words=0, n_runs=0), dict(n_words=0),                          # an empty list: the caller makes no launch
                 dict(n_words=-1), dict(n_words=hip.MAX_BAD_WORDS + 1, n_runs=3), dict(n_runs=0), dict(n_runs=-1), dict(n_runs=8),
                 dict(words=None), dict(word_off=None), dict(bias=None), dict(run_off=None),
                 dict(pos=13), dict(pos=-1), dict(logits=None), dict(tokens=None), dict(tok_row_mult=0), dict(rows=0), dict(rows_per_img=0),
                 dict(ldl=99), dict(V=0),
                 dict(group_max=64, gm_ld=2, n_groups=1, group_cols=64),          # 64 columns of groups for V = 100
                 dict(group_max=64, gm_ld=1, n_groups=2, group_cols=64),          # gm_ld < n_groups
                 dict(group_max=64, gm_ld=2, n_groups=2, group_cols=65),
                 dict(group_max=64, gm_ld=2000, n_groups=1025, group_cols=64),
                 dict(first_pos=64, rows=3, rows_per_img=2)):
        assert call(**over) == 1, over


# ---- golden G24 -----------------------------------------------------------------------------------------------------------------
def g24_pairs(g, slot):
    words, offs, bias = g[f"words_{slot}"].tolist(), g[f"offsets_{slot}"].tolist(), g[f"bias_{slot}"].tolist()
    return [(words[a:b], x) for a, b, x in zip(offs[:-1], offs[1:], bias)]


@pytest.mark.parametrize("kind", KINDS)
def test_g24_satisfies_the_tools_assertions(kind):
    """Per slot the list is the one the tool derives from the plain caption -- a positive single on a token the plain caption does
    not hold, of a size from the tool's ladder; -4 on its first token; +3 on its third token behind its second -- and the recorded
    caption differs from the plain one and holds the boosted token (tools/make_bias_golden.py)."""
    from deephumor_amd.models.beam import check_sequence_bias
    from helpers import golden
    g = golden(f"g24_sequence_bias_{kind}.npz")
    max_len = int(g["max_len"])
    assert max_len == (6 if kind in ("CaptioningTransformer", "CaptioningTransformerWithLabels") else 12)
    assert int(g["n_slots"]) == 2
    for slot in range(2):
        out, plain, pairs = g[f"out_{slot}"].tolist(), g[f"plain_{slot}"].tolist(), g24_pairs(g, slot)
        boost, size = int(g[f"boost_{slot}"]), float(g[f"boost_size_{slot}"])
        assert int(g[f"image_{slot}"]) == slot and size in (2.0, 4.0, 8.0, 16.0, 32.0)
        assert boost == next(t for t in range(10, 30) if t not in plain)
        assert pairs == [([boost], size), ([plain[0]], -4.0), (plain[1:3], 3.0)]
        assert 1 <= len(out) <= max_len and out != plain and boost in out and boost not in plain and int(g[f"edited_{slot}"]) > 0
        assert check_sequence_bias(pairs, 1000) == tuple((tuple(w), b) for w, b in pairs)
