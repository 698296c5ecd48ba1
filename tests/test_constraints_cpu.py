"""``min_len`` / ``bad_words_ids`` without a GPU: the restatement (``tests/constraints_ref.py``) against its brute-force scan, what the
kernel cases hold, ``beam.check_constraints`` on every public entry before the encoder runs, ``BadWords``, the text helper, the
signatures, the ABI of ``dh_beam_constrain_logits`` with its argument contract, and golden G22's own rule."""
import ctypes
import inspect
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from constraints_ref import (CASE_VS, EOS, NEG_INF, UNK, banned_phrase_in, brute_banned, brute_constrain_row, constrain_logits, eos_below,
                             fires, flatten, kernel_cases)
from helpers import GOLDEN, KINDS, golden, synthetic_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dh_beam_constrain_logits"


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_brute_force_scan(seed):
    """Random histories over a small alphabet and random lists of 1 .. 4-id phrases over the same alphabet (so that many fire),
    ids outside ``[0, V)`` among the last ids, every ``pos`` from 0 on, ``min_len`` on both sides of ``pos``."""
    g = torch.Generator().manual_seed(seed)
    for v, alphabet in ((130, 4), (70, 6), (200, 3)):
        rows, width = 5, 9
        hist = torch.randint(0, alphabet, (rows, width), generator=g)
        phrases = [torch.randint(0, alphabet, (int(torch.randint(1, 5, (1,), generator=g)),), generator=g).tolist() for _ in range(12)]
        phrases += [[0, v + 2], [1, -3], [1, v - 1], phrases[0]]
        logits = torch.randn(rows, v, generator=g) * 3
        logits[0, :3] = torch.tensor([0.0, -0.0, NEG_INF])
        gm0 = torch.full((rows, (v + 63) // 64 + 1), 777.0)             # poison: one word more than there are groups
        for pos in range(width + 1):
            for min_len in (0, pos, pos + 1):
                out, gm, stored = constrain_logits(logits, hist, pos, phrases, min_len, EOS, gm0, 64)
                for r in range(rows):
                    bx, bgm, bst = brute_constrain_row(logits[r], hist[r, :pos].tolist(), phrases, min_len, EOS, gm0[r], 64)
                    assert torch.equal(out[r], bx) and torch.equal(gm[r], bgm), (v, pos, min_len, r)
                    assert stored[r].nonzero().flatten().tolist() == bst
                assert bool((gm[:, -1] == 777.0).all())
                assert bool(stored[:, EOS].all()) == (pos < min_len) or any(w[-1] == EOS for w in phrases)


def test_the_two_rules_on_small_examples():
    # a single id is banned at every position, the empty history included
    assert brute_banned([], [[7]]) == {7} and brute_banned([1, 2, 3], [[7]]) == {7}
    # a phrase fires only when its prefix ENDS the history
    assert brute_banned([5, 6], [[5, 6, 9]]) == {9} and brute_banned([5, 6, 1], [[5, 6, 9]]) == set()
    assert brute_banned([6], [[5, 6, 9]]) == set() and brute_banned([], [[5, 9]]) == set()      # l - 1 > s
    assert brute_banned([5], [[5, 9], [5, 8], [4, 7]]) == {9, 8}
    # <eos> below min_len only; a phrase may hold <eos>
    assert brute_banned([1, 2], [], min_len=3, eos=3) == {3} and brute_banned([1, 2, 4], [], min_len=3, eos=3) == set()
    assert brute_banned([1], [[1, 3]], min_len=0, eos=3) == {3}
    x = torch.arange(8.0)[None, :]
    out, gm, stored = constrain_logits(x, torch.tensor([[5]]), 1, [[5, 7], [2]], 2, 3, torch.full((1, 1), 777.0), 64)
    assert stored[0].nonzero().flatten().tolist() == [2, 3, 7] and gm[0, 0] == 6.0
    assert bool((out[0, [2, 3, 7]] == NEG_INF).all()) and out[0, 6] == 6.0
    # a group whose columns are all banned; an untouched group keeps its word
    out, gm, _ = constrain_logits(torch.zeros(1, 70), torch.zeros(1, 0), 0, [[c] for c in range(64)], 0, -1, torch.full((1, 2), 777.0), 64)
    assert gm[0].tolist() == [NEG_INF, 777.0]
    # inactive rows keep every word
    out, gm, stored = constrain_logits(x.repeat(2, 1), torch.tensor([[5], [5]]), 1, [[5, 7]], 2, 3, torch.full((2, 1), 777.0), 64,
                                       active=torch.tensor([False, True]))
    assert torch.equal(out[0], x[0]) and gm[0, 0] == 777.0 and not stored[0].any() and stored[1].any()
    # the host scans
    assert banned_phrase_in([1, 5, 7, 2], [[5, 7]]) == ((5, 7), 2) and banned_phrase_in([1, 5, 7, 2], [[5, 7]], start=3) is None
    assert banned_phrase_in([1, 5, 2, 7], [[5, 7]]) is None
    assert eos_below([1, 3, 2], 2, 3) and not eos_below([1, 2, 3], 2, 3) and not eos_below([3, 1, 2], 2, 3, start=1)


@pytest.mark.parametrize("v", CASE_VS)
def test_kernel_cases_hold_what_they_promise(v):
    """On the reference alone, for every kernel case: a multi-token phrase fires in some row, a multi-token phrase fires in no row,
    and a group becomes all ``-inf``.  At ``pos = 0`` no multi-token phrase CAN fire (``l - 1 <= pos`` leaves only singles): there
    the first statement is replaced by its opposite -- every one of them is a phrase longer than ``pos + 1``."""
    cases = kernel_cases(v)
    assert [c["pos"] for c in cases] == [0, 1, 5, 40, 5] and [c["rows"] for c in cases] == [12, 12, 12, 12, 4]
    assert cases[-1]["mult"] == 3 and cases[-1]["table"].shape[0] == 12
    for c in cases:
        pos, phrases, named = c["pos"], c["phrases"], c["named"]
        h = c["table"][::c["mult"]]
        assert len(phrases) == 300 and max(len(w) for w in phrases) == 32 and min(len(w) for w in phrases) == 1
        assert phrases.count(named["A"]) == 2 and named["A"][-1] == named["A2"][-1]                  # a duplicate; one last id twice
        assert [v - 1] != phrases[-1] and any(w[-1] == v - 1 and len(w) > 1 for w in phrases)
        assert all([64 + k] in phrases for k in range(64))
        multi = [w for w in phrases if len(w) > 1]
        fired = [bool(fires(h, pos, w).any()) for w in multi]
        if pos == 0:
            assert not any(fired) and all(len(w) > pos + 1 for w in multi)
        else:
            assert any(fired)
            assert bool(fires(h, pos, named["A"]).any()) and bool(fires(h, pos, named["A2"]).any())
            assert not bool(fires(h, pos, named["A"]).all())                                           # the bans are the rows' own
        assert not all(fired) and not any(bool(fires(h, pos, w).any()) for w in named["never"])
        assert bool(fires(h, pos, named["B"]).any()) == (pos >= 4)
        if pos >= 4:                         # the near miss: its last prefix id matches, the one before does not
            assert h[3, pos - 1] == named["B"][3] and h[3, pos - 2] != named["B"][2] and not bool(fires(h, pos, named["B"])[3])
        assert bool(fires(h, pos, named["C"]).any()) == (pos == 40)
        if pos < 31:
            assert len(named["C"]) > pos + 1
        for min_len in c["min_lens"]:
            gm0 = torch.full((c["rows"], (v + 63) // 64), 777.0)
            out, gm, stored = constrain_logits(c["logits"], h, pos, phrases, min_len, c["eos"], gm0, 64)
            assert bool((gm[:, 1] == NEG_INF).all()) and bool((out[:, 64:128] == NEG_INF).all())        # group 1: all 64 columns
            assert bool(stored[:, c["eos"]].all()) == (pos < min_len)
            if pos >= 1:
                assert bool(stored[0, v - 1]) and not bool(stored[3, v - 1])                           # column V - 1, last partial group
                assert gm[0, (v - 1) // 64] == out[0, (v - 1) // 64 * 64:v].max()
        assert sorted(c["min_lens"]) == [0, pos, pos + 2] if pos else sorted(c["min_lens"]) == [0, 0, 2]


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_check_constraints():
    from deephumor_amd import hip
    from deephumor_amd.models.beam import check_constraints
    assert check_constraints() == (0, None) and check_constraints(3, [], 10) == (3, None)
    assert check_constraints(np.int64(2), [[1, 2], (3,)], 5, 10) == (2, ((1, 2), (3,)))
    assert isinstance(check_constraints(np.int32(2), None, 5)[0], int)
    m, ids = check_constraints(0, [np.array([1, 2]), torch.tensor([3]), [np.int64(4)], [7], [7]], None, 10)
    assert ids == ((1, 2), (3,), (4,), (7,), (7,)) and all(type(t) is int for w in ids for t in w)      # duplicates stay
    assert check_constraints(0, [[EOS, EOS]], None, 10)[1] == ((EOS, EOS),)                               # a phrase may hold <eos>
    for bad in (True, False, -1):
        with pytest.raises(ValueError):
            check_constraints(bad)
    for bad in (2.0, "2", None, [2], torch.tensor(2)):
        with pytest.raises(TypeError):
            check_constraints(bad)
    for m, t in ((5, 5), (6, 5), (25, 25)):
        with pytest.raises(ValueError, match="max_len"):
            check_constraints(m, None, t)
    check_constraints(4, None, 5)
    assert (hip.MAX_BAD_WORDS, hip.MAX_BAD_LEN) == (4096, 32)
    check_constraints(0, [[1] * 32], None, 10)
    check_constraints(0, [[1]] * 4096, None, 10)
    for bad, phrase in (([[1], []], "phrase 1"), ([[1], [2, 10]], "phrase 1"), ([[-1]], "phrase 0"), ([[1, 2.0]], "phrase 0"),
                        ([[1], [2], ["a"]], "phrase 2"), ([[True]], "phrase 0"), ([[1] * 33], "phrase 0"), ([[1]] * 4097, "phrase 4096"),
                        ([1, 2], "phrase 0"), ([[1], "ab"], "phrase 1"), ([[None]], "phrase 0")):
        with pytest.raises(ValueError, match=phrase):
            check_constraints(0, bad, None, 10)
    check_constraints(0, [[2, 10]], None, None)                   # no vocabulary size given: only the lower bound
    for bad in ("abc", 5, b"ab"):
        with pytest.raises(TypeError):
            check_constraints(0, bad, None, 10)


def test_bad_words_is_immutable_hashable_and_cached():
    from deephumor_amd.models.beam import BadWords, check_constraints, compile_bad_words
    a = compile_bad_words([[1, 2], [3]], 10, "cpu")
    b = compile_bad_words(((1, 2), (3,)), 10, "cpu")
    c = compile_bad_words([[1, 2], [4]], 10, "cpu")
    assert isinstance(a, BadWords) and a == b and hash(a) == hash(b) and a != c and len({a, b, c}) == 2
    assert a.words is b.words and a.offsets is b.offsets                     # the per-device cache: uploaded once
    assert a.ids == ((1, 2), (3,)) and len(a) == a.n_words == 2
    assert a.words.dtype == a.offsets.dtype == torch.int32
    assert a.words.tolist() == [1, 2, 3] and a.offsets.tolist() == [0, 2, 3]
    w, o = flatten([[1, 2], [3]])
    assert torch.equal(w, a.words) and torch.equal(o, a.offsets)
    for name in ("ids", "words", "offsets", "other"):
        with pytest.raises(AttributeError):
            setattr(a, name, None)
    with pytest.raises(AttributeError):
        del a.ids
    assert compile_bad_words(None, 10, "cpu") is None and compile_bad_words([], 10, "cpu") is None
    assert compile_bad_words(a, 10, "cpu") is a and check_constraints(0, a, None, 10) == (0, a)
    with pytest.raises(ValueError, match="phrase 1"):
        check_constraints(0, a, None, 3)                                         # compiled for a larger vocabulary
    with pytest.raises(ValueError, match="phrase 0"):
        compile_bad_words([[11]], 10, "cpu")
    key = tuple(sorted(dict(top_k=5, bad_words_ids=a, min_len=2).items()))       # what generate_batch_graphed keys its cache with
    assert hash(key) == hash(tuple(sorted(dict(top_k=5, bad_words_ids=b, min_len=2).items())))


BAD = (dict(min_len=-1), dict(min_len=True), dict(min_len=25), dict(min_len=7, max_len=7), dict(bad_words_ids=[[]]),
       dict(bad_words_ids=[[5], [1000]]), dict(bad_words_ids=[[-2]]), dict(bad_words_ids=[[1.5]]), dict(bad_words_ids=[[1] * 33]),
       dict(bad_words_ids=[[1]] * 4097), dict(bad_words_ids=[3, 4]))
BAD_TYPE = (dict(min_len=2.0), dict(min_len="2"), dict(bad_words_ids="word"), dict(bad_words_ids=7))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_values_fail_before_the_encoder(kind):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()                    # (CaptionPipeline needs a device: tests/test_constraints_gpu.py)

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


def test_keyword_only_and_positional_prefixes():
    import deephumor_amd.models as M
    from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder
    for name, default in (("min_len", 0), ("bad_words_ids", None)):
        assert getattr(DecodeSettings(), name) == default        # (the signatures and the keyword's way down: test_decode_settings_cpu)
        fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
        fns += [TransformerDecoder.generate_batch, SelfAttentionTransformerDecoder.generate_batch, LSTMDecoder.generate]
        for fn in fns:                                            # everywhere else the keywords ride in **kw
            ps = inspect.signature(fn).parameters
            assert name not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # LSTMDecoder.generate_batch keeps the parameter list it had and takes the two keywords by name
    names = list(inspect.signature(LSTMDecoder.generate_batch).parameters)
    assert names[19:] == ["return_beams", "top_p", "no_repeat_ngram_size", "repetition_penalty", "kw"]
    with pytest.raises(TypeError, match="unexpected keyword"):
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), min_len=0, no_such_keyword=1)
    # the helper: a method, the constructor's list ends where it ended
    assert list(inspect.signature(BeamSearchHelper.set_constraints).parameters) == ["self", "min_len", "bad_words_ids"]


def test_helper_set_constraints_and_method_surface():
    from deephumor_amd.models.beam import BadWords, BeamSearchHelper, compile_bad_words
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
    assert (h.min_len, h.bad_words) == (0, None)
    logits = torch.zeros(3, 8)
    for kw in (dict(min_len=2), dict(bad_words_ids=[[4, 5]]), dict(bad_words_ids=compile_bad_words([[4]], 8, "cpu"))):
        h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
        assert h.set_constraints(**kw) is h
        assert h.min_len == kw.get("min_len", 0) and isinstance(h.bad_words, BadWords) == ("bad_words_ids" in kw)
        with pytest.raises(NotImplementedError, match="min_len"):
            h.sample_k_indices(logits)
        with pytest.raises(NotImplementedError):
            h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))
    assert BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_constraints(0, []).bad_words is None
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", max_len=10).set_constraints(min_len=10)
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_constraints(bad_words_ids=[[]])
    with pytest.raises(TypeError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_constraints(min_len=2.0)


# ---- the text helper --------------------------------------------------------------------------------------------------------------
def test_bad_words_to_ids_word_and_character_tokenizer():
    from deephumor_amd.data import SPECIAL_TOKENS, CharTokenizer, Vocab, WordPunctTokenizer
    from deephumor_amd.experiments import bad_words_to_ids, text_to_seq
    g = json.load(open(os.path.join(GOLDEN, "g8_text_and_metrics.json")))
    wv, cv, wt, ct = Vocab(g["word_vocab"]), Vocab(g["char_vocab"]), WordPunctTokenizer(), CharTokenizer()
    unk, eos = wv.stoi[SPECIAL_TOKENS["UNK"]], wv.stoi[SPECIAL_TOKENS["EOS"]]
    known = [t for t in wv.tokens if t.isalpha()][:3]
    assert len(known) == 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # nothing is skipped: no warning
        ids = bad_words_to_ids([known[0].upper(), known[1] + " " + known[2], ""], wv, wt)
    assert ids == [[wv.stoi[known[0]]], [wv.stoi[known[1]], wv.stoi[known[2]]]]              # lower-cased; a phrase; '' skipped
    assert ids[1] == text_to_seq(known[1] + " " + known[2], wv, wt)[0].tolist()
    assert all(eos not in w and unk not in w for w in ids)
    with pytest.warns(UserWarning) as rec:
        ids = bad_words_to_ids([known[0], "zzzqqqxxx", known[1] + " zzzqqqxxx", "qqqzzz"], wv, wt)
    assert ids == [[wv.stoi[known[0]]]] and len(rec) == 1 and "3 of 4" in str(rec[0].message)
    # the character tokenizer: a word is a run of characters, so it matches inside longer words
    chars = [t for t in cv.tokens if len(t) == 1 and t.isalpha()]
    word = "".join(chars[:3])
    ids = bad_words_to_ids([word], cv, ct)
    assert ids == [[cv.stoi[ch] for ch in word]] and len(ids[0]) == 3
    longer = text_to_seq(chars[3] + word + chars[4], cv, ct)[0].tolist()
    assert banned_phrase_in(longer, ids) == (tuple(ids[0]), 3)
    from deephumor_amd.models.beam import check_constraints
    assert check_constraints(0, ids, None, len(cv))[1] == (tuple(ids[0]),)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
ARGS = ["logits", "ldl", "V", "group_max", "gm_ld", "n_groups", "group_cols", "tokens", "tok_ld", "tok_row_mult", "pos", "rows",
        "rows_per_img", "first_pos", "eos_index", "min_len", "words", "word_off", "n_words", "stream"]


def test_abi_header_table_and_library_agree():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NAME + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[NAME]
    assert len(args) == len(sig) == 20
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    assert int(re.search(r"#define DH_BEAM_MAX_BAD_WORDS (\d+)", header).group(1)) == _abi.MAX_BAD_WORDS == hip.MAX_BAD_WORDS == 4096
    assert int(re.search(r"#define DH_BEAM_MAX_BAD_LEN (\d+)", header).group(1)) == _abi.MAX_BAD_LEN == hip.MAX_BAD_LEN == 32
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, NAME)
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35
    # one new symbol, no prototype moved
    assert len(_abi.SIGNATURES["dh_beam_history_logits"]) == 17 and len(_abi.SIGNATURES["dh_beam_row_sample_groups"]) == 22
    assert len(_abi.SIGNATURES["dh_beam_row_sample_nucleus"]) == 25 and len(_abi.SIGNATURES["dh_beam_select"]) == 26
    readme = open(os.path.join(ROOT, "README.md")).read()
    n_protos = len(re.findall(r"^(?:int|const char\*|void|unsigned long long|double|float)\s+\*?dh_\w+\s*\(", text, flags=re.M))
    assert f"{n_protos} entry points" in readme


def test_entry_point_argument_contract():
    """Checked before any HIP call (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    from deephumor_amd import hip
    fn = getattr(hip.load(), NAME)
    #       logits ldl  V    gmax gm ng gc tokens tok_ld mult pos rows rpi first_pos eos min_len words off n_words stream
    good = [64, 128, 100, None, 0, 0, 0, 64, 12, 1, 5, 2, 1, None, 3, 0, 64, 64, 7, None]

    def call(**over):
        a = list(good)
        for k, val in over.items():
            a[ARGS.index(k)] = val
        return fn(*a)
    for over in (dict(n_words=0), dict(n_words=0, min_len=5),                         # nothing to ban: the caller makes no launch
                 dict(n_words=-1), dict(n_words=hip.MAX_BAD_WORDS + 1), dict(words=None), dict(word_off=None), dict(min_len=-1),
                 dict(pos=13), dict(pos=-1), dict(logits=None), dict(tokens=None), dict(tok_row_mult=0), dict(rows=0), dict(ldl=99),
                 dict(group_max=64, gm_ld=2, n_groups=1, group_cols=64),          # 64 columns of groups for V = 100
                 dict(group_max=64, gm_ld=1, n_groups=2, group_cols=64),          # gm_ld < n_groups
                 dict(group_max=64, gm_ld=2, n_groups=2, group_cols=65),
                 dict(group_max=64, gm_ld=2000, n_groups=1025, group_cols=64),
                 dict(first_pos=64, rows=3, rows_per_img=2)):
        assert call(**over) == 1, over


# ---- golden G22 -----------------------------------------------------------------------------------------------------------------
def g22_slot(g, slot):
    words, offs = g[f"words_{slot}"].tolist(), g[f"offsets_{slot}"].tolist()
    return [words[a:b] for a, b in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize("kind", KINDS)
def test_g22_satisfies_the_tools_assertions(kind):
    """Slots 0 / 1: the reference's ``<eos>``, the list with the plain caption's first token as a single.  Slots 2 / 3: an
    ``eos_index`` that ends the plain caption early, so that ``min_len`` bites; no single (tools/make_constraints_golden.py)."""
    from deephumor_amd.models.beam import check_constraints
    g = golden(f"g22_constraints_{kind}.npz")
    max_len = int(g["max_len"])
    assert max_len == (6 if kind in ("CaptioningTransformer", "CaptioningTransformerWithLabels") else 12)
    assert int(g["n_slots"]) == 4
    length = lambda toks, eos: toks.index(eos) + 1 if eos in toks else len(toks)
    for slot in range(4):
        out, plain, min_len, eos = g[f"out_{slot}"].tolist(), g[f"plain_{slot}"].tolist(), int(g[f"min_len_{slot}"]), int(g[f"eos_{slot}"])
        phrases = g22_slot(g, slot)
        assert int(g[f"image_{slot}"]) == slot % 2 and (eos == EOS) == (slot < 2)
        # the controls are the ones the tool derives from the plain caption
        n = length(plain, eos)
        assert min_len == (min(n + 2, max_len - 1) if n < max_len else 0) and 0 <= min_len < max_len
        want = ([[plain[0]]] if slot < 2 else []) + ([plain[1:3]] if len(plain) >= 3 else []) + [[UNK, 5]]
        assert phrases == want
        if slot >= 2:
            assert n < max_len and min_len > 0 and eos_below(plain, min_len, eos)          # the plain caption does end early
        # and the recorded caption obeys them
        assert 1 <= len(out) <= max_len and banned_phrase_in(out[:length(out, eos)], phrases) is None
        assert not eos_below(out, min_len, eos) and out != plain and int(g[f"edited_{slot}"]) > 0
        check_constraints(min_len, phrases, max_len, 1000)
