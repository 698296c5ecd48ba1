"""The shared pieces of the Python decode layer, on the CPU: ``beam.DecodeSettings`` against the ``check_*`` functions it runs, the one
row-draw path of ``BeamSearchHelper.step`` / ``step_prompted`` against its dispatch table, ``decode_with_overflow_retry`` and
``SessionResult``."""
import inspect
import itertools
import warnings

import numpy as np
import pytest
import torch

from deephumor_amd import hip
from deephumor_amd.models import beam
from deephumor_amd.models.beam import (BadWords, BeamCaptions, BeamOverflow, BeamSearchHelper, DecodeSettings, SessionResult,
                                       check_constraints, check_repeat, check_return_attention, check_return_beams, check_top_p,
                                       decode_with_overflow_retry)

INF, NAN = float("inf"), float("nan")
# every value the validation tests of the four features accept or reject (test_nucleus_cpu, test_repeat_cpu, test_constraints_cpu,
# test_attention_maps_cpu), one setting at a time; ``max_len`` / ``num_tokens`` beside a setting are from_kw's arguments
VALUES = (
    [dict(top_p=v) for v in (1.0, 1, 0.8, 1e-6, np.float32(0.5), np.float64(0.97), True, False, NAN, 0, 0.0, -0.1, 1.0000001, 1.5, 2, INF,
                             "0.8", None, [0.8], torch.tensor(0.8), 0.5 + 0j)]
    + [dict(no_repeat_ngram_size=v) for v in (0, 3, np.int64(2), np.int32(2), True, False, -1, 2.0, "2", None, [2], torch.tensor(2))]
    + [dict(repetition_penalty=v) for v in (1, 1.3, np.float32(0.5), True, False, 0, 0.0, -1.3, NAN, INF, "1.3", None, [1.3],
                                            torch.tensor(1.3), 1.3 + 0j)]
    + [dict(no_repeat_ngram_size=n, repetition_penalty=p, max_len=m)
       for n, p, m in ((0, 1.0, hip.MAX_HISTORY + 1), (2, 1.3, hip.MAX_HISTORY), (2, 1.0, hip.MAX_HISTORY + 1), (0, 1.3, hip.MAX_HISTORY + 1),
                       (2, 1.0, 5000), (0, 1.2, 5000))]
    + [dict(min_len=v) for v in (0, 3, np.int64(2), np.int32(2), True, False, -1, 25, 2.0, "2", None, [2], torch.tensor(2))]
    + [dict(min_len=m, max_len=t) for m, t in ((5, 5), (6, 5), (25, 25), (4, 5), (7, 7))]
    + [dict(bad_words_ids=v, num_tokens=10)
       for v in (None, [], [[1, 2], (3,)], [np.array([1, 2]), torch.tensor([3]), [np.int64(4)], [7], [7]], [[3, 3]], [[1] * 32], [[1]] * 4096,
                 [[1], []], [[1], [2, 10]], [[-1]], [[1, 2.0]], [[1], [2], ["a"]], [[True]], [[1] * 33], [[1]] * 4097, [1, 2], [[1], "ab"],
                 [[None]], "abc", 5, b"ab", "word", 7, [[]], [[-2]], [[1.5]], [3, 4])]
    + [dict(bad_words_ids=[[5], [1000]], num_tokens=1000), dict(bad_words_ids=[[2, 10]], num_tokens=None)]
    + [dict(return_attention=v) for v in (False, True, 1, 0, None, "yes", torch.tensor(True), 1.0)]
    + [dict(return_beams=v) for v in (False, True, 1, 0, None, "yes", torch.tensor(True))])


def outcome(fn):
    try:
        return "returned", fn()
    except Exception as e:          # noqa: BLE001  (the exception IS the outcome)
        return type(e), str(e)


def by_the_checks(kw, max_len, num_tokens, model=None):
    """The individual calls, in the documented order, on ``from_kw``'s defaults."""
    return (check_return_beams(kw.get("return_beams", False)), check_return_attention(kw.get("return_attention", False), model),
            check_top_p(kw.get("top_p", 1.0)), *check_repeat(kw.get("no_repeat_ngram_size", 0), kw.get("repetition_penalty", 1.0), max_len),
            *check_constraints(kw.get("min_len", 0), kw.get("bad_words_ids"), max_len, num_tokens))


def as_tuple(s):
    return (s.return_beams, s.return_attention, s.top_p, s.no_repeat_ngram_size, s.repetition_penalty, s.min_len, s.bad_words_ids)


@pytest.mark.parametrize("case", VALUES, ids=[f"{i}-{'-'.join(c)}" for i, c in enumerate(VALUES)])
def test_from_kw_returns_or_raises_what_the_checks_do(case):
    kw = dict(case)
    max_len, num_tokens = kw.pop("max_len", 25), kw.pop("num_tokens", 1000)
    before = dict(kw)
    want = outcome(lambda: by_the_checks(kw, max_len, num_tokens))
    got = outcome(lambda: as_tuple(DecodeSettings.from_kw(kw, max_len, num_tokens)))
    assert got == want
    assert kw.keys() == before.keys() and all(kw[k] is before[k] for k in kw)           # read, not removed
    if got[0] == "returned":
        assert [type(v) for v in got[1][:6]] == [bool, bool, float, int, float, int]


def test_from_kw_hands_the_model_to_check_return_attention():
    class NoCross:
        _cross = False

    class Reforward:
        _cross, pad_index = True, 1

    class Cross:
        _cross, pad_index = True, 0
    for model, exc in ((NoCross(), TypeError), (Reforward(), NotImplementedError)):
        assert DecodeSettings.from_kw(dict(return_attention=False), 25, 10, model).return_attention is False
        with pytest.raises(exc):
            DecodeSettings.from_kw(dict(return_attention=True), 25, 10, model)
    assert DecodeSettings.from_kw(dict(return_attention=True), 25, 10, Cross()).return_attention is True


@pytest.mark.parametrize("kw,exc,match", [
    (dict(return_beams=1, top_p=2), TypeError, "return_beams"),
    (dict(return_beams=1, return_attention=1), TypeError, "return_beams"),
    (dict(return_attention=1, top_p=2), TypeError, "return_attention"),
    (dict(top_p=2, min_len=-1), ValueError, "top_p"),
    (dict(top_p=2, no_repeat_ngram_size=-1), ValueError, "top_p"),
    (dict(no_repeat_ngram_size=-1, min_len=-1), ValueError, "no_repeat_ngram_size"),
    (dict(repetition_penalty="x", bad_words_ids=[[]]), TypeError, "repetition_penalty"),
])
def test_the_earlier_check_raises(kw, exc, match):
    with pytest.raises(exc, match=match):
        DecodeSettings.from_kw(kw, 25, 1000)


def test_records_are_frozen_hashable_and_equal_by_their_settings():
    kw = dict(top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3, min_len=3, bad_words_ids=[[17], [230, 45]], return_beams=True)
    a = DecodeSettings.from_kw(kw, 8, 1000)
    b = DecodeSettings.from_kw(dict(kw, top_p=np.float64(0.8), min_len=np.int64(3), bad_words_ids=((17,), [230, 45])), 25, 1000)
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    for other in (dict(top_p=0.9), dict(min_len=2), dict(bad_words_ids=[[17]]), dict(bad_words_ids=None), dict(return_beams=False),
                  dict(no_repeat_ngram_size=3), dict(repetition_penalty=1.0)):
        assert DecodeSettings.from_kw(dict(kw, **other), 8, 1000) != a
    with pytest.raises(AttributeError):
        a.top_p = 1.0
    c = a.compiled("cpu")
    assert isinstance(c.bad_words_ids, BadWords) and c.bad_words_ids.ids == a.bad_words_ids == ((17,), (230, 45))
    assert c.bad_words_ids.num_tokens == 1000 and c.bad_words_ids is beam.compile_bad_words(a.bad_words_ids, 1000, "cpu")
    assert c == a and hash(c) == hash(a) and c.compiled("cpu").bad_words_ids is c.bad_words_ids
    assert as_tuple(c)[:6] == as_tuple(a)[:6]
    assert DecodeSettings.from_kw(dict(kw, bad_words_ids=c.bad_words_ids), 8, 1000) == a         # a BadWords passes through
    assert DecodeSettings.from_kw({}, 25).compiled("cpu").bad_words_ids is None


def test_new_helper_is_the_constructor_then_set_constraints(monkeypatch):
    s = DecodeSettings.from_kw(dict(top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3, min_len=3, bad_words_ids=[[17]]), 8, 1000)
    calls = []
    real_init, real_set = BeamSearchHelper.__init__, BeamSearchHelper.set_constraints
    monkeypatch.setattr(BeamSearchHelper, "__init__", lambda self, *a, **k: (calls.append(("init", a, k)), real_init(self, *a, **k))[1])
    monkeypatch.setattr(BeamSearchHelper, "set_constraints", lambda self, *a, **k: (calls.append(("set", a, k)), real_set(self, *a, **k))[1])
    h = s.new_helper(temperature=1.2, beam_size=2, top_k=5, eos_index=4, device="cpu", n_img=3, max_len=8, seed=7, img0=2)
    assert calls == [("init", (), dict(temperature=1.2, beam_size=2, top_k=5, eos_index=4, device="cpu", n_img=3, max_len=8, seed=7, img0=2,
                                       top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3)), ("set", (3, ((17,),)), {})]
    assert isinstance(h, BeamSearchHelper) and (h.top_p, h.no_repeat_ngram_size, h.repetition_penalty, h.min_len) == (0.8, 2, 1.3, 3)
    assert h.bad_words.ids == ((17,),) and (h.temperature, h.beam_size, h.top_k, h.eos_index, h.n_img, h.seed, h.img0) == (1.2, 2, 5, 4, 3, 7, 2)
    plain = DecodeSettings.from_kw({}, 8).new_helper(beam_size=2, top_k=5, device="cpu", max_len=8)
    assert (plain.top_p, plain.min_len, plain.bad_words, plain._history_edits, plain._constraints) == (1.0, 0, None, False, False)


# ---- the row-draw dispatch ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_sample_nucleus", "beam_row_sample_prompted", "beam_row_sample_groups",
            "beam_row_sample", "beam_select_prompted", "beam_select")
V, N_IMG, BEAM, WRITE_POS = 100, 2, 2, 1
DISPATCH = list(itertools.product(("first", "later", "prompted"), (1.0, 0.8), (True, False), (False, True), (2, 3), (False, True), (3, 1),
                                  (False, True)))


@pytest.fixture
def recorded(monkeypatch):
    """The eight wrappers replaced by recorders: ``(name, arguments by parameter name)`` per call, nothing launched."""
    calls = []
    for name in WRAPPERS:
        sig = inspect.signature(getattr(hip, name))

        def recorder(*a, _name=name, _sig=sig, **k):
            bound = _sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append((_name, bound.arguments))
        monkeypatch.setattr(hip, name, recorder)
    return calls


@pytest.mark.parametrize("phase,top_p,with_gmax,exact,top_k,history,min_len,listed", DISPATCH)
def test_row_draw_dispatch_is_the_table(recorded, phase, top_p, with_gmax, exact, top_k, history, min_len, listed):
    """Dense first step, dense later step and prompted step x ``top_p`` x group maxima given x ``exact`` x ``top_k`` against
    ``n_groups(V)`` x history edits x ``min_len`` against ``write_pos`` x phrase list: the wrappers called, in order, and the arguments
    the routes differ in.  The expectation below restates the table of the design, not the code."""
    assert hip.n_groups(V) == 2 and BEAM <= 2 < 3
    prompted, first = phase == "prompted", phase == "first"
    settings = DecodeSettings.from_kw(dict(top_p=top_p, no_repeat_ngram_size=2 if history else 0, min_len=min_len,
                                           bad_words_ids=[[5]] if listed else None), 8, V)
    noise = None if prompted else (lambda kind, step, shape: torch.ones(shape))
    helper = settings.new_helper(beam_size=BEAM, top_k=top_k, device="cpu", n_img=N_IMG, max_len=8, exact=exact, noise_source=noise)
    rows = N_IMG * (1 if first else BEAM)
    logits = torch.zeros(rows, V)
    gmax = torch.zeros(rows, hip.n_groups(V)) if with_gmax else None
    if prompted:
        helper.set_prompts(torch.zeros(N_IMG, 2, dtype=torch.int64), torch.tensor([0, 1], dtype=torch.int32))
        assert helper.first_pos is not None
        helper.step_prompted(logits, write_pos=WRITE_POS, t=0, step_index=WRITE_POS, group_max=gmax)
    else:
        helper.step(logits, first=first, write_pos=WRITE_POS, t=0, step_index=WRITE_POS, group_max=gmax)

    gm = gmax if (with_gmax and not exact and top_k <= 2) else None
    fp = helper.first_pos if prompted else None
    edit = dict(tok_row_mult=BEAM if first else 1, group_max=gm, first_pos=fp)
    want = []
    if history:
        want.append(("beam_history_logits", edit))
    if listed or WRITE_POS < min_len:
        want.append(("beam_constrain_logits", edit))
    if top_p < 1:
        want.append(("beam_row_sample_nucleus", dict(exact=exact, group_max=gm, first_pos=fp)))
    elif prompted:
        want.append(("beam_row_sample_prompted", dict(exact=exact, group_max=gm, first_pos=fp)))
    elif gm is not None:
        want.append(("beam_row_sample_groups", dict(group_max=gm)))
    else:
        want.append(("beam_row_sample", dict(exact=exact)))
    want.append(("beam_select_prompted", dict(first_pos=fp)) if prompted else ("beam_select", dict(first=first)))

    assert [name for name, _ in recorded] == [name for name, _ in want]
    for (name, args), (_, expect) in zip(recorded, want):
        for key, value in expect.items():
            assert args[key] is value, (name, key)
        assert args.get("logits", logits) is logits
    draw, select = recorded[-2][1], recorded[-1][1]
    assert (draw["noise"] is None) == prompted                        # a dense row draw takes the source's noise, a prompted one Philox
    assert (select["noise"] is None) == (prompted or first)            # candidate noise only behind a later dense step


# ---- the overflow retry ------------------------------------------------------------------------------------------------------------
def test_overflow_retry(monkeypatch):
    runs = []

    def fine(exact):
        runs.append(exact)
        return "out"
    assert decode_with_overflow_retry(fine, 0) == "out" and runs == [False]
    assert decode_with_overflow_retry(fine, True) == "out" and runs == [False, True]

    state0 = torch.get_rng_state()
    states = []

    def overflows_once(exact):
        runs.append(exact)
        states.append(torch.get_rng_state())
        torch.rand(3)                                                 # the first attempt consumes the default generator
        if not exact:
            raise BeamOverflow("flat")
        return "exact out"
    monkeypatch.setattr(beam, "_overflow_warned", False)
    del runs[:]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert decode_with_overflow_retry(overflows_once, False, state0) == "exact out"
        assert decode_with_overflow_retry(overflows_once, False) == "exact out"          # (once per process)
    assert runs == [False, True, False, True]
    assert torch.equal(states[0], state0) and torch.equal(states[1], state0) and not torch.equal(states[3], states[2])
    assert [w.category for w in seen] == [RuntimeWarning] and "exact=True" in str(seen[0].message)

    def always(exact):
        runs.append(exact)
        raise BeamOverflow("still flat")
    for exact, want in ((True, [True]), (False, [False, True])):
        del runs[:]
        with pytest.raises(BeamOverflow, match="still flat"):
            decode_with_overflow_retry(always, exact)
        assert runs == want

    def other(exact):
        runs.append(exact)
        raise RuntimeError("not an overflow")
    del runs[:]
    with pytest.raises(RuntimeError, match="not an overflow"):
        decode_with_overflow_retry(other, False)
    assert runs == [False]


# ---- the session result ------------------------------------------------------------------------------------------------------------
def part(n, seed, beams, err, attention):
    g = torch.Generator().manual_seed(seed)
    ints = lambda *shape: torch.randint(0, 50, shape, generator=g)
    caps = (BeamCaptions(ints(n, 3, 6), ints(n, 3), torch.rand(n, 3, generator=g), ints(n, 3), ints(n) % 3, ints(n)) if beams
            else (ints(n, 6), ints(n)))
    return SessionResult(caps, None if err is None else torch.tensor([err], dtype=torch.int32),
                         torch.rand(n, 3, 6, 4, generator=g) if attention else None)


@pytest.mark.parametrize("beams,deferred,attention", [(False, False, False), (False, True, False), (True, False, False), (True, True, False),
                                                     (True, False, True), (True, True, True)],       # (maps: behind the beams launch only)
                         ids=("pair", "pair+err", "beams", "beams+err", "beams+maps", "beams+maps+err"))
def test_session_result_cat_and_public(beams, deferred, attention):
    a, b = part(2, 1, beams, 4 if deferred else None, attention), part(1, 2, beams, 1 if deferred else None, attention)
    both = SessionResult.cat([a, b])
    assert type(both.captions) is type(a.captions) and len(both.captions) == len(a.captions)
    for got, x, y in zip(both.captions, a.captions, b.captions):
        assert torch.equal(got, torch.cat([x, y], 0))
    if deferred:
        assert both.err.tolist() == [5] and a.err.tolist() == [4] and b.err.tolist() == [1]          # OR-ed into a copy
    else:
        assert both.err is None
    assert torch.equal(both.attention, torch.cat([a.attention, b.attention], 0)) if attention else both.attention is None
    assert SessionResult.cat([a]).captions[0] is not None and torch.equal(SessionResult.cat([a]).captions[0], a.captions[0])

    tail = ((both.err,) if deferred else ())
    for return_beams in ((False, True) if attention else (beams,)):
        out = both.public(return_beams)
        if attention and not return_beams:
            toks, lens = both.captions.best()
            drawn = both.attention[torch.arange(3), both.captions.drawn]
            want = (toks, lens, drawn) + tail
        elif beams:
            want = (both.captions,) + ((both.attention,) if attention else ()) + tail
        else:
            want = tuple(both.captions) + tail
        if len(want) == 1:
            assert out is want[0]
            continue
        assert type(out) is tuple and len(out) == len(want)
        for got, w in zip(out, want):
            assert got is w or (torch.is_tensor(w) and torch.equal(got, w))


# ---- the public callables and the record's field list ---------------------------------------------------------------------------------
KW, ONLY, VARARGS = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY", "VAR_POSITIONAL"
GEN = [("caption", KW, None), ("max_len", KW, 25), ("temperature", KW, 1.0), ("beam_size", KW, 10), ("top_k", KW, 50), ("eos_index", KW, 3)]
LENGTHS = [("caption_lengths", ONLY, None)]
GRAPHED = [("self", KW, None), ("inputs", VARARGS, None), ("seed", ONLY, None), ("caption", ONLY, None), ("caption_lengths", ONLY, None)]
ENGINE = [("seed", KW, None), ("img0", KW, 0), ("noise_source", KW, None), ("logits_hook", KW, None), ("streams", KW, 1), ("seed_tensor", KW, None),
          ("defer_check", KW, False), ("early_stop_every", KW, 0), ("exact", KW, False), ("rng", KW, None)]
MODEL_KINDS = {"CaptioningLSTM": ["images"], "CaptioningLSTMWithLabels": ["images", "labels"], "CaptioningTransformerBase": ["images"],
               "CaptioningTransformer": ["images"], "CaptioningTransformerWithLabels": ["images", "labels"]}
DECODER_KINDS = {"LSTMDecoder": ["image_emb"], "TransformerDecoder": ["start_emb", "enc_out"], "SelfAttentionTransformerDecoder": ["start_emb"]}
# every setting, in the record's order, with the value that switches it off and one that switches it on
SETTINGS = [("return_beams", False, True), ("return_attention", False, True), ("top_p", 1.0, 0.8), ("no_repeat_ngram_size", 0, 2),
            ("repetition_penalty", 1.0, 1.3), ("min_len", 0, 3), ("bad_words_ids", None, [[7]]), ("search", "sample", "beam"),
            ("return_logprobs", False, True), ("length_penalty", 0.0, 1.0), ("early_stopping", None, True), ("num_beam_groups", 1, 2),
            ("diversity_penalty", 0.0, 0.5), ("sequence_bias", None, {(7,): 1.0})]


def named(fn):
    """``fn``'s parameters but its ``**kw``: ``(name, kind, default or None)``."""
    empty = inspect.Parameter.empty
    return [(p.name, p.kind.name, None if p.default is empty else p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is not inspect.Parameter.VAR_KEYWORD]


def public_callables():
    """``{(class name, method name): the named parameters it has had since before the settings moved into ``kw``}``."""
    me = [("self", KW, None)]
    out = {}
    for kind, inputs in MODEL_KINDS.items():
        one = [(n[:-1], KW, None) for n in inputs]                     # images -> image, labels -> label
        out[kind, "generate_batch"] = me + [(n, KW, None) for n in inputs] + GEN + LENGTHS
        out[kind, "generate"] = me + one + GEN
        out[kind, "decode"] = me + [("encoded", KW, None)] + GEN + LENGTHS
        out[kind, "generate_batch_graphed"] = GRAPHED
    for kind, inputs in DECODER_KINDS.items():
        out[kind, "generate_batch"] = me + [(n, KW, None) for n in inputs] + GEN + LENGTHS
        out[kind, "generate"] = me + [(n, KW, None) for n in inputs] + GEN
    out["LSTMDecoder", "generate_batch"] = (me + [("image_emb", KW, None)] + GEN + ENGINE + LENGTHS + [
        ("return_beams", ONLY, False), ("top_p", ONLY, 1.0), ("no_repeat_ngram_size", ONLY, 0), ("repetition_penalty", ONLY, 1.0)])
    return out


def test_the_record_declares_one_field_per_setting():
    import dataclasses
    names = [f.name for f in dataclasses.fields(DecodeSettings)]
    assert names == ["return_beams", "return_attention", "top_p", "no_repeat_ngram_size", "repetition_penalty", "min_len", "bad_words_ids",
                     "num_tokens", "search", "return_logprobs", "length_penalty", "early_stopping", "num_beam_groups", "diversity_penalty",
                     "sequence_bias"]
    assert list(DecodeSettings.names()) == [n for n in names if n != "num_tokens"] == [s[0] for s in SETTINGS]
    off = DecodeSettings()
    assert [getattr(off, name) for name, _, _ in SETTINGS] == [default for _, default, _ in SETTINGS] and off.num_tokens is None
    assert off == DecodeSettings.from_kw({}, 25, 100) and off == DecodeSettings.from_kw({name: default for name, default, _ in SETTINGS}, 25, 100)


@pytest.mark.parametrize("cls,method", list(public_callables()), ids=lambda v: v)
def test_public_signature_and_every_setting_by_keyword(cls, method, monkeypatch):
    """The named parameters are what they were (name, position, kind, default); every setting is taken by keyword and reaches
    ``DecodeSettings.from_kw`` -- before anything else runs --; a keyword nobody knows is a ``TypeError``."""
    import deephumor_amd.models as M
    from deephumor_amd.models import rnn_models, transformers
    owner = getattr(M, cls, None) or getattr(rnn_models, cls, None) or getattr(transformers, cls)
    assert named(getattr(owner, method)) == public_callables()[cls, method]
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(getattr(owner, method)).parameters.values())

    obj = owner(50, n_layers=1) if "Transformer" in cls else owner(50)
    obj.eval()
    inputs = {"images": torch.zeros(1, 3, 224, 224), "labels": torch.zeros(1, 2, dtype=torch.long), "image_emb": torch.zeros(1, 256),
              "start_emb": torch.zeros(1, 512), "enc_out": torch.zeros(1, 49, 512)}
    args = [inputs[n] for n in {**MODEL_KINDS, **DECODER_KINDS}[cls]]
    if method == "decode":
        args = [tuple(inputs[n] for n in DECODER_KINDS[type(obj.decoder).__name__])]

    class Reached(Exception):
        pass
    seen = []

    def from_kw(kw, *a, **k):
        seen.append(dict(kw))
        raise Reached
    with monkeypatch.context() as mp:
        mp.setattr(DecodeSettings, "from_kw", from_kw)
        attention = not (cls == "LSTMDecoder" or (method == "decode" and "LSTM" in cls))      # (a decoder without maps does not know the keyword at all)
        for name, _, on in SETTINGS:
            if name == "return_attention" and not attention:
                continue
            with pytest.raises(Reached):
                getattr(obj, method)(*args, **{name: on})
            assert seen[-1][name] == on, name
        everything = {name: on for name, _, on in SETTINGS if attention or name != "return_attention"}
        with pytest.raises(Reached):
            getattr(obj, method)(*args, **everything)
        assert {k: seen[-1][k] for k in everything} == everything
    if cls in DECODER_KINDS or method == "decode":                     # (the models hand ``kw`` on: their decoder refuses the name)
        with pytest.raises(TypeError, match="unexpected keyword.*no_such_keyword"):
            getattr(obj, method)(*args, no_such_keyword=1)
        with pytest.raises(TypeError, match="unexpected keyword.*no_such_keyword"):
            getattr(obj, method)(*args, search="beam", sequence_bias=None, no_such_keyword=1)
    elif method != "generate_batch_graphed":                           # (that one meets its decoder inside the warm-up run, on a GPU)
        obj.encode = lambda *a: tuple(inputs[n] for n in DECODER_KINDS[type(obj.decoder).__name__])
        with pytest.raises(TypeError, match="unexpected keyword.*no_such_keyword"):
            getattr(obj, method)(*args, no_such_keyword=1)
