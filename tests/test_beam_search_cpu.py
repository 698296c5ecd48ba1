"""``search="beam"`` on the CPU: ``beam.check_search``, the ``DecodeSettings`` field, the helper's dispatch, the ABI of the two new entry
points and their argument contracts, the torch-CPU restatement (``tests/beam_search_ref.py``) against brute force, and the keyword
through every public layer."""
import ctypes
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from beam_search_ref import State, beam_search, finalize_best, rank_desc, row_best, select_best  # noqa: E402
from helpers import DECODE_FIELDS, KINDS, synthetic_sd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_check_search():
    from deephumor_amd.models.beam import check_search
    assert check_search("sample") == "sample" and check_search("beam") == "beam" and check_search("beam", 1.0) == "beam"
    assert check_search("sample", 0.5) == "sample"
    for bad in (None, 1, 0, True, 1.0, b"beam", ["beam"], ("beam",), np.str_, torch.tensor(1)):
        with pytest.raises(TypeError, match="search"):
            check_search(bad)
    for bad in ("", "Beam", "BEAM", "greedy", "sampling", "beam "):
        with pytest.raises(ValueError) as e:
            check_search(bad)
        assert '"sample"' in str(e.value) and '"beam"' in str(e.value)
    with pytest.raises(ValueError, match="top_p"):
        check_search("beam", 0.8)


def test_decode_settings_field_key_and_check_order():
    from deephumor_amd.models.beam import DecodeSettings
    fields = [f.name for f in __import__("dataclasses").fields(DecodeSettings)]
    assert fields == DECODE_FIELDS and fields.index("search") == 8
    assert DecodeSettings().search == "sample" and DecodeSettings(False, False, 1.0, 0, 1.0, 0, None, 10).search == "sample"
    plain, none = DecodeSettings.from_kw({}, 25, 100), DecodeSettings.from_kw(dict(search="sample"), 25, 100)
    best = DecodeSettings.from_kw(dict(search="beam"), 25, 100)
    assert plain == none and hash(plain) == hash(none) and plain.search == "sample"
    assert best.search == "beam" and best != plain and len({plain, none, best}) == 2 and type(best.search) is str
    assert best == DecodeSettings.from_kw(dict(search="beam", top_p=1), 8, 100)
    kw = dict(search="beam", return_beams=True)
    before = dict(kw)
    DecodeSettings.from_kw(kw, 25, 100)
    assert kw == before                                               # read, not removed
    # checked LAST: every other bad value raises first
    for other, exc, match in ((dict(return_beams=1), TypeError, "return_beams"), (dict(top_p=2), ValueError, "top_p"),
                              (dict(no_repeat_ngram_size=-1), ValueError, "no_repeat_ngram_size"), (dict(min_len=-1), ValueError, "min_len"),
                              (dict(bad_words_ids=[[]]), ValueError, "bad_words_ids")):
        with pytest.raises(exc, match=match):
            DecodeSettings.from_kw(dict(other, search="nope"), 25, 100)
    with pytest.raises(ValueError, match="search"):
        DecodeSettings.from_kw(dict(search="nope"), 25, 100)
    with pytest.raises(TypeError, match="search"):
        DecodeSettings.from_kw(dict(search=None), 25, 100)
    with pytest.raises(ValueError, match="top_p"):
        DecodeSettings.from_kw(dict(search="beam", top_p=0.9), 25, 100)
    assert DecodeSettings.from_kw(dict(search="sample", top_p=0.9), 25, 100).top_p == 0.9


def test_set_search_and_new_helper():
    from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings
    assert list(inspect.signature(BeamSearchHelper.set_search).parameters) == ["self", "search"]
    assert "search" not in inspect.signature(BeamSearchHelper.__init__).parameters
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
    assert h.search == "sample" and h.set_search("beam") is h and h.search == "beam" and h.set_search("sample").search == "sample"
    with pytest.raises(ValueError):
        h.set_search("best")
    with pytest.raises(TypeError):
        h.set_search(1)
    with pytest.raises(ValueError, match="top_p"):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", top_p=0.5).set_search("beam")
    with pytest.raises(AssertionError):                               # top_k keeps its assertion
        DecodeSettings.from_kw(dict(search="beam"), 8).new_helper(beam_size=6, top_k=5, device="cpu", max_len=8)
    got = DecodeSettings.from_kw(dict(search="beam", min_len=2), 8).new_helper(beam_size=2, top_k=5, device="cpu", max_len=8)
    assert got.search == "beam" and got.min_len == 2
    assert DecodeSettings.from_kw({}, 8).new_helper(beam_size=2, top_k=5, device="cpu", max_len=8).search == "sample"
    logits = torch.zeros(3, 8)
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu").set_search("beam")
    with pytest.raises(NotImplementedError, match="search"):          # the reference-style method surface draws
        h.sample_k_indices(logits)
    with pytest.raises(NotImplementedError, match="search"):
        h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))


# ---- the helper's launches ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_sample_nucleus", "beam_row_sample_prompted", "beam_row_sample_groups",
            "beam_row_sample", "beam_select_prompted", "beam_select", "beam_row_best", "beam_select_best", "beam_finalize",
            "beam_finalize_beams", "beam_gather_attention")
V, N_IMG, BEAM = 100, 2, 2


@pytest.fixture
def recorded(monkeypatch):
    from deephumor_amd import hip
    calls = []
    for name in WRAPPERS:
        sig = inspect.signature(getattr(hip, name))

        def recorder(*a, _name=name, _sig=sig, **k):
            bound = _sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append((_name, bound.arguments))
        monkeypatch.setattr(hip, name, recorder)
    return calls


@pytest.mark.parametrize("phase,with_gmax,exact,top_k,history,min_len",
                         list(itertools.product(("first", "later", "prompted"), (True, False), (False, True), (2, 3), (False, True), (3, 0))))
def test_beam_mode_launches(recorded, phase, with_gmax, exact, top_k, history, min_len):
    """The edits and the bans in front, then ``beam_row_best`` and ``beam_select_best`` -- no sampler, no sampled select, no noise asked
    for; the group maxima go to all three whenever they are given (nothing is filtered by ``top_k``, ``exact`` has nothing to do)."""
    from deephumor_amd import hip
    from deephumor_amd.models.beam import DecodeSettings
    prompted, first = phase == "prompted", phase == "first"
    settings = DecodeSettings.from_kw(dict(search="beam", no_repeat_ngram_size=2 if history else 0, min_len=min_len), 8, V)
    asked = []
    helper = settings.new_helper(beam_size=BEAM, top_k=top_k, device="cpu", n_img=N_IMG, max_len=8, exact=exact, temperature=1.3,
                                 noise_source=lambda *a: asked.append(a))
    rows = N_IMG * (1 if first else BEAM)
    logits = torch.zeros(rows, V)
    gmax = torch.zeros(rows, hip.n_groups(V)) if with_gmax else None
    if prompted:
        helper.set_prompts(torch.zeros(N_IMG, 2, dtype=torch.int64), torch.tensor([0, 1], dtype=torch.int32))
        helper.step_prompted(logits, write_pos=1, t=0, step_index=1, group_max=gmax)
    else:
        helper.step(logits, first=first, write_pos=1, t=0, step_index=1, first_sets_ended=False, group_max=gmax)
    fp = helper.first_pos if prompted else None
    want = (["beam_history_logits"] if history else []) + (["beam_constrain_logits"] if 1 < min_len else []) + ["beam_row_best", "beam_select_best"]
    assert [n for n, _ in recorded] == want and asked == []
    for name, args in recorded:
        if name != "beam_select_best":
            assert args["group_max"] is gmax and args["logits"] is logits
        assert args["first_pos"] is fp
    row, sel = recorded[-2][1], recorded[-1][1]
    assert (row["rows"], row["rows_per_img"], row["beam"], row["temperature"], row["unk_index"], row["step"]) == (rows, 1 if first else BEAM, BEAM, 1.3, 1, 1)
    assert row["pick_idx"] is helper.pick_idx and row["pick_val"] is helper.pick_val and row["err"] is helper.err
    assert sel["first"] == first and sel["first_sets_ended"] is True and (sel["write_pos"], sel["t"], sel["step_index"]) == (1, 0, 1)
    assert sel["hparent"] is helper.hparent and sel["tokens"] is helper.tokens and sel["eos_index"] == 3


def test_default_launches_are_unchanged_and_finalize_takes_slot_zero(recorded):
    from deephumor_amd.models.beam import BeamCaptions, DecodeSettings
    for search in ({}, dict(search="sample")):
        del recorded[:]
        h = DecodeSettings.from_kw(search, 8, V).new_helper(beam_size=BEAM, top_k=3, device="cpu", n_img=N_IMG, max_len=8)
        h.step(torch.zeros(N_IMG, V), first=True, write_pos=0, t=0, step_index=0)
        h.finalize(1, 8, defer_check=True)
        assert [n for n, _ in recorded] == ["beam_row_sample", "beam_select", "beam_finalize"]
    asked = []
    for beams in (False, True):
        del recorded[:]
        h = DecodeSettings.from_kw(dict(search="beam"), 8, V).new_helper(beam_size=BEAM, top_k=3, device="cpu", n_img=N_IMG, max_len=8,
                                                                          noise_source=lambda *a: asked.append(a))
        res = h.finalize(1, 8, defer_check=True, beams=beams, first_beam=True)
        assert [n for n, _ in recorded] == ["beam_finalize_beams"] and recorded[0][1]["noise"] is None and asked == []
        caps = res.captions
        if beams:
            assert isinstance(caps, BeamCaptions) and caps.drawn.tolist() == [0, 0] and caps.tokens.shape == (N_IMG, BEAM, 8)
        else:
            assert isinstance(caps, tuple) and caps[0].shape == (N_IMG, 8) and caps[1].shape == (N_IMG,)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
ROW_ARGS = ["logits", "ldl", "V", "group_max", "gm_ld", "n_groups", "group_cols", "rows", "rows_per_img", "beam", "temperature", "unk_index",
            "step", "first_pos", "pick_idx", "pick_val", "err", "stream"]
SEL_ARGS = ["pick_idx", "pick_val", "tokens", "tok_ld", "vals", "ended", "src", "src_ld", "parent", "hparent", "done", "end_step", "n_img",
            "beam", "first", "first_pos", "first_sets_ended", "write_pos", "t", "step_index", "eos_index", "stream"]


@pytest.mark.parametrize("name,names", [("dh_beam_row_best", ROW_ARGS), ("dh_beam_select_best", SEL_ARGS)])
def test_abi_header_table_and_library_agree(name, names):
    from deephumor_amd import _abi, _build, hip
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
    assert int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1)) == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, name)
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35
    # additive: no existing prototype moved
    assert [len(_abi.SIGNATURES[n]) for n in ("dh_beam_row_sample", "dh_beam_row_sample_groups", "dh_beam_row_sample_nucleus", "dh_beam_select",
                                              "dh_beam_select_prompted", "dh_beam_finalize_beams")] == [18, 22, 25, 26, 26, 26]
    assert "beam_best.hip" in _build.SOURCES and hasattr(hip, name[3:]) and lib.dh_option_count() == 15


def call_with(fn, names, good, **over):
    a = list(good)
    for k, val in over.items():
        a[names.index(k)] = val
    return fn(*a)


def test_row_best_argument_contract():
    """Checked before any HIP call (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    from deephumor_amd import hip
    fn = hip.load().dh_beam_row_best
    #       logits ldl  V   gmax gm ng gc rows rpi beam T   unk step first_pos pick_idx pick_val err stream
    good = [64, 128, 100, None, 0, 0, 0, 6, 3, 3, 1.0, 1, 0, None, 64, 64, 64, None]
    for over in (dict(logits=None), dict(pick_idx=None), dict(pick_val=None), dict(err=None), dict(rows=0), dict(rows=-3), dict(rows_per_img=0),
                 dict(V=0), dict(ldl=99), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1), dict(temperature=0.0), dict(temperature=-1.0),
                 dict(temperature=float("nan")), dict(temperature=float("inf")),
                 dict(group_max=64, gm_ld=2, n_groups=1, group_cols=64),          # 64 columns of groups for V = 100
                 dict(group_max=64, gm_ld=1, n_groups=2, group_cols=64),          # gm_ld < n_groups
                 dict(group_max=64, gm_ld=2, n_groups=2, group_cols=65), dict(group_max=64, gm_ld=2, n_groups=2, group_cols=0),
                 dict(group_max=64, gm_ld=2000, n_groups=1025, group_cols=64), dict(group_max=64, gm_ld=0, n_groups=0, group_cols=64),
                 dict(first_pos=64, rows_per_img=1), dict(first_pos=64, rows=7), dict(first_pos=64, rows_per_img=2, rows=6)):
        assert call_with(fn, ROW_ARGS, good, **over) == 1, over


def test_select_best_argument_contract():
    from deephumor_amd import hip
    fn = hip.load().dh_beam_select_best
    #       pi  pv  tok ld vals end src sld par hpar done estep n b first first_pos fse wp t step eos stream
    good = [64, 64, 64, 8, 64, 64, None, 0, 64, 64, 64, 64, 2, 3, 0, None, 1, 1, 0, 1, 3, None]
    for over in (dict(pick_idx=None), dict(pick_val=None), dict(tokens=None), dict(vals=None), dict(ended=None), dict(parent=None),
                 dict(hparent=None), dict(done=None), dict(end_step=None), dict(n_img=0), dict(beam=0), dict(beam=hip.MAX_BEAMS + 1),
                 dict(tok_ld=0), dict(t=-1), dict(src=64, src_ld=0, t=0), dict(src=64, src_ld=5, t=5),
                 dict(beam=64, tok_ld=300), dict(first_pos=64, beam=64, tok_ld=300)):      # more staging than the LDS holds
        assert call_with(fn, SEL_ARGS, good, **over) == 1, over


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def table_model(v, seed, scale=2.0):
    """A 'model' whose logits depend on the whole prefix: a table row per prefix, drawn on demand from a generator keyed by it."""
    cache = {}

    def row(prefix):
        if prefix not in cache:
            g = torch.Generator().manual_seed(hash((seed,) + prefix) % (1 << 31))
            cache[prefix] = torch.randn(v, generator=g) * scale
        return cache[prefix]

    def logits_fn(tokens, pos, rows_per_img):
        return torch.stack([row(tuple(int(t) for t in tokens[r, :pos])) for r in range(tokens.shape[0])])
    return row, logits_fn


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("temperature", (1.0, 1.3))
def test_restatement_finds_the_exhaustive_best_sequences(seed, temperature):
    """``V = 5``, 3 steps, ``B = 25``: the beam is never narrower than the set of live sequences (``<unk>`` is never a token, so
    ``4 ** 2 = 16`` before the last step), so nothing is pruned early and the result must be the 25 best of all ``4 ** 3`` sequences by
    their summed fp64 log-probability.  ``eos`` is outside the vocabulary: nothing ends."""
    v, steps, b, unk = 5, 3, 25, 1
    row, logits_fn = table_model(v, seed)
    out, err = beam_search(logits_fn, 1, b, steps, temperature, unk, eos=99)
    assert err == 4                                                   # TOO_FEW (4 eligible tokens for 25 beams): dead beams, no error
    every = []
    for seq in itertools.product([t for t in range(v) if t != unk], repeat=steps):
        lp = 0.0
        for i in range(steps):
            lp += float(torch.log_softmax(row(seq[:i]).double() / temperature, 0)[seq[i]])
        every.append((lp, seq))
    every.sort(key=lambda e: -e[0])
    got = [tuple(out["tokens"][0, j].tolist()) for j in range(b)]
    assert got == [seq for _, seq in every[:b]]
    assert np.allclose(out["scores"][0].numpy(), [lp for lp, _ in every[:b]], rtol=0, atol=1e-5)
    assert out["drawn"].tolist() == [0] and out["row_lengths"].tolist() == [steps] and out["lengths"].tolist() == [[steps] * b]
    assert bool((out["scores"][0, :-1] >= out["scores"][0, 1:]).all())


@pytest.mark.parametrize("seed", range(3))
def test_restatement_at_beam_one_is_the_greedy_arg_max(seed):
    v, steps, unk, eos = 9, 6, 1, 3
    row, logits_fn = table_model(v, 100 + seed)
    out, err = beam_search(logits_fn, 2, 1, steps, 1.0, unk, eos)
    assert err == 0
    for img in range(2):
        prefix, lp, ended = (), 0.0, False
        want = []
        for pos in range(steps):
            if ended:
                break
            x = row(prefix).clone()
            lsm = torch.log_softmax(x.double(), 0)
            x[unk] = float("-inf")
            tok = int(torch.argmax(x))
            lp += float(lsm[tok])
            want.append(tok)
            prefix += (tok,)
            ended = tok == eos
        n = int(out["lengths"][img, 0])
        assert out["tokens"][img, 0, :n].tolist() == want and abs(float(out["scores"][img, 0]) - lp) <= 1e-5


def test_row_best_rules():
    ninf, nan, inf = float("-inf"), float("nan"), float("inf")
    x = torch.tensor([[0.5, 9.0, 0.5, 0.25, -0.0, 0.0, ninf, 0.5],          # unk (1) is the arg-max; three equal 0.5; -0.0 == +0.0
                      [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],             # constant: the lowest eligible indices
                      [ninf, 3.0, ninf, 2.0, ninf, ninf, ninf, ninf],       # one eligible: TOO_FEW
                      [ninf, 3.0, ninf, ninf, ninf, ninf, ninf, ninf],      # only unk: ALL_FILTERED
                      [0.0, 1.0, nan, 0.0, 0.0, 0.0, 0.0, 0.0],
                      [0.0, 1.0, inf, 0.0, 0.0, 0.0, 0.0, 0.0]])
    picks, vals, err = row_best(x, 2.0, 4, 1)
    assert picks[0].tolist() == [0, 2, 7, 3] and picks[1].tolist() == [0, 2, 3, 4] and err[:2] == [0, 0]
    lse0 = math.log(sum(math.exp(float(t) / 2.0) for t in x[0].tolist()))
    assert abs(float(vals[0, 0]) - (0.25 - lse0)) < 1e-12 and abs(float(vals[1, 0]) + math.log(8)) < 1e-12      # unk's mass counts
    assert row_best(x[:1], 1.0, 6, 1)[0][0].tolist() == [0, 2, 7, 3, 4, 5]                                          # -0.0 before +0.0: index
    assert picks[2].tolist() == [3, 0, 0, 0] and vals[2, 1:].tolist() == [ninf] * 3 and err[2] == 4
    assert abs(float(vals[2, 0]) - (1.0 - math.log(math.exp(1.5) + math.exp(1.0)))) < 1e-12
    assert err[3:] == [1, 8, 8] and picks[3:].tolist() == [[0] * 4] * 3 and vals[3:].tolist() == [[0.0] * 4] * 3
    assert rank_desc(torch.tensor([1.0, nan, 2.0, ninf, 2.0])) == [2, 4, 0, 1, 3]


def test_select_best_rules():
    """Two images, ``B = 3``: an ended beam brings one candidate (token 0, its score), equal scores go to the lower candidate index,
    ``-inf`` ranks last, ``hparent`` is the real parent, the last column's step writes nothing, a finished image is frozen."""
    b, eos = 3, 3
    st = State(2, b, 4, src_len=5)
    st.tokens[:, 0] = torch.tensor([10, 11, 12, 20, 21, 22], dtype=torch.int32)
    st.vals = torch.tensor([-1.0, -0.5, -2.0, -1.0, -1.0, float("-inf")])
    st.ended[1] = 1
    pick_idx = torch.tensor([[5, 3, 6], [9, 9, 9], [7, 8, 9], [4, 5, 6], [7, 8, 9], [1, 1, 1]])
    pick_val = torch.tensor([[-0.25, -0.5, -3.0], [-9.0, -9.0, -9.0], [-0.1, -4.0, -5.0], [-1.0, -2.0, -3.0], [-1.0, -2.0, -9.0],
                             [-0.125, -0.125, -0.125]])
    select_best(st, pick_idx, pick_val, False, 1, 1, 1, eos)
    # image 0: candidates -1.25 (5), -1.5 (eos), -4 | -0.5 (ended) | -2.1, -6, -7 -> the ended beam, 5, eos
    assert st.tokens[:3, :2].tolist() == [[11, 0], [10, 5], [10, 3]] and st.vals[:3].tolist() == [-0.5, -1.25, -1.5]
    assert st.ended[:3].tolist() == [1, 0, 1] and st.parent[:3].tolist() == [1, 0, 0] and st.hparent[:3].tolist() == [1, 0, 0]
    assert st.src[:3, 1].tolist() == [1, 0, 0] and st.done.tolist() == [0, 0]
    # image 1: -2 (4), -3, -4 | -2 (7), -3, -10 | -inf x 3 -> 4 before 7 (equal, lower index), then the first -3
    assert st.tokens[3:, :2].tolist() == [[20, 4], [21, 7], [20, 5]] and st.vals[3:].tolist() == [-2.0, -2.0, -3.0]
    assert st.hparent[3:].tolist() == [3, 4, 3]
    frozen = {k: None if t is None else t.clone() for k, t in st.fields().items()}
    st.ended[:3] = 1
    select_best(st, pick_idx, pick_val, False, 4, 2, 2, eos)          # write_pos == tok_ld: no token column is written
    assert st.done.tolist() == [1, 0] and st.end_step.tolist() == [2, 0] and torch.equal(st.tokens[:3], frozen["tokens"][:3])
    # image 1: -3 (beam 0), -4, -5 | -3 (beam 1), -4, -11 | -3.125 x 3 (beam 2)
    assert st.tokens[3:].tolist() == [[20, 4, 0, 0], [21, 7, 0, 0], [20, 5, 0, 0]] and st.vals[3:].tolist() == [-3.0, -3.0, -3.125]
    again = {k: None if t is None else t.clone() for k, t in st.fields().items()}
    select_best(st, pick_idx, pick_val, False, 3, 3, 3, eos)          # image 0 is done: frozen
    for k in ("tokens", "vals", "ended", "parent", "hparent", "src"):
        assert torch.equal(st.fields()[k][:3], again[k][:3]), k
    out = finalize_best(st, 1, 4, eos=eos, pos=1)
    assert out["row_lengths"].tolist() == [3, 4] and out["beam_index"][0].tolist() == [0, 1, 2] and out["drawn"].tolist() == [0, 0]
    assert out["tokens"][0, 2].tolist() == [10, 3, 0, 0] and out["lengths"][0].tolist() == [3, 3, 2]


def test_select_best_first_step_and_prompted_phases():
    b, eos = 2, 3
    st = State(3, b, 5, src_len=6)
    st.tokens[0:2, :2] = torch.tensor([[8, 9], [8, 9]], dtype=torch.int32)          # image 0: a prompt of 2, still forced at step 1
    st.tokens[2:4, :1] = 7                                                            # image 1: a prompt of 1: its first step
    st.vals[4:6] = torch.tensor([-1.0, -2.0])                                         # image 2: no prompt, a normal step
    pick_idx = torch.tensor([[1, 1], [1, 1], [3, 4], [6, 6], [5, 6], [7, 8]])
    pick_val = torch.tensor([[-9.0, -9.0], [-9.0, -9.0], [-0.5, -1.5], [-7.0, -7.0], [-0.25, -3.0], [-0.5, -0.75]])
    select_best(st, pick_idx, pick_val, False, 1, 1, 1, eos, first_pos=[2, 1, 0])
    assert st.tokens[0:2].tolist() == [[8, 9, 0, 0, 0]] * 2 and st.vals[:2].tolist() == [0.0, 0.0] and st.src[:2, 1].tolist() == [0, 0]
    assert st.tokens[2:4, :2].tolist() == [[7, 3], [7, 4]] and st.vals[2:4].tolist() == [-0.5, -1.5] and st.ended[2:4].tolist() == [1, 0]
    assert st.parent[2:4].tolist() == [2, 2] and st.hparent[2:4].tolist() == [2, 2] and st.done.tolist() == [0, 0, 0]
    assert st.tokens[4:6, 1].tolist() == [5, 7] and st.vals[4:6].tolist() == [-1.25, -2.5] and st.hparent[4:6].tolist() == [4, 5]
    dense = State(2, b, 5)
    select_best(dense, torch.tensor([[3, 4], [5, 6]]), torch.tensor([[-0.5, -1.5], [-0.1, -2.0]]), True, 0, 0, 0, eos)
    assert dense.tokens[:, 0].tolist() == [3, 4, 5, 6] and dense.ended.tolist() == [1, 0, 0, 0] and dense.parent.tolist() == [0, 0, 2, 2]


# ---- the keyword through the layers ------------------------------------------------------------------------------------------------
def test_keyword_reaches_every_public_layer():
    import deephumor_amd.models as M
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder, _IncrementalDecoder
    # (the signatures of every public callable, and the keyword on its way to DecodeSettings.from_kw: test_decode_settings_cpu)
    fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
    fns += [TransformerDecoder.generate_batch, TransformerDecoder.generate, SelfAttentionTransformerDecoder.generate_batch,
            SelfAttentionTransformerDecoder.generate, LSTMDecoder.generate]
    for fn in fns:                                                    # everywhere else it rides in **kw
        ps = inspect.signature(fn).parameters
        assert "search" not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    assert [p.name for p in inspect.signature(LSTMDecoder.generate_batch).parameters.values() if p.kind is not p.VAR_KEYWORD][-1] == "repetition_penalty"
    with pytest.raises(ValueError, match="search"):                   # ... and takes the keyword by name
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="nope")
    with pytest.raises(TypeError, match="unexpected keyword"):
        LSTMDecoder(50).generate_batch(torch.zeros(1, 256), search="beam", no_such_keyword=1)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_values_fail_before_the_encoder_and_good_ones_reach_the_decoder(kind, monkeypatch):
    import deephumor_amd.models as M
    from deephumor_amd.models import beam
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    monkeypatch.setattr(model, "encode", boom)
    images = torch.zeros(1, 3, 224, 224)
    dec_args = (torch.zeros(1, 256),) if kind == "CaptioningLSTM" else (torch.zeros(1, 512), torch.zeros(1, 49, 512))
    for bad, exc in (("greedy", ValueError), (None, TypeError), (1, TypeError)):
        for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
            with pytest.raises(exc, match="search"):
                call(images, search=bad)
        with pytest.raises(exc, match="search"):
            model.decode((None,) * len(dec_args), search=bad)
        with pytest.raises(exc, match="search"):
            model.decoder.generate_batch(*dec_args, search=bad)
        with pytest.raises(exc, match="search"):
            model.decoder.generate(*dec_args, search=bad)
    for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
        with pytest.raises(ValueError, match="top_p"):
            call(images, search="beam", top_p=0.5)
    # a good value travels: the record the decoder builds carries it (the stub stands where the first device work would start)
    seen = []

    class Reached(Exception):
        pass

    def from_kw(kw, *a, **k):
        s = real(kw, *a, **k)
        seen.append(s.search)
        return s
    real = beam.DecodeSettings.from_kw
    monkeypatch.setattr(beam.DecodeSettings, "from_kw", staticmethod(from_kw))
    monkeypatch.setattr(model, "encode", lambda *a: dec_args)
    monkeypatch.setattr(type(model.decoder), "_check_mode", lambda self: (_ for _ in ()).throw(Reached()))
    for call in (model.generate_batch, model.generate):
        del seen[:]
        with pytest.raises(Reached):
            call(images, search="beam", rng="torch", noise_source=lambda *a: None)
        assert seen and set(seen) == {"beam"}
    del seen[:]
    with pytest.raises(Reached):
        model.decode(dec_args, search="beam")
    assert seen == ["beam"]


def test_pipeline_and_sharded_callers_carry_the_keyword(monkeypatch):
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline
    src = inspect.getsource(CaptionPipeline.__init__)
    assert "DecodeSettings.from_kw(gen_kw" in src and "settings.search" in src           # validated with the rest, before a batch is staged
    assert "search" in dist.generate_sharded.__doc__

    class Model:
        _hp = {"num_tokens": 50}

        def parameters(self):
            return iter([torch.zeros(1)])
    for bad, exc in (("greedy", ValueError), (3, TypeError)):
        with pytest.raises(exc, match="search"):
            CaptionPipeline(Model(), overlap=False, search=bad)
    with pytest.raises(ValueError, match="top_p"):
        CaptionPipeline(Model(), overlap=False, search="beam", top_p=0.5)
    seen = {}
    got = dist.generate_sharded(lambda lo, hi: seen.update(lo=lo, hi=hi, search="beam") or (torch.zeros(hi - lo, 4, dtype=torch.int64),
                                                                                         torch.ones(hi - lo, dtype=torch.int64)), 3)
    assert seen == dict(lo=0, hi=3, search="beam") and got[0].shape == (3, 4)
