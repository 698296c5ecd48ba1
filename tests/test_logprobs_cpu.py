"""``return_logprobs`` on the CPU: the validation, the settings record, the result layouts, the helper's launch order, the C-ABI
additions, the refusals -- and the two restatements of ``tests/logprobs_ref.py`` against each other: the slab tables walked backwards
(``gather(record(...))``, what the kernels do) and the rows carried forwards (``track``) on random searches."""
import dataclasses
import inspect
import os
import re

import pytest
import torch

import logprobs_ref as R
from helpers import DECODE_FIELDS, synthetic_sd

from deephumor_amd import _abi, _build, hip
from deephumor_amd.models import beam
from deephumor_amd.models.beam import (BeamCaptions, BeamSearchHelper, DecodeSettings, SessionResult, check_return_logprobs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the check ---------------------------------------------------------------------------------------------------------------------
class Reforward:
    pad_index = 1


class Holder:
    decoder = Reforward()


class Plain:
    pad_index = 0


def test_check_return_logprobs():
    assert check_return_logprobs(False) is False and check_return_logprobs(True) is True
    for bad in (1, 0, None, "yes", 1.0, torch.tensor(True), [True]):
        with pytest.raises(TypeError, match="return_logprobs must be a bool"):
            check_return_logprobs(bad)
        with pytest.raises(TypeError, match="return_logprobs must be a bool"):
            check_return_logprobs(bad, Plain())
    for model in (Reforward(), Holder()):
        assert check_return_logprobs(False, model) is False                  # off, nothing is refused
        with pytest.raises(NotImplementedError, match="pad_index == 1"):
            check_return_logprobs(True, model)
    assert check_return_logprobs(True, Plain()) is True
    assert check_return_logprobs(True, object()) is True                     # every decoder kind has logits: no kind is refused


# ---- the settings record -----------------------------------------------------------------------------------------------------------
def test_settings_carry_it_last():
    names = [f.name for f in DecodeSettings.__dataclass_fields__.values()]
    assert names == DECODE_FIELDS and names[9] == "return_logprobs" and names[:9] == [
        "return_beams", "return_attention", "top_p", "no_repeat_ngram_size", "repetition_penalty", "min_len", "bad_words_ids", "num_tokens",
        "search"]
    plain = DecodeSettings.from_kw({}, 25, 1000)
    off = DecodeSettings.from_kw(dict(return_logprobs=False), 25, 1000)
    on = DecodeSettings.from_kw(dict(return_logprobs=True), 25, 1000)
    assert plain.return_logprobs is False and DecodeSettings().return_logprobs is False and on.return_logprobs is True
    assert plain == off and hash(plain) == hash(off) and on != plain and len({plain, off, on}) == 2
    assert on == DecodeSettings.from_kw(dict(return_logprobs=True), 8, 10) and hash(on) == hash(DecodeSettings.from_kw(dict(return_logprobs=True), 8))
    assert on.search == "sample" and type(on.search) is str and dataclasses.replace(on, return_logprobs=False) == plain
    with pytest.raises(AttributeError):
        on.return_logprobs = False
    kw = dict(return_logprobs=True, top_p=0.5)
    DecodeSettings.from_kw(kw, 25, 1000)
    assert kw == dict(return_logprobs=True, top_p=0.5)                       # read, not removed


def test_from_kw_checks_it_last_and_hands_the_model_on():
    for kw, exc, match in ((dict(return_logprobs=1, search="nope"), ValueError, "search"),
                           (dict(return_logprobs=1, return_beams=1), TypeError, "return_beams"),
                           (dict(return_logprobs=1, top_p=2), ValueError, "top_p"),
                           (dict(return_logprobs=1), TypeError, "return_logprobs")):
        with pytest.raises(exc, match=match):
            DecodeSettings.from_kw(kw, 25, 1000)
    with pytest.raises(NotImplementedError, match="pad_index == 1"):
        DecodeSettings.from_kw(dict(return_logprobs=True), 25, 10, Reforward())
    assert DecodeSettings.from_kw(dict(return_logprobs=False), 25, 10, Reforward()).return_logprobs is False
    assert DecodeSettings.from_kw(dict(return_logprobs=True), 25, 10, Plain()).return_logprobs is True


def test_new_helper_sets_it_behind_the_search(monkeypatch):
    assert list(inspect.signature(BeamSearchHelper.set_logprobs).parameters) == ["self", "on"]
    calls = []
    for name in ("set_constraints", "set_search", "set_logprobs"):
        real = getattr(BeamSearchHelper, name)
        monkeypatch.setattr(BeamSearchHelper, name, lambda self, *a, _n=name, _r=real, **k: (calls.append((_n, a)), _r(self, *a, **k))[1])
    h = DecodeSettings.from_kw(dict(return_logprobs=True), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert [c[0] for c in calls] == ["set_constraints", "set_search", "set_logprobs"] and calls[-1][1] == (True,)
    assert h.logprobs is True and h.lp_w.shape == h.par_w.shape == (9, 6) and h.pick_lp.shape == (6, 2)
    assert h.lp_w.dtype == h.pick_lp.dtype == torch.float32 and h.par_w.dtype == torch.int32
    assert bool((h.lp_w == 0).all()) and torch.equal(h.par_w, torch.arange(6, dtype=torch.int32).repeat(9, 1))
    off = DecodeSettings.from_kw({}, 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
    assert off.logprobs is False and off.lp_w is None and off.par_w is None and off.pick_lp is None
    bare = BeamSearchHelper(1.0, 2, 5, 1, 3, "cpu")
    assert bare.logprobs is False and bare.lp_w is None
    assert list(inspect.signature(BeamSearchHelper.__init__).parameters)[-1] == "repetition_penalty"
    with pytest.raises(TypeError, match="must be a bool"):
        bare.set_logprobs(1)


# ---- the helper's launches ---------------------------------------------------------------------------------------------------------
WRAPPERS = ("beam_history_logits", "beam_constrain_logits", "beam_row_sample_nucleus", "beam_row_sample_prompted", "beam_row_sample_groups",
            "beam_row_sample", "beam_select_prompted", "beam_select", "beam_row_best", "beam_select_best", "beam_pick_logprobs",
            "beam_record_logprobs", "beam_finalize", "beam_finalize_beams", "beam_gather_logprobs")


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


@pytest.mark.parametrize("search", ("sample", "beam"))
@pytest.mark.parametrize("phase", ("first", "later", "prompted", "no column"))
def test_two_launches_around_the_select_and_only_with_the_keyword(recorded, search, phase):
    v, n, b, max_len = 100, 2, 2, 8
    for on in (False, True):
        del recorded[:]
        s = DecodeSettings.from_kw(dict(search=search, return_logprobs=on, no_repeat_ngram_size=2), max_len, v)
        h = s.new_helper(beam_size=b, top_k=3, device="cpu", n_img=n, max_len=max_len)
        first = phase == "first"
        wp = max_len if phase == "no column" else 1
        logits = torch.zeros(n * (1 if first else b), v)
        if phase == "prompted":
            h.set_prompts(torch.zeros(n, 2, dtype=torch.int64), torch.tensor([0, 1], dtype=torch.int32))
            h.step_prompted(logits, write_pos=wp, t=0, step_index=wp)
        else:
            h.step(logits, first=first, write_pos=wp, t=0, step_index=wp)
        names = [c[0] for c in recorded]
        if search == "beam" and phase == "no column":
            assert names == []                                               # the early return stays: nothing moves, the slab stays identity
            continue
        select = "beam_select_best" if search == "beam" else "beam_select_prompted" if phase == "prompted" else "beam_select"
        draw = "beam_row_best" if search == "beam" else "beam_row_sample_prompted" if phase == "prompted" else "beam_row_sample"
        assert names == ["beam_history_logits", draw] + (["beam_pick_logprobs", select, "beam_record_logprobs"] if on else [select])
        if not on:
            continue
        pick, rec = recorded[2][1], recorded[4][1]
        fp = h.first_pos if phase == "prompted" else None
        assert pick["from_vals"] is (search == "beam") and pick["first_pos"] is fp and rec["first_pos"] is fp
        assert pick["logits"] is (None if search == "beam" else logits) and pick["rows"] == logits.shape[0]
        assert pick["rows_per_img"] == (1 if first else b) and pick["ended"] is h._ended and pick["pick_lp"] is h.pick_lp is rec["pick_lp"]
        assert pick["pick_idx"] is h.pick_idx is rec["pick_idx"] and pick["pick_val"] is h.pick_val and pick["step"] == wp
        assert rec["lp_w"] is h.lp_w and rec["par_w"] is h.par_w and rec["parent"] is h.parent and rec["tokens"] is h.tokens
        assert (rec["first"], rec["write_pos"], rec["step_index"], rec["n_img"], rec["beam"]) == (first, wp, wp, n, b)


@pytest.mark.parametrize("search", ("sample", "beam"))
def test_finalize_takes_the_beams_launch_and_gathers(recorded, search):
    for on, beams in ((False, False), (True, False), (True, True)):
        del recorded[:]
        h = DecodeSettings.from_kw(dict(search=search, return_logprobs=on), 8).new_helper(beam_size=2, top_k=5, device="cpu", n_img=3, max_len=8)
        res = h.finalize(1, 8, defer_check=True, beams=beams, pos=2)
        names = [c[0] for c in recorded]
        if not on:
            assert names == (["beam_finalize_beams"] if search == "beam" else ["beam_finalize"]) and res.logprobs is None
            continue
        assert names == ["beam_finalize_beams", "beam_gather_logprobs"]
        g = recorded[1][1]
        assert g["lp_w"] is h.lp_w and g["par_w"] is h.par_w and g["pos"] == 2 and g["first_pos"] is None
        assert g["out"] is res.logprobs and res.logprobs.shape == (3, 2, 8) and res.logprobs.dtype == torch.float32
        assert isinstance(res.captions, BeamCaptions) and res.err is h.err and res.attention is None


# ---- the session result ------------------------------------------------------------------------------------------------------------
def part(n, seed, err, attention, logprobs):
    g = torch.Generator().manual_seed(seed)
    ints = lambda *shape: torch.randint(0, 50, shape, generator=g)
    caps = BeamCaptions(ints(n, 3, 6), ints(n, 3), torch.rand(n, 3, generator=g), ints(n, 3), ints(n) % 3, ints(n))
    return SessionResult(caps, None if err is None else torch.tensor([err], dtype=torch.int32),
                         torch.rand(n, 3, 6, 4, generator=g) if attention else None, torch.rand(n, 3, 6, generator=g) if logprobs else None)


def test_session_result_has_it_last():
    assert SessionResult._fields == ("captions", "err", "attention", "logprobs") and SessionResult((1, 2)).logprobs is None


@pytest.mark.parametrize("return_beams", (False, True), ids=("pair", "beams"))
@pytest.mark.parametrize("attention", (False, True), ids=("", "maps"))
@pytest.mark.parametrize("deferred", (False, True), ids=("", "err"))
def test_public_layout_in_all_eight_combinations(return_beams, attention, deferred):
    a, b = part(2, 1, 4 if deferred else None, attention, True), part(1, 2, 1 if deferred else None, attention, True)
    both = SessionResult.cat([a, b])
    assert torch.equal(both.logprobs, torch.cat([a.logprobs, b.logprobs], 0)) and (both.attention is not None) == attention
    assert both.err is None or both.err.tolist() == [5]
    out = both.public(return_beams)
    rows = torch.arange(3)
    if return_beams:
        want = (both.captions,) + ((both.attention,) if attention else ()) + (both.logprobs,)
    else:
        want = both.captions.best() + ((both.attention[rows, both.captions.drawn],) if attention else ()) + (both.logprobs[rows, both.captions.drawn],)
    want += (both.err,) if deferred else ()
    assert type(out) is tuple and len(out) == len(want) == (1 if return_beams else 2) + attention + 1 + deferred
    for got, w in zip(out, want):
        assert got is w or (torch.is_tensor(w) and torch.equal(got, w))
    lp = out[-2] if deferred else out[-1]
    assert lp.shape == ((3, 3, 6) if return_beams else (3, 6)) and lp.dtype == torch.float32
    # record_stream reaches the new field
    seen = []

    class T:
        def record_stream(self, s):
            seen.append(s)
    SessionResult((T(), T()), None, None, T()).record_stream("s")
    assert seen == ["s"] * 3
    # without the field the layouts are what they were
    old = SessionResult.cat([part(2, 1, None, attention, False), part(1, 2, None, attention, False)])
    assert old.logprobs is None and len(old.public(True) if attention else (old.public(True),)) == 1 + attention


# ---- the two restatements against each other ---------------------------------------------------------------------------------------
def random_search(n, b, width, v, seed, prompted, no_column_last, temperature):
    """A random search in the engine's own terms: per step random parents, picks, ended flags (so images finish and freeze), per-image
    prompt phases, and optionally a last step that re-draws the beams and writes no column.  Returns (steps for ``track``, slab tables
    filled by ``record`` on the fp64 ``pick_logprobs``, final)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda hi: int(torch.randint(0, hi, (), generator=g))
    rows, n_pos = n * b, width + 1
    first_pos = [rnd(width - 1) for _ in range(n)] if prompted else None
    if prompted:
        first_pos[0], first_pos[-1] = 0, width - 2
    pos = 0 if prompted else rnd(3)
    st = dict(tokens=torch.randint(6, v, (rows, width), generator=g).int(), ended=torch.zeros(rows, dtype=torch.uint8),
              done=torch.zeros(n, dtype=torch.uint8), end_step=torch.zeros(n, dtype=torch.int32),
              parent=(torch.arange(rows, dtype=torch.int32) // b) * b if prompted else torch.zeros(rows, dtype=torch.int32))
    lp_w, par_w = R.new_tables(n_pos, rows)
    steps = []
    start = min(first_pos) if prompted else pos
    for s in range(start, width + (1 if no_column_last else 0)):
        wp = s
        dense_first = not prompted and s == pos
        mixed = prompted and s <= max(first_pos)
        lrows = n if dense_first else rows
        logits = (torch.randn(lrows, v, generator=g) * 3).float()
        logits[torch.rand(lrows, v, generator=g) < 0.1] = float("-inf")
        logits[:, 0] = 0.5                                                   # (column 0, the token an ended beam repeats, is a real column)
        pick_idx = torch.full((rows, b), -5, dtype=torch.int32)
        picks = torch.stack([torch.randperm(v, generator=g)[:b] for _ in range(lrows)]).int()
        before = {k: t.clone() for k, t in st.items()}
        if dense_first:
            pick_idx[:n] = picks
            ended_rows = before["ended"][::b]
        else:
            pick_idx[:] = picks
            ended_rows = before["ended"]
        pick_lp = torch.zeros((rows, b), dtype=torch.float64)
        pick_lp[:lrows] = R.pick_logprobs(logits, picks, ended_rows, temperature)
        for img in range(n):
            base = img * b
            first = dense_first or (mixed and s == first_pos[img])
            if (mixed and s < first_pos[img]) or int(before["done"][img]):
                continue
            for k in range(b):
                row = base + k
                par = base if first else base + rnd(b)
                was = bool(before["ended"][par]) and not first
                prow = (img if dense_first else base) if first else par
                tok = 0 if was else int(pick_idx[prow, k if first else rnd(b)])
                st["tokens"][row] = before["tokens"][par]
                if wp < width:
                    st["tokens"][row, wp] = tok
                st["ended"][row] = int(was or rnd(4) == 0)
                st["parent"][row] = par
            if not first and bool(st["ended"][base:base + b].all()):
                st["done"][img], st["end_step"][img] = 1, s
        R.record(lp_w, par_w, s, st["tokens"], st["parent"], st["done"], st["end_step"], pick_idx, pick_lp, b, dense_first, wp,
                 first_pos if mixed else None)
        steps.append(dict(logits=logits, before=before, after={k: t.clone() for k, t in st.items()}, first=dense_first, write_pos=wp, step=s,
                          first_pos=first_pos if mixed else None, temperature=temperature, beam=b))
    lengths = torch.tensor([[(first_pos[i] if prompted else pos) + rnd(width + 1 - (first_pos[i] if prompted else pos)) for _ in range(b)]
                            for i in range(n)])
    lengths[0, 0] = width
    index = torch.stack([torch.randperm(b, generator=g) for _ in range(n)])
    final = dict(beam_index=index, lengths=lengths, pos=pos, first_pos=first_pos, width=width)
    return steps, (lp_w, par_w), final, st


@pytest.mark.parametrize("prompted", (False, True), ids=("dense", "prompted"))
@pytest.mark.parametrize("no_column_last", (False, True), ids=("", "no-column"))
@pytest.mark.parametrize("n,b,width", [(1, 1, 3), (3, 2, 6), (2, 5, 9)])
def test_the_slabs_walked_back_are_the_rows_carried_forward(n, b, width, prompted, no_column_last):
    seen_done = seen_ended = 0
    for seed in range(6):
        steps, (lp_w, par_w), final, st = random_search(n, b, width, 23, 100 * seed + n + b, prompted, no_column_last, 1.0 + 0.3 * (seed % 2))
        got = R.gather(lp_w, par_w, final["beam_index"], final["lengths"], width, final["pos"], final["first_pos"])
        want = R.track(steps, final)
        assert got.shape == want.shape == (n, b, width)
        assert torch.allclose(got, want, rtol=0, atol=1e-12), seed
        cols = torch.arange(width)[None, None, :]
        p0 = torch.tensor(final["first_pos"] if prompted else [final["pos"]] * n)[:, None, None]
        assert bool((got[(cols < p0) | (cols >= final["lengths"][:, :, None])] == 0).all()) and not bool(got.isnan().any())
        seen_done += int(st["done"].sum())
        seen_ended += int(st["ended"].sum())
    assert seen_ended > 0 and (seen_done > 0 or b > 2 or n * b == 1)          # the frozen phases were walked, not only the live ones


def test_untouched_slabs_are_the_identity():
    """No step at all: every kept beam reads zeros, and the walk stays on its own row."""
    lp_w, par_w = R.new_tables(5, 6)
    out = R.gather(lp_w, par_w, torch.tensor([[1, 0], [0, 1], [1, 0]]), torch.full((3, 2), 4), 4)
    assert out.shape == (3, 2, 4) and bool((out == 0).all())


# ---- the C-ABI additions -----------------------------------------------------------------------------------------------------------
def test_three_entry_points_in_header_table_and_build():
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    for name, nargs in (("dh_beam_pick_logprobs", 15), ("dh_beam_record_logprobs", 17), ("dh_beam_gather_logprobs", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_abi.SIGNATURES[name]) and hasattr(hip, name[3:])
    assert "beam_logprobs.hip" in _build.SOURCES
    assert int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1)) == _abi.ABI_VERSION


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = hip.load()
    p = 1 << 20          # (never dereferenced: every call below fails its argument check first)
    assert lib.dh_beam_pick_logprobs(p, 8, 8, 1, 1, 65, 1.0, 0, None, p, p, p, 0, p, None) == 1          # beam > 64
    assert lib.dh_beam_pick_logprobs(p, 7, 8, 1, 1, 2, 1.0, 0, None, p, p, p, 0, p, None) == 1           # ldl < V
    assert lib.dh_beam_pick_logprobs(p, 8, 8, 2, 3, 2, 1.0, 0, None, p, p, p, 0, p, None) == 1           # rows_per_img not 1 or beam
    assert lib.dh_beam_pick_logprobs(p, 8, 8, 2, 1, 2, 0.0, 0, None, p, p, p, 0, p, None) == 1           # temperature
    assert lib.dh_beam_pick_logprobs(None, 0, 0, 2, 2, 2, 1.0, 0, None, p, None, None, 1, p, None) == 1  # from_vals without pick_val
    assert lib.dh_beam_pick_logprobs(p, 8, 8, 3, 2, 2, 1.0, 0, p, p, p, p, 0, p, None) == 1              # prompted rows not whole images
    assert lib.dh_beam_record_logprobs(p, 4, p, p, p, p, p, 1, 2, 0, None, 0, 5, 5, p, p, None) == 1     # step_index outside the table
    assert lib.dh_beam_record_logprobs(p, 4, p, p, p, p, p, 1, 2, 0, None, 0, -1, 5, p, p, None) == 1
    assert lib.dh_beam_gather_logprobs(p, p, p, p, 1, 2, 6, 5, 0, None, p, None) == 1                    # T > n_pos
    assert lib.dh_beam_gather_logprobs(p, p, p, p, 1, 2, 4, 5, -1, None, p, None) == 1                   # pos < 0


# ---- the keyword through the layers, and the refusals ------------------------------------------------------------------------------
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
    for bad in (1, None, "yes"):
        for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
            with pytest.raises(TypeError, match="return_logprobs must be a bool"):
                call(images, return_logprobs=bad)
        with pytest.raises(TypeError, match="return_logprobs must be a bool"):
            model.decode((None,) * len(dec_args), return_logprobs=bad)
        for call in (model.decoder.generate_batch, model.decoder.generate):
            with pytest.raises(TypeError, match="return_logprobs must be a bool"):
                call(*dec_args, return_logprobs=bad)
    seen = []

    class Reached(Exception):
        pass

    def from_kw(kw, *a, **k):
        s = real(kw, *a, **k)
        seen.append(s.return_logprobs)
        return s
    real = beam.DecodeSettings.from_kw
    monkeypatch.setattr(beam.DecodeSettings, "from_kw", staticmethod(from_kw))
    monkeypatch.setattr(model, "encode", lambda *a: dec_args)
    monkeypatch.setattr(type(model.decoder), "_check_mode", lambda self: (_ for _ in ()).throw(Reached()))
    for call in (model.generate_batch, model.generate):
        del seen[:]
        with pytest.raises(Reached):
            call(images, return_logprobs=True)
        assert seen and set(seen) == {True}
    for value in (True, False):
        del seen[:]
        with pytest.raises(Reached):
            model.decode(dec_args, return_logprobs=value)
        assert seen == [value]


def test_pad_index_one_is_refused_before_the_encoder(monkeypatch):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd("CaptioningTransformer")
    model = M.CaptioningTransformer(**dict(hp, pad_index=1)).eval()
    monkeypatch.setattr(model, "encode", lambda *a: (_ for _ in ()).throw(AssertionError("the encoder ran")))
    images = torch.zeros(1, 3, 224, 224)
    for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
        with pytest.raises(NotImplementedError, match="return_logprobs with pad_index == 1"):
            call(images, return_logprobs=True)
    with pytest.raises(NotImplementedError, match="return_logprobs with pad_index == 1"):
        model.decoder.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), return_logprobs=True)


def test_pipeline_and_sharded_callers_refuse():
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline

    class Model:
        _hp = {"num_tokens": 50}

        def parameters(self):
            return iter([torch.zeros(1)])
    with pytest.raises(NotImplementedError, match="^return_logprobs: CaptionPipeline"):
        CaptionPipeline(Model(), overlap=False, return_logprobs=True)
    with pytest.raises(TypeError, match="return_logprobs must be a bool"):
        CaptionPipeline(Model(), overlap=False, return_logprobs=1)
    toks, lens, lp = torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, dtype=torch.int64), torch.zeros(2, 4)
    with pytest.raises(NotImplementedError, match="return_logprobs"):
        dist.generate_sharded(lambda lo, hi: (toks, lens, lp), 2)
    caps = BeamCaptions(toks[:, None], lens[:, None], torch.zeros(2, 1), lens[:, None], lens, lens)
    with pytest.raises(NotImplementedError, match="return_logprobs"):
        dist.generate_sharded(lambda lo, hi: (caps, lp[:, None]), 2)


def test_single_image_outputs():
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import _IncrementalDecoder
    toks, lens, lp = torch.arange(12).view(2, 6), torch.tensor([4, 6]), torch.rand(2, 6)
    for one in (lambda r: LSTMDecoder.single_output(r, None, 6, 3), _IncrementalDecoder._one):
        cap, got = one((toks, lens, lp))
        assert cap.tolist() == [0, 1, 2, 3] and torch.equal(got, lp[0, :4])
        assert one((toks, lens)).tolist() == [0, 1, 2, 3]
        caps = BeamCaptions(toks[:1, None], lens[:1, None], torch.zeros(1, 1), lens[:1, None], lens[:1], lens[:1])
        res = one((caps, lp[:1, None]))
        assert res[0] is caps and res[1].shape == (1, 1, 6)
    att = torch.rand(2, 6, 49)
    cap, a, got = _IncrementalDecoder._one((toks, lens, att, lp))
    assert torch.equal(a, att[0, :4]) and torch.equal(got, lp[0, :4])


def test_beam_logprob_scores():
    from deephumor_amd.experiments import beam_logprob_scores
    lens = torch.tensor([[5, 3], [6, 2]])
    lp = -torch.rand(2, 2, 6)
    lp[torch.arange(6)[None, None, :] >= lens[:, :, None]] = 0.0
    lp[:, :, :2] = 0.0                                                       # a prefix of two tokens
    caps = BeamCaptions(torch.zeros(2, 2, 6, dtype=torch.int64), lens, torch.zeros(2, 2), lens, lens[:, 0], lens[:, 0])
    total = beam_logprob_scores(caps, lp)
    assert total.shape == (2, 2) and torch.allclose(total, lp.sum(-1))
    mean = beam_logprob_scores(caps, lp, length_normalize=True, first_pos=2)
    assert torch.allclose(mean, lp.sum(-1) / torch.tensor([[3.0, 1.0], [4.0, 1.0]]))
    per_image = beam_logprob_scores(caps, lp, True, torch.tensor([2, 0]))
    assert torch.allclose(per_image[1], lp[1].sum(-1) / torch.tensor([6.0, 2.0])) and torch.equal(per_image[0], mean[0])
    poisoned = lp.clone()
    poisoned[0, 1, 4] = 7.0                                                  # behind the beam's own length: not looked at
    assert torch.equal(beam_logprob_scores(caps, poisoned), total)
    from deephumor_amd.experiments import rank_beams
    assert "beam_logprob_scores" in rank_beams.__doc__ and "rank_beams" in beam_logprob_scores.__doc__
