"""``experiments.text_occlusion`` without a GPU: its refusals (all of which fire before the encoder runs), the variant builder against
the restated one, the ``TextOcclusionScores`` record, ``occlusion_to_texts``, the restatement of ``text_occlusion_ref`` against golden
G29 and its structure, and the pins this feature must not move: 129 prototypes, ABI 35, 124 signatures, 15 options.

Bounds.  The restatement runs ``oracle.ref_path`` in fp32 and G29 is the real reference in fp32: both are fp32 statements of the same
model.  The gate is 1.25 x the difference measured on the CPU that recorded G29 -- ``MEASURED`` below, the worst over 1, 2, 3, 4 and 8
threads of (base, drop, token_drop) per (kind, level, fill); the test prints what it sees."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import explain_ref as E
import text_occlusion_ref as T
from helpers import synth_images
from deephumor_amd import experiments
from deephumor_amd.experiments import TextOcclusionScores, occlusion_to_texts, text_occlusion

product = importlib.import_module("deephumor_amd.experiments.text_occlusion")      # (the package attribute of that name is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_L, _LL, _B, _T, _TL = E.KINDS
MEASURED = {                               # (kind, level, fill) -> (base, drop, token_drop); a base near -78 has an fp32 ulp of 7.6e-6
    (_L, "history", "pad"): (3.920e-06, 7.964e-06, 6.253e-06), (_L, "history", "unk"): (3.920e-06, 1.296e-05, 7.427e-06),
    (_LL, "history", "pad"): (3.155e-06, 6.994e-06, 4.308e-06), (_LL, "history", "unk"): (3.155e-06, 5.533e-06, 3.457e-06),
    (_LL, "label", "unk"): (4.564e-06, 5.509e-06, 3.614e-06),
    (_B, "history", "pad"): (5.822e-06, 3.276e-06, 2.683e-06), (_B, "history", "unk"): (5.822e-06, 4.434e-06, 3.230e-06),
    (_T, "history", "pad"): (7.850e-06, 6.347e-06, 3.880e-06), (_T, "history", "unk"): (7.850e-06, 6.089e-06, 4.653e-06),
    (_TL, "history", "pad"): (4.261e-06, 1.143e-05, 2.961e-06), (_TL, "history", "unk"): (4.261e-06, 5.499e-06, 3.138e-06),
    (_TL, "label", "unk"): (4.261e-06, 9.003e-06, 3.629e-06),
}


def build(kind, **extra):
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_state_dict
    model = getattr(M, kind)(**dict(E.HP[kind], **extra)).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=E.SEED))
    return model


def lab(kind, labels):
    return labels if "WithLabels" in kind else None


def test_it_is_exported():
    for name in ("text_occlusion", "TextOcclusionScores", "occlusion_to_texts"):
        assert name in experiments.__all__
    assert experiments.text_occlusion is product.text_occlusion


# ---- refusals, before the encoder runs ----------------------------------------------------------------------------------------------
class Reached(Exception):
    pass


def guarded(model, monkeypatch):
    """Every way into the encoder raises: its ``forward``, the image trunk's and the label mean's."""
    entered = []

    def encoder(*a, **kw):
        entered.append(1)
        raise Reached
    monkeypatch.setattr(model.encoder, "forward", encoder)
    for part in ("image_encoder", "label_encoder"):
        if hasattr(model.encoder, part):
            monkeypatch.setattr(getattr(model.encoder, part), "forward", encoder)
            if part == "label_encoder":
                monkeypatch.setattr(model.encoder.label_encoder, "check", encoder)
    return entered


@pytest.mark.parametrize("kind,level", [(_L, "history"), (_T, "history"), (_B, "history"), (_LL, "label"), (_TL, "label"), (_TL, "history")])
def test_arguments_are_checked_before_the_encoder_runs(kind, level, monkeypatch):
    images, cap, lengths, index, labels = T.inputs(torch.zeros(3, 3, 8, 8))
    model = build(kind)
    entered = guarded(model, monkeypatch)
    call = lambda **kw: text_occlusion(model, images, kw.pop("index", index), kw.pop("cap", cap), kw.pop("lengths", lengths),      # noqa: E731
                                       labels=kw.pop("labels", lab(kind, labels)), level=kw.pop("level", level), **kw)
    bad = cap.clone()
    bad[1, 2] = E.V
    with pytest.raises(IndexError, match="index out of range in self"):                  # explain_captions' rules
        call(cap=bad)
    with pytest.raises(IndexError, match="index out of range in self"):
        call(index=index + 1)
    with pytest.raises(ValueError, match=r"template_index must be an integer tensor of shape \[12\]"):
        call(index=index[:5])
    with pytest.raises(ValueError, match="lengths must be >= 1"):
        call(lengths=lengths - 2)
    with pytest.raises(ValueError, match="captions must be an int64 tensor"):
        call(cap=cap.int())
    with pytest.raises(ValueError, match="batch_size must be an int >= 1"):
        call(batch_size=0)
    with pytest.raises(TypeError, match="pad_index must be an int"):
        call(pad_index=0.0)
    for bad_level in ("patch", "pixel", "text", None, 0):                                # the new ones
        with pytest.raises(ValueError, match="level must be 'history' or 'label'.*occlusion_maps"):
            call(level=bad_level)
    for bad_fill in (True, False, -1, E.V, 1.0, None, "unk", "<unk>", (1,), torch.tensor(1)):
        with pytest.raises(ValueError, match=r'fill must be "pad" .* or an int token id in \[0, 300\)'):
            call(fill=bad_fill)
    with pytest.raises(ValueError, match=r'fill must be "pad"'):                         # "pad" is the call's pad_index: it must be a token too
        call(pad_index=-1)
    for bad_flag in (1, None, "yes"):
        with pytest.raises(TypeError, match="return_tokens must be a bool"):
            call(return_tokens=bad_flag)
    if level == "history":
        with pytest.raises(ValueError, match='level="history" needs captions of L >= 2 positions'):
            call(cap=torch.full((12, 1), E.EOS), lengths=torch.ones(12, dtype=torch.int64))
        with pytest.raises(ValueError, match=r'level="history": lengths must be <= L = 7'):   # a region past the last column otherwise
            call(lengths=lengths + 1)
    else:
        with pytest.raises(ValueError, match='level="label" needs labels.*level="history"'):
            call(labels=None)
        with pytest.raises(ValueError, match=r'labels must be an int64 tensor \[T, l\]'):
            call(labels=labels[0])
        model.train()                                                                    # the encoder's own rule: inference only
        with pytest.raises(RuntimeError, match="call model.eval()"):
            call()
        model.eval()
    assert not entered
    for ok in (dict(), dict(fill=1), dict(fill=0), dict(fill=E.V - 1), dict(fill="pad", pad_index=2), dict(return_tokens=True, batch_size=1)):
        with pytest.raises(Reached):                                                     # valid arguments reach it
            call(**ok)
    assert entered and all(entered)


def test_refusals_by_level_kind_and_pad_index(monkeypatch):
    images, cap, lengths, index, labels = T.inputs(torch.zeros(3, 3, 8, 8))
    for kind in (_L, _B, _T):                                                            # no labels: no label level
        model = build(kind)
        entered = guarded(model, monkeypatch)
        with pytest.raises(TypeError, match='level="label": .* takes no labels .*level="history" works for every kind'):
            text_occlusion(model, images, index, cap, lengths, labels=labels, level="label")
        with pytest.raises(TypeError, match='level="label": .* takes no labels'):
            text_occlusion(model, images, index, cap, lengths, level="label")
        with pytest.raises(Reached):                                                     # the history level takes every kind
            text_occlusion(model, images, index, cap, lengths)
        assert entered == [1]
    for kind in (_B, _T):
        one = build(kind, pad_index=1)
        entered = guarded(one, monkeypatch)
        with pytest.raises(NotImplementedError, match='level="history" with pad_index == 1.*position 0 attends over every position'):
            text_occlusion(one, images, index, cap, lengths, pad_index=1)
        assert not entered
        two = build(kind, pad_index=2)
        entered = guarded(two, monkeypatch)
        with pytest.raises(Reached):
            text_occlusion(two, images, index, cap, lengths, pad_index=2)
        assert entered == [1]


# ---- the variants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill_id", (0, 1, 299))
def test_variant_builder_against_the_restated_one(fill_id):
    _, cap, lengths, _, labels = T.inputs(torch.zeros(3, 3, 8, 8))
    # the inputs plus the two edges: a caption that is only <eos> (no real region) and full-length ones (L - 1 regions: rows 0 .. 3)
    only_eos = torch.zeros((1, T.L), dtype=torch.int64)
    only_eos[0, 0] = E.EOS
    cap, lengths = torch.cat([cap[:6], only_eos, cap[6:]]), torch.cat([lengths[:6], torch.tensor([1]), lengths[6:]])
    caption, region, inputs = product.history_variants(cap, lengths, fill_id)
    want_caption, want_region, want_inputs = T.history_inputs(cap, lengths, fill_id)
    assert torch.equal(caption, want_caption) and torch.equal(region, want_region) and torch.equal(inputs, want_inputs)
    assert inputs.dtype == torch.int64 and inputs.shape == (int(lengths.sum()), T.L - 1)
    real = T.real_mask(lengths, T.L - 1)
    for i in range(cap.shape[0]):
        mine = (caption == i).nonzero().squeeze(1)
        assert region[mine].tolist() == [-1] + [j for j in range(T.L - 1) if real[i, j]]     # base first, then the real regions in order
        assert int(real[i].sum()) == int(lengths[i]) - 1
        for k in mine.tolist():
            j = int(region[k])
            changed = (inputs[k] != cap[i, :-1]).nonzero().squeeze(1).tolist()
            assert changed == ([] if j < 0 or int(cap[i, j]) == fill_id else [j])        # only column j, and the captions are untouched
            assert j < 0 or (int(inputs[k, j]) == fill_id and int(cap[i, j]) != E.EOS and int(cap[i, j]) != E.PAD)
    assert region[caption == 6].tolist() == [-1] and int(real[6].sum()) == 0             # only <eos>
    assert region[caption == 0].tolist() == [-1, 0, 1, 2, 3, 4, 5]                       # full length
    row = labels[1]
    got = product.label_variants(row, fill_id)
    assert torch.equal(got, T.label_rows(row, fill_id)) and torch.equal(got[0], row) and got.shape == (4, 3)
    assert all(int(got[1 + k, k]) == fill_id and (got[1 + k] != row).sum() <= 1 for k in range(3))


# ---- the record and the readable form -----------------------------------------------------------------------------------------------
def test_text_occlusion_scores_record():
    a = TextOcclusionScores(torch.zeros(2), torch.ones(2, 4))
    assert a._fields == ("base", "drop", "token_drop") and a.token_drop is None
    d = a.map(lambda t: t.double())
    assert isinstance(d, TextOcclusionScores) and d.base.dtype == d.drop.dtype == torch.float64 and d.token_drop is None
    c = TextOcclusionScores.cat([a, a.map(lambda t: t + 1)])
    assert isinstance(c, TextOcclusionScores) and c.base.tolist() == [0, 0, 1, 1] and c.drop.shape == (4, 4) and c.token_drop is None
    b = TextOcclusionScores(torch.zeros(2), torch.ones(2, 4), torch.full((2, 5, 4), 2.0))
    c = TextOcclusionScores.cat([b, b])
    assert c.token_drop.shape == (4, 5, 4) and b.map(torch.clone).token_drop is not b.token_drop


def test_occlusion_to_texts_on_captions_and_labels():
    from deephumor_amd.data import SPECIAL_TOKENS, Vocab, WordPunctTokenizer
    from deephumor_amd.experiments import text_to_seq
    tok = WordPunctTokenizer()
    vocab = Vocab(tok.tokenize("one does not simply walk into mordor boromir"))
    eos, pad = vocab.stoi[SPECIAL_TOKENS["EOS"]], vocab.stoi[SPECIAL_TOKENS["PAD"]]
    ids = text_to_seq("one does not simply", vocab, tok)[0].tolist()
    cap = torch.full((3, 6), pad, dtype=torch.int64)
    cap[0, :4], cap[0, 4] = torch.tensor(ids), eos                                       # four words, <eos>, one pad
    cap[1, 0] = eos                                                                      # only <eos>: no real region
    cap[2, :5], cap[2, 5] = torch.tensor(ids + ids[:1]), eos                             # full length: L - 1 regions
    drop = torch.arange(15.0).view(3, 5)
    out = occlusion_to_texts(cap, TextOcclusionScores(torch.zeros(3), drop), vocab)
    assert out[0] == [("one", 0.0), ("does", 1.0), ("not", 2.0), ("simply", 3.0)]
    assert out[1] == []
    assert out[2] == [("one", 10.0), ("does", 11.0), ("not", 12.0), ("simply", 13.0), ("one", 14.0)]
    assert occlusion_to_texts(cap, drop, vocab) == out                                   # the bare tensor is taken too
    labels = torch.tensor([[vocab.stoi["boromir"], vocab.stoi["mordor"], pad]])          # a label row: every column, a pad included
    got = occlusion_to_texts(labels[torch.tensor([0, 0])], torch.tensor([[0.5, -0.25, 0.125], [1.0, 2.0, 3.0]]), vocab)
    assert got == [[("boromir", 0.5), ("mordor", -0.25), ("<pad>", 0.125)], [("boromir", 1.0), ("mordor", 2.0), ("<pad>", 3.0)]]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images4():
    return T.inputs(synth_images(E.N_TEMPLATES, seed=0))


_SD = {}


def weights(kind):
    if kind not in _SD:
        sd = {k: v.detach() for k, v in build(kind).state_dict().items()}
        _SD[kind] = (sd, None)
    return _SD[kind][0]


def encoded(kind, images4):
    if _SD.get(kind, (None, None))[1] is None:
        sd = weights(kind)
        _SD[kind] = (sd, T.encode3(kind, sd, images4[0], images4[4]))
    return _SD[kind][1]


def half_ulp_bound(tokens, drop):
    """``test_occlusion_gpu.py::check_shapes``' bound: every per-token difference is rounded to fp32 once, and ``drop`` once."""
    return (np.spacing(np.abs(tokens.numpy())).astype(np.float64).sum(1) + np.spacing(np.abs(drop.numpy())).astype(np.float64)) / 2


def check_golden_inputs(g, images4):
    _, cap, lengths, index, labels = images4
    assert int(g["seed"]) == E.SEED and np.array_equal(g["captions"], cap.numpy()) and np.array_equal(g["template_index"], index.numpy())
    assert np.array_equal(g["lengths"], lengths.numpy()) and tuple(g["templates"]) == T.O.TEMPLATES and np.array_equal(g["labels"], labels.numpy())


def compare(kind, level, name, got, want):
    errs = tuple(float(np.abs(a.double().numpy() - np.asarray(b)).max()) for a, b in zip(got, want))
    seen = MEASURED.get((kind, level, name))
    print(f"[text occlusion cpu] {kind} {level} fill={name}: restatement vs G29 base {errs[0]:.3e}, drop {errs[1]:.3e}, tokens {errs[2]:.3e} "
          f"(measured {seen})")
    assert seen is not None, "no measured value recorded"
    for e, w in zip(errs, seen):
        assert e <= T.gate(w), (errs, seen)


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("name,fill_id", T.FILLS)
def test_history_restatement_against_g29_and_its_structure(kind, name, fill_id, images4):
    images, cap, lengths, index, labels = images4
    g = T.golden(kind)
    check_golden_inputs(g, images4)
    sd = weights(kind)
    nh = E.HP[kind].get("n_heads", 0)
    caption, region, rows = T.history_rows(kind, sd, nh, *encoded(kind, images4), cap, lengths, index, fill_id)
    base, drop, tokens = T.history_scores(caption, region, rows, lengths)
    assert base.shape == (12,) and drop.shape == (12, 6) and tokens.shape == (12, 7, 6) and base.dtype == drop.dtype == tokens.dtype == torch.float32
    compare(kind, "history", name, (base, drop, tokens), (g["base"], g[f"hist_{name}_drop"], g[f"hist_{name}_tokens"]))
    # exact zeros: positions p <= j, pads, regions that are not real -- in the restatement and in G29
    real = T.real_mask(lengths, 6)
    p, j = torch.arange(7)[None, :, None], torch.arange(6)[None, None, :]
    live = real[:, None, :] & (j < p) & (p < lengths[:, None, None])
    for tk, dr in ((tokens, drop), (torch.from_numpy(g[f"hist_{name}_tokens"]), torch.from_numpy(g[f"hist_{name}_drop"]))):
        assert bool((tk[~live] == 0).all()) and bool((dr[~real] == 0).all()) and bool((tk[live] != 0).all()) and bool((dr[real] != 0).all())
    assert bool((tokens[cap == E.PAD] == 0).all())
    # causality of the restated decoders themselves: a variant's row is the base row at every p <= j, bit for bit
    for k in range(caption.shape[0]):
        if int(region[k]) >= 0:
            first = int((caption == caption[k]).nonzero()[0])
            assert torch.equal(rows[k, :int(region[k]) + 1], rows[first, :int(region[k]) + 1])
    for x in (base, drop, tokens):                                                       # the copy of template 0: rows 4 c + 3 and 4 c
        assert torch.equal(x[3::4], x[0::4])
    total = tokens.double().sum(1).numpy()
    assert bool((np.abs(total - drop.double().numpy()) <= half_ulp_bound(tokens, drop)).all())
    # the filter of the GPU test: at least half of the real entries stand above twice the gate (all do at these shapes)
    share = T.share_passing(g[f"hist_{name}_drop"], real.numpy(), T.gate(T.WORST[(kind, "history", name, "g29")][1]))
    print(f"[text occlusion cpu] {kind} history fill={name}: {share:.0%} of the real entries exceed twice the gate")
    assert share >= 0.5


@pytest.mark.parametrize("kind", (_L, _T))
def test_a_fill_equal_to_the_token_changes_nothing(kind, images4):
    """Row 1 of the inputs (caption 0 under template 1), its column 2 filled with the token that is already there."""
    images, cap, lengths, index, labels = images4
    sd = weights(kind)
    same = int(cap[1, 2])
    caption, region, rows = T.history_rows(kind, sd, E.HP[kind].get("n_heads", 0), *encoded(kind, images4), cap[1:2], lengths[1:2], index[1:2], same)
    base, drop, tokens = T.history_scores(caption, region, rows, lengths[1:2])
    assert float(drop[0, 2]) == 0.0 and bool((tokens[0, :, 2] == 0.0).all()) and bool((drop[0, [0, 1, 3, 4, 5]] != 0).all())
    got_caption, got_region, got_inputs = product.history_variants(cap[1:2], lengths[1:2], same)
    assert torch.equal(got_inputs[3], cap[1, :-1]) and int(got_region[3]) == 2


@pytest.mark.parametrize("kind", T.LABEL_KINDS)
def test_label_restatement_against_g29_and_its_structure(kind, images4):
    images, cap, lengths, index, labels = images4
    g = T.golden(kind)
    check_golden_inputs(g, images4)
    sd = weights(kind)
    base, drop, tokens = T.label_level(kind, sd, E.HP[kind].get("n_heads", 0), images, labels, cap, index, T.UNK)
    assert base.shape == (12,) and drop.shape == (12, 3) and tokens.shape == (12, 7, 3)
    compare(kind, "label", "unk", (base, drop, tokens), (g["label_base"], g["label_drop"], g["label_tokens"]))
    assert bool((tokens[cap == E.PAD] == 0).all()) and bool((torch.from_numpy(g["label_tokens"])[cap == E.PAD] == 0).all())
    assert bool((drop != 0).all())
    for x in (base, drop, tokens):
        assert torch.equal(x[3::4], x[0::4])
    total = tokens.double().sum(1).numpy()
    assert bool((np.abs(total - drop.double().numpy()) <= half_ulp_bound(tokens, drop)).all())
    # a label word replaced by itself: the variant is the base
    t = 1
    same = T.label_rows(labels[t], int(labels[t, 0]))
    assert torch.equal(same[1], same[0]) and torch.equal(product.label_variants(labels[t], int(labels[t, 0]))[1], labels[t])
    share = T.share_passing(g["label_drop"], np.ones((12, 3), dtype=bool), T.gate(T.WORST[(kind, "label", "unk", "g29")][1]))
    print(f"[text occlusion cpu] {kind} label: {share:.0%} of the entries exceed twice the gate")
    assert share >= 0.5
    # the history level's base of G29 is the label level's: one reference model, nothing hidden (two encoder batches: to fp32 rounding)
    assert float(np.abs(g["label_base"] - g["base"]).max()) <= 1e-5


# ---- the pins -------------------------------------------------------------------------------------------------------------------------
def test_the_pins_did_not_move():
    import test_occlusion_cpu as before
    from deephumor_amd import _abi, _build, hip
    before.test_the_pins_did_not_move()                                                  # the header regex of test_occlusion_cpu.py itself
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    n_protos = len(re.findall(r"^(?:int|const char\*|void|unsigned long long|double|float)\s+\*?dh_\w+\s*\(", text, flags=re.M))
    assert n_protos == 129 and "129 entry points" in open(os.path.join(ROOT, "README.md")).read()
    assert int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1)) == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    assert len(hip.SIGNATURES) == len(_abi.SIGNATURES) == 124
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    lib.dh_option_count.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35 and lib.dh_option_count() == 15
