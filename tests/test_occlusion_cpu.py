"""``experiments.occlusion_maps`` without a GPU: its argument rules (all of which run before the encoder), the refusals by level, kind
and ``pad_index``, the region geometry, the ``OcclusionScores`` record, the restatement of ``occlusion_ref`` against a dense fp64
statement and against golden G27, and the pins this feature must not move: 129 prototypes, ABI 35, 124 signatures, 15 options.

Bounds.  The restatement runs ``oracle.ref_path`` in fp32 and takes log-softmax and sums in fp64; the dense statement is the fp64
decoder of ``attention_maps_ref``; G27 is the real reference in fp32.  ``test_explain_cpu.py`` holds the same two comparisons per token
at 1e-4; a caption sums at most L = 7 tokens and a drop is the difference of two such sums: 7e-4 and 1.4e-3."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attention_maps_ref as AR
import explain_ref as E
import occlusion_ref as O
from helpers import synth_images
from deephumor_amd import experiments
from deephumor_amd.experiments import OcclusionScores, attention_to_heatmaps, occlusion_maps
from deephumor_amd.experiments import occlusion as product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_ATOL = O.L * 1e-4
DROP_ATOL = 2 * O.L * 1e-4


def build(kind, **extra):
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_state_dict
    model = getattr(M, kind)(**dict(E.HP[kind], **extra)).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=E.SEED))
    return model


def test_it_is_exported():
    assert "occlusion_maps" in experiments.__all__ and "OcclusionScores" in experiments.__all__
    assert experiments.occlusion_maps is product.occlusion_maps


# ---- validation, before the encoder runs --------------------------------------------------------------------------------------------
class Reached(Exception):
    pass


def guarded(model, monkeypatch):
    entered = []

    def encoder(*a, **kw):
        entered.append(1)
        raise Reached
    monkeypatch.setattr(model.encoder, "forward", encoder)
    return entered


@pytest.mark.parametrize("kind,level", [("CaptioningTransformer", "patch"), ("CaptioningTransformer", "pixel"), ("CaptioningLSTM", "pixel"),
                                        ("CaptioningTransformerBase", "pixel")])
def test_arguments_are_checked_before_the_encoder_runs(kind, level, monkeypatch):
    images, cap, lengths, index, _ = O.inputs(torch.zeros(3, 3, 8, 8))
    model = build(kind)
    entered = guarded(model, monkeypatch)
    call = lambda **kw: occlusion_maps(model, kw.pop("images", images), kw.pop("index", index), kw.pop("cap", cap),      # noqa: E731
                                       kw.pop("lengths", lengths), level=level, **kw)
    bad = cap.clone()
    bad[1, 2] = E.V
    with pytest.raises(IndexError, match="index out of range in self"):                  # explain_captions' rules
        call(cap=bad)
    with pytest.raises(IndexError, match="index out of range in self"):
        call(index=index + 1)
    with pytest.raises(ValueError, match=r"template_index must be an integer tensor of shape \[12\]"):
        call(index=index[:5])
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[12\]"):
        call(lengths=lengths.float())
    with pytest.raises(ValueError, match="lengths must be >= 1"):
        call(lengths=lengths - 2)
    with pytest.raises(ValueError, match="captions must be an int64 tensor"):
        call(cap=cap.int())
    with pytest.raises(ValueError, match="batch_size must be an int >= 1"):
        call(batch_size=0)
    with pytest.raises(TypeError, match="pad_index must be an int"):
        call(pad_index=0.0)
    with pytest.raises(ValueError, match="level must be 'patch' or 'pixel'"):            # the new ones
        occlusion_maps(model, images, index, cap, lengths, level="region")
    with pytest.raises(ValueError, match="level must be 'patch' or 'pixel'"):
        occlusion_maps(model, images, index, cap, lengths, level=None)
    for bad_flag in (1, None, "yes"):
        with pytest.raises(TypeError, match="return_tokens must be a bool"):
            call(return_tokens=bad_flag)
    if level == "pixel":
        for grid in ((0, 2), (2, 0), (9, 2), (2, 9), (2,), (2, 2, 2), (2.0, 2), (True, 2), 4, None, "22"):
            with pytest.raises(ValueError, match=r"grid must be two ints \(gh, gw\) with 1 <= gh <= 8 and 1 <= gw <= 8"):
                call(grid=grid)
        for fill in ((0.0, 1.0), (0.0, 1.0, 2.0, 3.0), "0", None, float("nan"), float("inf"), (0.0, float("nan"), 0.0), True, [0.0, "1", 0.0],
                     torch.zeros(2)):
            with pytest.raises(ValueError, match="fill must be one finite real number or one per channel"):
                call(fill=fill)
        with pytest.raises(ValueError, match=r"template_images must be a tensor \[T, C, H, W\]"):
            call(images=images[:, 0])
    else:
        call_ok = dict(grid=(0, 99), fill="ignored")                                     # patch level ignores both
        with pytest.raises(Reached):
            call(**call_ok)
        del entered[:]
    assert not entered
    for ok in (dict(), dict(grid=(8, 8)), dict(grid=[1, 3], fill=(0.5, -1, 2.0)), dict(fill=torch.tensor([0.1, 0.2, 0.3])), dict(fill=1),
               dict(return_tokens=True, batch_size=1)):
        if level == "patch" and "grid" in ok:
            continue
        with pytest.raises(Reached):                                                     # valid arguments reach it
            call(**ok)
    assert entered and all(entered)


def test_refusals_by_level_kind_and_pad_index(monkeypatch):
    images, cap, lengths, index, labels = O.inputs(torch.zeros(3, 3, 8, 8))
    for kind in E.KINDS[:3]:                                                             # no encoder attention: no patch level
        model = build(kind)
        entered = guarded(model, monkeypatch)
        with pytest.raises(TypeError, match='level="patch": .* has no encoder attention'):
            occlusion_maps(model, images, index, cap, lengths, labels=labels if "WithLabels" in kind else None)
        with pytest.raises(Reached):                                                     # the pixel level takes every kind
            occlusion_maps(model, images, index, cap, lengths, labels=labels if "WithLabels" in kind else None, level="pixel", grid=(2, 2))
        assert entered == [1]
    for kind in E.CROSS_KINDS:
        one = build(kind, pad_index=1) if kind == "CaptioningTransformer" else None
        if one is None:
            continue
        entered = guarded(one, monkeypatch)
        with pytest.raises(NotImplementedError, match='level="patch" with pad_index == 1'):
            occlusion_maps(one, images, index, cap, lengths)
        two = build(kind, pad_index=2)
        entered2 = guarded(two, monkeypatch)
        with pytest.raises(ValueError, match='masks no image key.*level="pixel"'):
            occlusion_maps(two, images, index, cap, lengths)
        for model in (one, two):
            with pytest.raises(Reached):
                occlusion_maps(model, images, index, cap, lengths, level="pixel")
        assert entered == [1] and entered2 == [1]


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def dense_region_index(h, w, grid):
    """Pixel (y, x) belongs to the region (a, b) with a * h // gh <= y < (a + 1) * h // gh: found by trying every a, b."""
    gh, gw = grid
    out = np.full((h, w), -1)
    for y in range(h):
        a = [a for a in range(gh) if a * h // gh <= y < (a + 1) * h // gh]
        for x in range(w):
            b = [b for b in range(gw) if b * w // gw <= x < (b + 1) * w // gw]
            assert len(a) == 1 and len(b) == 1                                           # a partition: every pixel in exactly one region
            out[y, x] = a[0] * gw + b[0]
    return out


@pytest.mark.parametrize("h,w,grid", [(224, 224, (3, 2)), (224, 224, (7, 7)), (224, 224, (1, 1)), (10, 7, (3, 7)), (5, 9, (5, 4)), (8, 8, (3, 3))])
def test_region_geometry(h, w, grid):
    if (h, w, grid) == (224, 224, (3, 2)):
        assert product.region_edges(224, 3) == [0, 74, 149, 224] and product.region_edges(224, 2) == [0, 112, 224]
        assert O.edges(224, 3) == [0, 74, 149, 224]
    want = dense_region_index(h, w, grid)
    g = torch.Generator().manual_seed(h * w)
    image = torch.rand(3, h, w, generator=g) + 1.0                                       # no pixel equals a fill value
    fill = [-1.0, -2.0, -3.0]
    got = product.occluded_images(image, grid, fill)
    boxes = O.regions(h, w, grid)
    assert got.shape == (1 + grid[0] * grid[1], 3, h, w) and torch.equal(got[0], image) and len(boxes) == grid[0] * grid[1]
    for r, box in enumerate(boxes):
        inside = torch.from_numpy(want == r)
        assert bool(inside.any())                                                        # never empty
        for c in range(3):
            assert bool((got[1 + r, c][inside] == fill[c]).all()) and torch.equal(got[1 + r, c][~inside], image[c][~inside])
        assert torch.equal(got[1 + r], O.occlude(image, box, fill))                      # the restatement's own occluder agrees
    assert torch.equal(product.occluded_images(image.to(torch.bfloat16), grid, fill)[1:].float(),
                       torch.stack([O.occlude(image.to(torch.bfloat16), b, fill) for b in boxes]).float())


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def test_occlusion_scores_record():
    a = OcclusionScores(torch.zeros(2), torch.ones(2, 4))
    assert a._fields == ("base", "drop", "token_drop") and a.token_drop is None
    d = a.map(lambda t: t.double())
    assert isinstance(d, OcclusionScores) and d.base.dtype == d.drop.dtype == torch.float64 and d.token_drop is None
    c = OcclusionScores.cat([a, a.map(lambda t: t + 1)])
    assert isinstance(c, OcclusionScores) and c.base.tolist() == [0, 0, 1, 1] and c.drop.shape == (4, 4) and c.token_drop is None
    b = OcclusionScores(torch.zeros(2), torch.ones(2, 4), torch.full((2, 7, 4), 2.0))
    c = OcclusionScores.cat([b, b])
    assert c.token_drop.shape == (4, 7, 4) and b.map(torch.clone).token_drop is not b.token_drop
    maps = attention_to_heatmaps(torch.arange(8.0).view(2, 4), size=(6, 6), grid=(2, 2))     # [n, R] -> [n, H, W] with the existing helper
    # a corner pixel lies beyond its cell's centre: the clamped bilinear weights give the corner cell's value, to fp32 rounding
    assert maps.shape == (2, 6, 6) and float(maps[0, 0, 0]) == 0.0 and abs(float(maps[1, -1, -1]) - 7.0) <= 1e-6


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images4():
    return O.inputs(synth_images(E.N_TEMPLATES, seed=0))


@pytest.mark.parametrize("kind", E.CROSS_KINDS)
def test_patch_restatement_against_the_dense_statement_and_g27(kind, images4):
    """Dense fp64: ``attention_maps_ref.teacher_forced_maps``' whole decoder on ``enc_out`` with one row zeroed, one variant at a time."""
    images, cap, lengths, index, labels = images4
    g = O.golden(kind)
    assert int(g["seed"]) == E.SEED and np.array_equal(g["captions"], cap.numpy()) and np.array_equal(g["template_index"], index.numpy())
    assert np.array_equal(g["lengths"], lengths.numpy()) and tuple(g["templates"]) == O.TEMPLATES and np.array_equal(g["labels"], labels.numpy())
    sd = {k: v.detach() for k, v in build(kind).state_dict().items()}
    nh = E.HP[kind]["n_heads"]
    with torch.no_grad():
        start, enc = O.R._encode(kind, sd, images[:3], labels[:3])
    start, enc = start[torch.tensor(O.TEMPLATES)], enc[torch.tensor(O.TEMPLATES)]
    base, drop, tokens = O.patch_level(sd, nh, start, enc, cap, index)
    assert base.shape == (12,) and drop.shape == (12, 49) and tokens.shape == (12, O.L, 49)
    assert bool((tokens[cap == E.PAD] == 0).all()) and float((tokens.sum(1) - drop).abs().max()) < 1e-12
    assert torch.equal(drop[0::4], drop[3::4]) and torch.equal(base[0::4], base[3::4])   # the copy of template 0
    worst = 0.0
    for i in (0, 5, 10):                                                                 # one caption of every length, three templates
        t = int(index[i])
        for s in (0, 24, 48):
            e = enc[t:t + 1].clone()
            e[0, s] = 0.0
            _, logits = AR.teacher_forced_maps(sd, start[t:t + 1], e, cap[i:i + 1, :-1], E.PAD, nh, with_logits=True)
            occluded = float(E.token_logprobs(logits, cap[i:i + 1]).sum())
            worst = max(worst, abs(float(base[i] - drop[i, s]) - occluded))
    print(f"[occlusion cpu] {kind} patch: restatement vs dense fp64 {worst:.3e} (bound {BASE_ATOL:.1e})")
    assert worst <= BASE_ATOL
    eb, ed = float(np.abs(base.numpy() - g["patch_base"]).max()), float(np.abs(drop.numpy() - g["patch_drop"]).max())
    print(f"[occlusion cpu] {kind} patch: restatement vs G27 base {eb:.3e}, drop {ed:.3e}; G27 margin {O.margin(g['patch_drop']):.3e}")
    assert eb <= BASE_ATOL and ed <= DROP_ATOL
    assert np.array_equal(g["patch_base"], g["pixel_base"])                              # one reference model, one unoccluded image


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformerBase", "CaptioningTransformerWithLabels"))
def test_pixel_restatement_against_g27(kind, images4):
    images, cap, lengths, index, labels = images4
    g = O.golden(kind)
    assert tuple(g["grid"]) == O.GOLDEN_GRID and tuple(g["fill"]) == O.FILL and g["pixel_drop"].shape == (12, 4)
    sd = {k: v.detach() for k, v in build(kind).state_dict().items()}
    rows = torch.tensor([0, 5, 10, 3])                                                   # every length, every template (3: the copy)
    base, drop, tokens = O.pixel_level(kind, sd, E.HP[kind].get("n_heads", 0), images, labels, cap[rows], index[rows], O.GOLDEN_GRID, O.FILL)
    assert torch.equal(base[0], base[3]) and torch.equal(drop[0], drop[3])
    assert bool((tokens[cap[rows] == E.PAD] == 0).all()) and float((tokens.sum(1) - drop).abs().max()) < 1e-12
    eb = float(np.abs(base.numpy() - g["pixel_base"][rows.numpy()]).max())
    ed = float(np.abs(drop.numpy() - g["pixel_drop"][rows.numpy()]).max())
    print(f"[occlusion cpu] {kind} pixel: restatement vs G27 base {eb:.3e}, drop {ed:.3e}; G27 margin {O.margin(g['pixel_drop']):.3e}")
    assert eb <= BASE_ATOL and ed <= DROP_ATOL
    assert O.margin(g["pixel_drop"]) > 0 and np.array_equal(g["pixel_drop"][0::4], g["pixel_drop"][3::4])


# ---- the pins -------------------------------------------------------------------------------------------------------------------------
def test_the_pins_did_not_move():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    n_protos = len(re.findall(r"^(?:int|const char\*|void|unsigned long long|double|float)\s+\*?dh_\w+\s*\(", text, flags=re.M))
    assert n_protos == 129 and "129 entry points" in open(os.path.join(ROOT, "README.md")).read()
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    assert len(hip.SIGNATURES) == len(_abi.SIGNATURES) == 124
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    lib.dh_option_count.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35 and lib.dh_option_count() == 15
