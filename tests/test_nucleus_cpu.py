"""Nucleus (top-p) filtering without a GPU: ``beam.check_top_p``, the ABI of ``dh_beam_row_sample_nucleus``, its argument contract,
golden G20 pinned to the patched CPU restatement of the reference, and the restatement's own edge cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import KINDS, captions_and_lengths, golden, synthetic_sd, synth_images
from nucleus_ref import nucleus_keep, nucleus_row_sample, patched_keep_top_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20_KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
NAME = "dh_beam_row_sample_nucleus"


def test_check_top_p():
    from deephumor_amd.models.beam import check_top_p
    for ok in (1.0, 1, 0.8, 1e-6, np.float32(0.5), np.float64(0.97)):
        assert check_top_p(ok) == float(ok)
    assert isinstance(check_top_p(1), float)
    for bad in (True, False, float("nan"), 0, 0.0, -0.1, 1.0000001, 1.5, 2, float("inf")):
        with pytest.raises(ValueError):
            check_top_p(bad)
    for bad in ("0.8", None, [0.8], torch.tensor(0.8), 0.5 + 0j):
        with pytest.raises(TypeError):
            check_top_p(bad)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_top_p_fails_before_the_encoder(kind):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    model.encode = boom
    images = torch.zeros(1, 3, 224, 224)
    for bad, exc in ((0, ValueError), (1.5, ValueError), (True, ValueError), (float("nan"), ValueError), ("0.9", TypeError)):
        for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
            with pytest.raises(exc):
                call(images, top_p=bad)
    dec = model.decoder
    with pytest.raises(ValueError):
        if kind == "CaptioningLSTM":
            dec.generate_batch(torch.zeros(1, 256), top_p=0)
        else:
            dec.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), top_p=0)


def test_helper_keyword_and_method_surface():
    """``top_p`` is a keyword behind the reference's positional signature; the reference-style methods have no nucleus."""
    import inspect
    from deephumor_amd.models.beam import BeamSearchHelper
    names = list(inspect.signature(BeamSearchHelper.__init__).parameters)
    assert names[1:7] == ["temperature", "beam_size", "top_k", "unk_index", "eos_index", "device"] and "top_p" in names[7:]
    assert inspect.signature(BeamSearchHelper.__init__).parameters["top_p"].default == 1.0
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", top_p=0.9)
    assert h.top_p == 0.9
    logits = torch.zeros(3, 8)
    with pytest.raises(NotImplementedError):
        h.sample_k_indices(logits)
    with pytest.raises(NotImplementedError):
        h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", top_p=0.0)


def test_overflow_message_names_top_p():
    from deephumor_amd import hip
    from deephumor_amd.models.beam import BeamOverflow, BeamSearchHelper
    with pytest.raises(BeamOverflow, match="top_p=0.9"):
        BeamSearchHelper.raise_for(hip.ERR_OVERFLOW, 0.9)
    with pytest.raises(BeamOverflow) as e:
        BeamSearchHelper.raise_for(hip.ERR_OVERFLOW)
    assert "top_p" not in str(e.value)


def test_abi_header_table_and_library_agree():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NAME + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[NAME]
    assert len(args) == len(sig) == 25
    for a, t in zip(args, sig):                         # argument by argument: pointer / int / float / uint64_t
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_uint64 if a.startswith("uint64_t") \
            else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args if "top_p" in a or a.endswith("exact") or "first_pos" in a or "group_max" in a] == \
        ["group_max", "top_p", "first_pos", "exact"]
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, NAME)
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35
    # one entry point for every route, not six twins
    assert [n for n in _abi.SIGNATURES if "nucleus" in n] == [NAME]
    # the existing prototypes keep their arity
    assert len(_abi.SIGNATURES["dh_beam_row_sample"]) == 18 and len(_abi.SIGNATURES["dh_beam_row_sample_groups_prompted"]) == 23


def test_entry_point_rejects_top_p_outside_the_open_interval():
    """Checked before any HIP call: otherwise valid arguments (pointers are never dereferenced on the host) with ``top_p`` of 0, 1
    and 1.5 return DH_ERR_BAD_ARG; so do NaN and a negative value."""
    from deephumor_amd import hip
    lib = hip.load()
    fn = getattr(lib, NAME)
    for top_p in (0.0, 1.0, 1.5, float("nan"), -0.5):
        #        logits ldl  V   gmax gm ng gc rows rpi beam top_k top_p  T   unk noise seed sp img0 step fp exact pi pv err stream
        assert fn(64, 128, 100, None, 0, 2, 64, 2, 1, 3, 5, top_p, 1.0, 1, None, 0, None, 0, 0, None, 0, 64, 64, 64, None) == 1, top_p
    # a valid top_p reaches the other argument checks (NULL logits)
    assert fn(None, 128, 100, None, 0, 2, 64, 2, 1, 3, 5, 0.5, 1.0, 1, None, 0, None, 0, 0, None, 0, 64, 64, 64, None) == 1


# ---- the restatement's own edge cases -------------------------------------------------------------------------------------------
def _filtered(vals):
    """A keep_top_k result: the given logits at columns 2.., -inf elsewhere (column 1 is <unk>)."""
    row = torch.full((1, len(vals) + 4), float("-inf"))
    row[0, 2:2 + len(vals)] = torch.tensor(vals)
    return row


def test_one_dominant_token_keeps_beam_size_tokens():
    filt = _filtered([0.0, 12.0, 1.0, 0.5, 3.0, 2.0])             # p(12.0) > 0.999 > top_p
    for beam in (1, 3, 5):
        keep, margin = nucleus_keep(filt, 1.0, 0.9, beam)
        assert keep[0].nonzero().flatten().tolist() == sorted([3, 6, 7, 4, 5][:beam])       # by p descending: columns 3, 6, 7, 4, 5, 2
        assert margin > 0.09


def test_equal_p_orders_by_index():
    # four bit-equal logits (p = 0.2 each) behind one of p = 0.2 + ...: with top_p between two prefixes the LOWER indices stay
    filt = _filtered([1.0, 1.0, 1.0, 1.0, 1.0])
    keep, margin = nucleus_keep(filt, 1.0, 0.5, 1)                # prefixes 0, .2, .4, .6, .8: positions 0..2 stay
    assert keep[0].nonzero().flatten().tolist() == [2, 3, 4] and abs(margin - 0.1) < 1e-6
    keep, _ = nucleus_keep(filt, 1.0, 0.5, 4)                     # the beam floor reaches further than the nucleus
    assert keep[0].nonzero().flatten().tolist() == [2, 3, 4, 5]
    filt = _filtered([1.0, 3.0, 1.0, 3.0, 1.0])                   # two classes of equal p: each in index order
    keep, _ = nucleus_keep(filt, 1.0, 0.9, 1)
    p = torch.softmax(filt, -1)[0]
    assert float(p[3] + p[5] + p[2]) < 0.9 <= float(p[3] + p[5] + p[2] + p[4])
    assert keep[0].nonzero().flatten().tolist() == [2, 3, 4, 5]   # 3, 5 (p high), then 2, 4 of the low class; 6 leaves


def test_top_p_above_every_prefix_keeps_all_survivors():
    filt = _filtered([0.3, -1.0, 2.0, 0.1, 0.7])
    keep, margin = nucleus_keep(filt, 0.7, 0.999999, 2)
    p = torch.softmax(filt / 0.7, -1)[0]
    last = 1.0 - float(p[torch.isfinite(filt[0])].min())          # the largest exclusive prefix
    assert last < 0.999999 and torch.equal(keep, torch.isfinite(filt)) and margin > 0


def test_row_sample_restatement_races_over_the_kept_only():
    logits = torch.randn(4, 60, generator=torch.Generator().manual_seed(0)) * 3
    noise = torch.empty(4, 60).exponential_(1, generator=torch.Generator().manual_seed(1))
    noise[:, :] = torch.where(torch.rand(4, 60, generator=torch.Generator().manual_seed(2)) < 0.5, noise, noise * 1e-3)
    picks, vals, margin, keep = nucleus_row_sample(logits, noise, 1.0, 3, 20, 0.5)
    assert bool(keep.gather(1, picks).all()) and bool((keep.sum(1) >= 3).all()) and bool((keep.sum(1) < 20).any())
    assert bool(torch.isfinite(vals).all()) and torch.allclose(vals.exp().sum(1), torch.ones(4), atol=1e-5)
    assert not keep[:, 1].any()                                   # <unk>


# ---- golden G20 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_g20_is_pinned_to_the_patched_restatement(kind):
    """The committed G20 arrays (recorded from the real reference by tools/make_nucleus_golden.py, its ``filter_top_k`` wrapped)
    re-derived from ``oracle.ref_path.model_generate`` with ``BeamBook.keep_top_k`` wrapped the same way, under the same seed.
    The margin is a condition on the fixture's inputs (>= 1e-3, recorder's rule), and the restatement meets the same boundary
    distances to its fp32 agreement with the reference's logits."""
    from oracle import ref_path as R
    g = golden(f"g20_nucleus_{kind}.npz")
    assert abs(float(g["top_p"]) - 0.8) < 1e-7
    sd, hp = synthetic_sd(kind)
    images = synth_images(4, seed=0)
    _, _, labels = captions_and_lengths()
    differs = 0
    for i in range(2):
        img = int(g[f"image_{i}"])
        lab = labels[img:img + 1] if "WithLabels" in kind else None
        margins = []
        torch.manual_seed(int(g[f"seed_{i}"]))
        with patched_keep_top_k(0.8, margins):
            out = R.model_generate(kind, sd, hp, images[img:img + 1], lab, **dict(G20_KW, max_len=int(g["max_len"]))).reshape(-1).numpy()
        assert "beam.py:32-37" in R.BeamBook.keep_top_k.__doc__   # the patch is gone again
        assert out.tolist() == g[f"out_{i}"].tolist(), (kind, i)
        assert float(g[f"margin_{i}"]) >= 1e-3
        assert abs(min(margins) - float(g[f"margin_{i}"])) < 1e-4
        kept, surv = g[f"kept_{i}"].tolist()
        assert 0 < kept < surv                                    # the nucleus cut something
        differs += g[f"out_{i}"].tolist() != g[f"plain_{i}"].tolist()
    print(kind, "captions that differ from top_p = 1:", differs)


def test_g20_differs_from_the_plain_captions():
    """At least one fixture caption is not the ``top_p = 1`` caption of its seed: G20 cannot pass without the feature."""
    n = 0
    for kind in KINDS:
        g = golden(f"g20_nucleus_{kind}.npz")
        n += sum(g[f"out_{i}"].tolist() != g[f"plain_{i}"].tolist() for i in range(2))
    assert n >= 1
