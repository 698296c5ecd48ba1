"""``return_attention`` without a GPU: the fp64 restatement every GPU test measures against (``attention_maps_ref.teacher_forced_maps``)
is pinned to the real reference -- golden G23, recorded by ``tools/make_attention_golden.py`` from a hook on the reference's
last-layer encoder attention, and the oracle's logits --, the committed G23 files are what the tests need them to be, and the
Python-side pieces (``beam.check_return_attention``, ``experiments.attention_to_heatmaps``, the C-ABI table) behave as documented."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import attention_maps_ref as R
from helpers import KINDS, captions_and_lengths, synthetic_sd, synth_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_path  # noqa: E402


@pytest.fixture(scope="module")
def encoded():
    """kind -> (state dict, hp, start_emb, enc_out) of the two G23 images through the oracle's encoder, once."""
    out = {}
    images = synth_images(2, seed=0)
    _, _, labels = captions_and_lengths()
    with torch.no_grad():
        for kind in R.KINDS:
            sd, hp = synthetic_sd(kind)
            out[kind] = (sd, hp) + tuple(ref_path._encode(kind, sd, images, labels[:2]))
    return out


# ---- 1. the restatement is the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_reproduces_g23_and_the_oracle_logits(kind, encoded):
    sd, hp, start, enc = encoded[kind]
    g = R.golden(kind)
    prompt = torch.from_numpy(g["prompt"])
    assert prompt.shape == (2, 5) and int(prompt.min()) > 3
    for name, weights in (("plain", sd), ("sharp", R.sharpened(sd))):
        with torch.no_grad():
            maps, logits = R.teacher_forced_maps(weights, start, enc, prompt, hp["pad_index"], hp["n_heads"], with_logits=True)
            want = ref_path.transformer_forward(weights, "decoder", prompt, enc, start, hp["pad_index"], hp["n_heads"])
        assert maps.shape == (2, 6, 49) and maps.dtype == torch.float64
        err = float((maps - torch.from_numpy(g[name]).double()).abs().max())
        lerr = float((logits - want.double()).abs().max())
        print(f"[g23 {kind} {name}] maps {err:.3e}, logits {lerr:.3e}")
        assert err <= 1e-6 and lerr <= 1e-4
    # the gain touches the last layer's energies only, so it moves the maps and leaves nothing in front of them changed
    assert float(np.abs(g["sharp"] - g["plain"]).max()) > 0.05


def test_restatement_positions_do_not_look_ahead(encoded):
    """Position ``c`` depends on ``tokens[:, :c]`` only: a longer teacher-forced row gives the same leading maps."""
    kind = R.KINDS[0]
    sd, hp, start, enc = encoded[kind]
    sd = R.sharpened(sd)
    prompt = torch.from_numpy(R.golden(kind)["prompt"])
    with torch.no_grad():
        full = R.teacher_forced_maps(sd, start, enc, prompt, hp["pad_index"], hp["n_heads"])
        short = R.teacher_forced_maps(sd, start, enc, prompt[:, :2], hp["pad_index"], hp["n_heads"])
    assert short.shape == (2, 3, 49) and float((full[:, :3] - short).abs().max()) < 1e-12
    assert float((full[:, 3] - full[:, 2]).abs().max()) > 1e-2           # ... and the positions differ from each other


# ---- 2. the committed fixtures -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_g23_files(kind):
    g = R.golden(kind)
    assert sorted(g.files) == ["gain", "n_images", "plain", "prompt", "sharp"] and float(g["gain"]) == R.GAIN
    for name in ("plain", "sharp"):
        a = g[name]
        assert a.shape == (2, 6, 49) and a.dtype == np.float32 and bool((a >= 0).all())
        assert float(np.abs(a.astype(np.float64).sum(-1) - 1).max()) <= 1e-6
    assert float(g["sharp"].max()) > 0.1 and float(g["plain"].max()) < 0.05


# ---- 3. check_return_attention -----------------------------------------------------------------------------------------------------
def test_check_return_attention_type():
    from deephumor_amd.models.beam import check_return_attention
    assert check_return_attention(False) is False and check_return_attention(True) is True
    for bad in (1, 0, None, "yes", torch.tensor(True), 1.0):
        with pytest.raises(TypeError, match="return_attention must be a bool"):
            check_return_attention(bad)


@pytest.mark.parametrize("kind", [k for k in KINDS if k not in R.KINDS])
def test_kinds_without_encoder_attention_refuse_before_any_device_work(kind, monkeypatch):
    """CPU models and CPU inputs: anything that reached the encoder or a kernel would raise RuntimeError (no CPU path); the
    refusal is a TypeError that names the reason.  ``return_attention=False`` on those kinds is the call without the keyword."""
    import deephumor_amd.models as M
    from deephumor_amd import hip
    from deephumor_amd.models.beam import check_return_attention
    _, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()
    monkeypatch.setattr(hip, "_launch", lambda *a, **k: pytest.fail("a kernel was launched"))
    images = synth_images(1, seed=0)
    args = (images, torch.tensor([[7, 8, 9]])) if "WithLabels" in kind else (images,)
    for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
        with pytest.raises(TypeError, match="no encoder attention"):
            call(*args, max_len=6, beam_size=2, top_k=5, return_attention=True)
        with pytest.raises(TypeError, match="must be a bool"):
            call(*args, max_len=6, beam_size=2, top_k=5, return_attention=1)
    with pytest.raises(TypeError, match="no encoder attention"):
        check_return_attention(True, model.decoder)
    kw = {"return_attention": False}
    assert model._check_prompts(None, None, 6, kw) is None and kw == {}


@pytest.mark.parametrize("kind", R.KINDS)
def test_cross_attention_kinds_refusals_on_the_cpu(kind):
    import deephumor_amd.models as M
    from deephumor_amd.models.beam import check_return_attention
    from deephumor_amd.pipeline import CaptionPipeline
    _, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()
    assert check_return_attention(True, model) is True and check_return_attention(True, model.decoder) is True
    kw = {"return_attention": True}
    model._check_prompts(None, None, 6, kw)
    assert kw == {"return_attention": True}
    with pytest.raises(TypeError, match="must be a bool"):
        model.generate_batch(*((synth_images(1, seed=0), torch.tensor([[7, 8, 9]])) if "WithLabels" in kind else (synth_images(1, seed=0),)),
                             return_attention="on")
    one = getattr(M, kind)(**dict(hp, pad_index=1)).eval()
    with pytest.raises(NotImplementedError, match="pad_index == 1"):
        check_return_attention(True, one)
    with pytest.raises(NotImplementedError, match="pad_index == 1"):
        one._check_prompts(None, None, 6, {"return_attention": True})
    with pytest.raises(NotImplementedError, match="^return_attention: "):      # (before the pipeline makes its streams)
        CaptionPipeline(model, return_attention=True)
    with pytest.raises(TypeError, match="must be a bool"):
        CaptionPipeline(model, return_attention=1)


def test_generate_sharded_refuses_maps():
    from deephumor_amd import dist
    from deephumor_amd.models.beam import BeamCaptions
    toks, lens, att = torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, dtype=torch.int64), torch.zeros(2, 4, 49)
    with pytest.raises(NotImplementedError, match="^return_attention: "):
        dist.generate_sharded(lambda lo, hi: (toks, lens, att), 2)
    beams = BeamCaptions(toks[:, None], lens[:, None], torch.zeros(2, 1), torch.zeros(2, 1, dtype=torch.int64), lens * 0, lens)
    with pytest.raises(NotImplementedError, match="^return_attention: "):
        dist.generate_sharded(lambda lo, hi: (beams, att[:, None]), 2)


# ---- 4. attention_to_heatmaps -------------------------------------------------------------------------------------------------------
def test_attention_to_heatmaps():
    from deephumor_amd import experiments
    from deephumor_amd.experiments import attention_to_heatmaps
    assert "attention_to_heatmaps" in experiments.__all__
    a = torch.from_numpy(R.golden(R.KINDS[0])["sharp"]).clone()          # [2, 6, 49]
    a[1, 4:] = 0.0
    h = attention_to_heatmaps(a)
    assert h.shape == (2, 6, 224, 224) and h.dtype == torch.float32
    area = h.double().sum((-1, -2)) * 49 / (224 * 224)                  # the map's mean over the image x the number of patches
    filled = torch.ones(2, 6, dtype=torch.bool)
    filled[1, 4:] = False
    assert float((area[filled] - 1).abs().max()) < 1e-4
    assert bool((h[1, 4:] == 0).all()) and bool((h[filled] >= 0).all())
    # the peak stays in the strongest patch's cell
    r, c = divmod(int(a[0, 3].argmax()), 7)
    pr, pc = divmod(int(h[0, 3].argmax()), 224)
    assert (pr // 32, pc // 32) == (r, c)
    # other sizes / leading shapes / the padded-key case (keys beyond the grid are dropped)
    wide = torch.cat([a, torch.zeros(2, 6, 15)], -1)[:, None]
    assert torch.equal(attention_to_heatmaps(wide, size=(56, 70)), attention_to_heatmaps(a, size=(56, 70))[:, None])
    assert attention_to_heatmaps(a[0, 0], size=(14, 14)).shape == (14, 14)
    with pytest.raises(ValueError):
        attention_to_heatmaps(a[..., :48])


# ---- 5. the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    """Three new symbols and no existing prototype or struct changed: the ABI version does not step (as for
    ``dh_beam_history_logits`` / ``dh_beam_constrain_logits``)."""
    from deephumor_amd import _abi, _build
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = ctypes.CDLL(_build.build())
    for name, nargs in (("dh_attn_cross_weights", 14), ("dh_beam_gather_attention", 13), ("dh_transformer_decode_position_attn", 20)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name + " is not declared in the header"
        args = [a.strip() for a in m.group(1).split(",")]
        sig = _abi.SIGNATURES[name]
        assert len(args) == len(sig) == nargs
        for a, t in zip(args, sig):
            if "dh_tr_" in a:
                continue
            want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
            assert t is want, (name, a, t)
        assert hasattr(lib, name)
    old, new = _abi.SIGNATURES["dh_transformer_decode_position"], _abi.SIGNATURES["dh_transformer_decode_position_attn"]
    assert new[:len(old) - 1] == old[:-1] and len(old) == 18
    assert [n for n, _ in _abi.TrModel._fields_][-2:] == ["cls_b_pad", "cls_w_x"]
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == _abi.ABI_VERSION == int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))


def test_new_entry_points_check_their_arguments():
    """Before any HIP call (nothing is dereferenced on the host): DH_ERR_BAD_ARG = 1, DH_ERR_UNSUPPORTED = 2."""
    from deephumor_amd import hip
    lib = hip.load()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    ok = dict(q=p, ldq=512, kv=p, keymask=p, out=p, n_img=1, rpi=1, mult=1, S=49, D=512, H=8, scale=8.0, dt=hip.BF16)

    def weights(**over):
        a = dict(ok, **over)
        return lib.dh_attn_cross_weights(a["q"], a["ldq"], a["kv"], a["keymask"], a["out"], a["n_img"], a["rpi"], a["mult"], a["S"],
                                         a["D"], a["H"], a["scale"], a["dt"], None)
    for over in (dict(q=None), dict(kv=None), dict(keymask=None), dict(out=None), dict(n_img=0), dict(rpi=0), dict(rpi=65), dict(mult=0),
                 dict(S=0), dict(H=0), dict(D=500), dict(D=32), dict(ldq=256), dict(ldq=516), dict(q=p + 2), dict(kv=p + 4), dict(scale=0.0)):
        assert weights(**over) == 1, over
    assert weights(S=8193) == 2 and weights(dt=hip.BF16_OUT_F32) == 2

    def gather(attn=p, src=p, src_ld=8, index=p, length=p, out=p, n=1, b=2, t=6, n_pos=7, rows=2, s=49):
        return lib.dh_beam_gather_attention(attn, src, src_ld, index, length, out, n, b, t, n_pos, rows, s, None)
    for over in (dict(attn=None), dict(src=None), dict(index=None), dict(length=None), dict(out=None), dict(n=0), dict(b=0), dict(b=65),
                 dict(t=0), dict(t=8), dict(src_ld=5), dict(s=0), dict(rows=1)):
        assert gather(**over) == 1, over
    sig = hip.SIGNATURES["dh_transformer_decode_position_attn"]
    assert lib.dh_transformer_decode_position_attn(*([None] * 4 + [0, None] + [0] * 6 + [None, None, 0, None, 0, None, 0, None])) == 1
    assert len(sig) == 20
