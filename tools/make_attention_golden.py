"""Records golden G23 (``tests/golden/g23_attention_<kind>.npz``): the attention weights the reference computes and throws away
(``MultiHeadAttentionLayer.forward``, transformers.py:106-120) -- what ``generate_batch(..., return_attention=True)`` must return
on the columns of a prompt.

Build-container only, like ``tools/make_constraints_golden.py``, whose pattern this follows: it imports the real reference and
commits nothing but arrays.  A forward pre-hook on ``model.decoder.layers[-1].enc_attn.dropout`` sees that layer's
``[bs, H, seq, seq]`` softmax (the dropout's input, :115-116).  The teacher-forced ``forward`` runs on ``synth_images(2, seed=0)``
and a 2 x 5 prompt without pad tokens; recorded are the image's own 49 keys (the reference pads ``enc_out`` with masked zero rows
up to ``seq``; here ``seq`` is 49 anyway), the mean over the heads, and positions ``0 .. 5`` -- the image slot and the five
prompt tokens, i.e. the positions whose logits decide token columns ``0 .. 5``.

Two settings per kind: the synthetic weights as they are (``plain``: almost flat maps, largest weight ~0.03), and ``sharp``: the
last layer's ``enc_attn.fc_q`` weight and bias multiplied by 8 (``tests/attention_maps_ref.sharpened``), where maps of different
rows or positions are far enough apart for a test to tell them from each other.

    python tools/make_attention_golden.py [kind ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as mg                                                   # noqa: E402  (puts the reference on sys.path)
from deephumor_amd.synth import synth_images                               # noqa: E402
from attention_maps_ref import GAIN, KINDS, N_KEYS, sharpened              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N_IMG, PROMPT_LEN = 2, 5


def maps_of(model, args):
    """Head-mean softmax of the last layer's encoder attention at positions 0 .. PROMPT_LEN over the image's keys [N, P + 1, 49]."""
    seen = []
    handle = model.decoder.layers[-1].enc_attn.dropout.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
    try:
        with torch.no_grad():
            model(*args)
    finally:
        handle.remove()
    assert len(seen) == 1 and seen[0].dim() == 4, [tuple(s.shape) for s in seen]
    att = seen[0]                                                          # [bs, H, seq, seq]
    rows = att.sum(-1)
    assert float((rows - 1).abs().max()) < 1e-5
    assert float(att[..., N_KEYS:].abs().max()) == 0.0 if att.shape[-1] > N_KEYS else True      # no weight on the padded rows
    return att.mean(1)[:, :PROMPT_LEN + 1, :N_KEYS].contiguous()


def main():
    torch.set_num_threads(4)
    images = synth_images(N_IMG, seed=0)
    cap, _, labels = mg.captions_and_lengths(mg.V_SMALL)
    prompt = cap[:N_IMG, :PROMPT_LEN].contiguous()
    assert int(prompt.min()) > 3                                           # no pad / special tokens
    for kind in (sys.argv[1:] or KINDS):
        model = mg.build(kind, mg.V_SMALL)
        args = (images, prompt, None, labels[:N_IMG]) if "WithLabels" in kind else (images, prompt)
        fix = {"prompt": prompt.numpy(), "gain": np.float64(GAIN), "n_images": np.int64(N_IMG)}
        fix["plain"] = maps_of(model, args).numpy()
        model.load_state_dict(sharpened(model.state_dict()))
        fix["sharp"] = maps_of(model, args).numpy()
        for k in ("plain", "sharp"):
            assert fix[k].shape == (N_IMG, PROMPT_LEN + 1, N_KEYS) and fix[k].dtype == np.float32
            print(kind, k, "largest weight", float(fix[k].max()), "rows sum to 1 within", float(np.abs(fix[k].sum(-1) - 1).max()))
        np.savez_compressed(os.path.join(OUT, f"g23_attention_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
