"""Records golden G25 (``tests/golden/g25_explain_<kind>.npz``): what the real reference computes for GIVEN captions and
``experiments.explain_captions`` must return -- the per-token log-probabilities of its teacher-forced logits and, for the two
kinds with encoder attention, the last decoder layer's head-mean attention maps.

Build-container only, like ``tools/make_bias_golden.py``, whose pattern this follows: it imports the real reference at run time and
commits nothing but arrays.  The models are the tiny ones of ``tests/explain_ref.HP`` on the synthetic weights of seed
``explain_ref.SEED`` (a pure function of seed, key and shape: the test builds the same weights), the inputs
``synth_images(3, seed=0)`` and ``explain_ref.captions()``: 7 captions of lengths 1 .. 9 over 3 templates.

Logits: ``model(images[index], captions[:, :-1], lengths)`` (trainer.py:69-73; the LSTM kinds get no lengths, as
``score_captions`` calls them), log-softmax and gather in fp64 on the reference's fp32 logits, position ``p`` predicting
``captions[:, p]``.  Maps: a forward pre-hook on ``decoder.layers[-1].enc_attn.dropout`` sees that layer's ``[bs, H, seq, seq]``
softmax (transformers.py:106-116), as ``tools/make_attention_golden.py`` does for G23; recorded are its head mean at positions
``0 .. L-1`` over the image's own 49 keys (the zero rows the reference pads the encoder output with carry weight exactly 0:
asserted).  Pad positions are recorded as computed; the tests mask them.

    python tools/make_explain_golden.py [kind ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as mg                                                   # noqa: E402  (puts the reference on sys.path)
from deephumor.models import (CaptioningLSTM, CaptioningLSTMWithLabels, CaptioningTransformer,      # noqa: E402
                              CaptioningTransformerBase)
from deephumor_amd.synth import load_synthetic, synth_images               # noqa: E402
import explain_ref as E                                                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CLASSES = {"CaptioningLSTM": CaptioningLSTM, "CaptioningLSTMWithLabels": CaptioningLSTMWithLabels,
           "CaptioningTransformerBase": CaptioningTransformerBase, "CaptioningTransformer": CaptioningTransformer,
           "CaptioningTransformerWithLabels": mg._WithLabelsTransformer}


def main():
    torch.set_num_threads(4)
    images = synth_images(E.N_TEMPLATES, seed=0)
    cap, lengths, index, labels = E.captions()
    for kind in (sys.argv[1:] or E.KINDS):
        model = load_synthetic(CLASSES[kind](**E.HP[kind]).eval(), seed=E.SEED)
        args = (images[index], cap[:, :-1], None)
        if "WithLabels" in kind:
            args = args + (labels[index],)
        seen = []
        handle = None
        if kind in E.CROSS_KINDS:
            handle = model.decoder.layers[-1].enc_attn.dropout.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
        with torch.no_grad():
            logits = model(*args)
        assert logits.shape[0] == cap.shape[0] and logits.shape[1] >= E.L and logits.shape[2] == E.V, tuple(logits.shape)
        lp = torch.log_softmax(logits[:, :E.L].double(), -1).gather(-1, cap.unsqueeze(-1)).squeeze(-1)
        fix = {"seed": np.int64(E.SEED), "captions": cap.numpy(), "lengths": lengths.numpy(), "template_index": index.numpy(),
               "labels": labels.numpy(), "logprobs": lp.numpy()}
        if handle is not None:
            handle.remove()
            assert len(seen) == 1 and seen[0].dim() == 4, [tuple(s.shape) for s in seen]
            att = seen[0]
            assert float((att.sum(-1) - 1).abs().max()) < 1e-5
            assert att.shape[-1] == E.N_KEYS or float(att[..., E.N_KEYS:].abs().max()) == 0.0
            fix["attention"] = att.mean(1)[:, :E.L, :E.N_KEYS].contiguous().numpy()
            print(kind, "largest weight", float(fix["attention"].max()))
        print(kind, "log-probs from", float(lp.min()), "to", float(lp.max()))
        np.savez_compressed(os.path.join(OUT, f"g25_explain_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
