"""Records golden G26 (``tests/golden/g26_pairs_<kind>.npz``): what the real reference computes for EVERY caption under EVERY
template and ``experiments.score_pairs`` must return -- per (caption, template) pair the log-probability of the caption (the sum of
the per-token log-probabilities of its teacher-forced logits) and its perplexity.

Build-container only, like ``tools/make_explain_golden.py``, whose method this follows line for line: it imports the real reference at
run time and commits nothing but arrays.  The models are the tiny ones of ``tests/explain_ref.HP`` on the synthetic weights of seed
``explain_ref.SEED``; the templates are ``synth_images(3, seed=0)`` plus a SECOND COPY of template 0 (4 templates: columns 0 and 3 of
the matrix must agree, and a stable ranking puts 0 first), the captions the 7 of ``explain_ref.captions()`` (lengths 1 .. 9); the label
models give the copy template 0's label.

Per template ``t``: ``model(images[t] repeated 7 times, captions[:, :-1], lengths)`` (trainer.py:69-73; the LSTM kinds get no lengths,
as ``score_captions`` calls them), log-softmax and gather in fp64 on the reference's fp32 logits, position ``p`` predicting
``captions[:, p]``; pads count 0.  ``logprob[i, t]`` is the fp64 sum over the caption's positions, ``perplexity[i, t]`` is
``exp(-logprob[i, t] / lengths[i])`` (deephumor/experiments/metrics.py:4-9, per sequence).

    python tools/make_pairs_golden.py [kind ...]
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
TEMPLATES = (0, 1, 2, 0)                                                   # rows of synth_images(3): the fourth template is a copy of the first


def main():
    torch.set_num_threads(4)
    base = synth_images(E.N_TEMPLATES, seed=0)
    cap, lengths, _, base_labels = E.captions()
    pick = torch.tensor(TEMPLATES)
    images, labels = base[pick], base_labels[pick]
    n = cap.shape[0]
    for kind in (sys.argv[1:] or E.KINDS):
        model = load_synthetic(CLASSES[kind](**E.HP[kind]).eval(), seed=E.SEED)
        logprob = np.zeros((n, len(TEMPLATES)), dtype=np.float64)
        for t in range(len(TEMPLATES)):
            args = (images[t:t + 1].expand(n, -1, -1, -1), cap[:, :-1], None)
            if "WithLabels" in kind:
                args = args + (labels[t:t + 1].expand(n, -1),)
            with torch.no_grad():
                logits = model(*args)
            assert logits.shape[0] == n and logits.shape[1] >= E.L and logits.shape[2] == E.V, tuple(logits.shape)
            lp = torch.log_softmax(logits[:, :E.L].double(), -1).gather(-1, cap.unsqueeze(-1)).squeeze(-1)
            logprob[:, t] = lp.masked_fill(cap == E.PAD, 0.0).sum(-1).numpy()
        perplexity = np.exp(-logprob / lengths.numpy()[:, None].astype(np.float64))
        fix = {"seed": np.int64(E.SEED), "captions": cap.numpy(), "lengths": lengths.numpy(), "templates": np.asarray(TEMPLATES, dtype=np.int64),
               "labels": labels.numpy(), "logprob": logprob, "perplexity": perplexity}
        print(kind, "pair log-probs from", float(logprob.min()), "to", float(logprob.max()),
              "| copy column apart by", float(np.abs(logprob[:, 0] - logprob[:, 3]).max()))
        np.savez_compressed(os.path.join(OUT, f"g26_pairs_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
