"""Records golden G28 (``tests/golden/g28_alternatives_<kind>.npz``): what the real reference's teacher-forced ``forward`` ranks
first at every position of GIVEN captions, and what ``experiments.token_alternatives`` must therefore return.

Build-container only, like ``tools/make_explain_golden.py``, whose pattern this follows: it imports the real reference at run time and
commits nothing but arrays.  The models are the tiny ones of ``tests/explain_ref.HP`` on synthetic weights (a pure function of seed,
key and shape: the test builds the same weights from the stored seed), the inputs are G27's (``alternatives_ref.g28_inputs``): 4
templates, the fourth a second copy of the first, x 3 captions of 7 positions.

Per position ``p`` (predicting ``captions[:, p]``) of the reference's fp32 logits: ``tokens`` -- the ids of the 8 largest logits,
largest first, equal logits to the lower id --, ``logprobs`` -- their log-softmax, taken in fp64 and stored as fp32 --, and ``gaps`` --
the logit gap between each of ranks 0 .. 7 and the next rank below it.  An id is only comparable where its gap exceeds 2e-3, twice the
1e-3 fp32 logits tolerance the project is judged by; the tool asserts that at least 90 % of the (non-pad position, rank) entries are,
and picks the weights' seed -- the first from ``explain_ref.SEED`` upwards -- so that the reference alone satisfies it.  Pad positions
are recorded as computed; the tests mask them.

    python tools/make_alternatives_golden.py [kind ...]
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
import alternatives_ref as A                                               # noqa: E402
import explain_ref as E                                                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CLASSES = {"CaptioningLSTM": CaptioningLSTM, "CaptioningLSTMWithLabels": CaptioningLSTMWithLabels,
           "CaptioningTransformerBase": CaptioningTransformerBase, "CaptioningTransformer": CaptioningTransformer,
           "CaptioningTransformerWithLabels": mg._WithLabelsTransformer}
MAX_SEEDS = 20


def record(kind, seed, images, cap, lengths, index, labels):
    model = load_synthetic(CLASSES[kind](**E.HP[kind]).eval(), seed=seed)
    args = (images[index], cap[:, :-1], None)
    if "WithLabels" in kind:
        args = args + (labels[index],)
    with torch.no_grad():
        logits = model(*args)
    l = cap.shape[1]
    assert logits.shape[0] == cap.shape[0] and logits.shape[1] >= l and logits.shape[2] == E.V and logits.dtype == torch.float32
    logits = logits[:, :l]
    order = torch.sort(logits, dim=-1, descending=True, stable=True)
    top = order.indices[..., :A.G28_TOP]
    gaps = order.values[..., :A.G28_TOP] - order.values[..., 1:A.G28_TOP + 1]
    lp = torch.log_softmax(logits.double(), -1).gather(-1, top).float()
    return {"seed": np.int64(seed), "captions": cap.numpy(), "lengths": lengths.numpy(), "template_index": index.numpy(),
            "labels": labels.numpy(), "tokens": top.numpy(), "logprobs": lp.numpy(), "gaps": gaps.numpy()}


def main():
    torch.set_num_threads(4)
    images, cap, lengths, index, labels = A.g28_inputs(synth_images(3, seed=0))
    for kind in (sys.argv[1:] or E.KINDS):
        for seed in range(E.SEED, E.SEED + MAX_SEEDS):
            fix = record(kind, seed, images, cap, lengths, index, labels)
            share = A.gap_share(fix)
            print(f"{kind} seed {seed}: {share:.3f} of the entries have a gap above {A.GAP}; log-probs from "
                  f"{float(fix['logprobs'].min()):.3f} to {float(fix['logprobs'].max()):.3f}")
            if share >= A.GAP_SHARE:
                break
        assert share >= A.GAP_SHARE, f"{kind}: no seed in {MAX_SEEDS} gives {A.GAP_SHARE:.0%} of the entries a gap above {A.GAP}"
        np.savez_compressed(os.path.join(OUT, f"g28_alternatives_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
