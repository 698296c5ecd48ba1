"""Records ``tests/golden/g19_prompted.npz`` from the REAL reference on the CPU: the greedy caption of 8 images under 8 prompts of
different lengths (``[0, 1, 3, 3, 7, 12, 5, 0]``), for the five model kinds on the synthetic weights every other fixture uses.

    python tools/make_prompted_golden.py --reference /path/to/deephumor-checkout

The reference is imported by path with the stand-in torchvision of ``oracle/_standin``, as ``oracle/make_golden.py`` does (whose
model builders and logit tap are reused).  Only data is written: token ids, lengths, the prompts, the labels and the per-step top-2
logit margins.  The prompt seed is the first of ``range(20)`` for which the smallest margin over all kinds, images and steps is at
least 1e-3 -- the project's fp32 logit bar, below which an arg-max flip on the GPU would be allowed rather than a bug; if none
qualifies the best one is recorded, with its margin, and the script says so."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 3, 3, 7, 12, 5, 0]
V, MAX_LEN, BAR = 1000, 32, 1e-3
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")


def inputs(seed):
    g = np.random.Generator(np.random.Philox(key=[1234, 1900 + seed]))
    prompts = torch.from_numpy(g.integers(6, V, size=(len(LENGTHS), max(LENGTHS))).astype(np.int64))
    labels = torch.from_numpy(g.integers(6, V, size=(len(LENGTHS), 3)).astype(np.int64))
    return prompts, labels


def record(G, models, images, seed):
    prompts, labels = inputs(seed)
    rec = dict(prompts=prompts.numpy(), lengths=np.array(LENGTHS, np.int64), labels=labels.numpy(), seed=np.array([seed]))
    worst = float("inf")
    for kind in KINDS:
        for i, n in enumerate(LENGTHS):
            cap = prompts[i:i + 1, :n] if n else None
            lab = labels[i:i + 1] if "WithLabels" in kind else None
            ids, margins, _ = G.greedy_with_margins(models[kind], kind, images[i:i + 1], lab, cap, max_len=MAX_LEN)
            rec[f"{kind}_ids_{i}"], rec[f"{kind}_margins_{i}"] = ids.astype(np.int64), margins
            worst = min(worst, float(margins.min()))
    rec["min_margin"] = np.array([worst], np.float32)
    return rec, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DEEPHUMOR_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--seeds", type=int, default=20)
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or DEEPHUMOR_REFERENCE) is required")
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_standin"))
    sys.path.insert(0, args.reference)
    sys.path.insert(0, ROOT)
    from oracle import make_golden as G
    from deephumor_amd.synth import synth_images
    torch.manual_seed(0)
    images = synth_images(len(LENGTHS), seed=0)
    models = {kind: G.build(kind, V) for kind in KINDS}
    best = None
    for seed in range(args.seeds):
        rec, worst = record(G, models, images, seed)
        print(f"seed {seed}: smallest top-2 margin {worst:.6f}", flush=True)
        if best is None or worst > best[1]:
            best = (rec, worst)
        if worst >= BAR:
            break
    rec, worst = best
    if worst < BAR:
        print(f"no seed of the first {args.seeds} clears {BAR}: recording the best one (seed {int(rec['seed'][0])}, margin {worst:.6f})")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g19_prompted.npz"), **rec)
    print("wrote g19_prompted.npz: seed", int(rec["seed"][0]), "min margin", worst)


if __name__ == "__main__":
    main()
