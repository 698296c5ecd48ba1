"""Records golden G29 (``tests/golden/g29_text_occlusion_<kind>.npz``): what the real reference computes when one word of the decoder's
input -- or one word of the template's label -- is replaced, and ``experiments.text_occlusion`` must return: per caption its
log-probability (``base``), per region how much of it is lost (``drop``) and the same per token (``tokens``).

Build-container only, like ``tools/make_occlusion_golden.py``, whose method this follows: it imports the real reference at run time and
commits nothing but arrays.  The models are the tiny ones of ``tests/explain_ref.HP`` on the synthetic weights of seed
``explain_ref.SEED``; the inputs are ``tests/occlusion_ref.inputs``: ``synth_images(3, seed=0)`` plus a second copy of template 0, the
three captions of 7 positions (lengths 7, 4, 2), every caption under every template -- 12 rows.

  history level, all five kinds, ``fill="pad"`` (id 0) and ``fill=1`` (``<unk>``): the reference's own encoder once on the three
  distinct templates, then ``model.decoder`` on ``caption[:-1]`` and on its copies with column ``j`` replaced, ``j`` in front of the
  caption's ``<eos>`` (``text_occlusion_ref.history_inputs``).  ``hist_<fill>_drop [12, 6]``, ``hist_<fill>_tokens [12, 7, 6]``: zero
  where the region is not real and at positions ``p <= j``;
  label level, the two label kinds, ``fill=1``: the reference's FULL encoder on the template repeated ``l + 1`` times with the label
  rows of ``text_occlusion_ref.label_rows``, then the decoder on ``caption[:-1]``.  ``label_base [12]``, ``label_drop [12, 3]``,
  ``label_tokens [12, 7, 3]``.

Log-softmax and gather in fp64 on the reference's fp32 logits against the ORIGINAL targets, position ``p`` predicting ``captions[:, p]``;
pads count 0; sums and differences in fp64, not rounded.

    python tools/make_text_occlusion_golden.py [kind ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as mg                                                   # noqa: E402  (puts the reference on sys.path)
from deephumor.models import (CaptioningLSTM, CaptioningLSTMWithLabels, CaptioningTransformer,      # noqa: E402
                              CaptioningTransformerBase)
from deephumor_amd.synth import load_synthetic, synth_images               # noqa: E402
import explain_ref as E                                                    # noqa: E402
import occlusion_ref as O                                                  # noqa: E402
import text_occlusion_ref as T                                             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CLASSES = {"CaptioningLSTM": CaptioningLSTM, "CaptioningLSTMWithLabels": CaptioningLSTMWithLabels,
           "CaptioningTransformerBase": CaptioningTransformerBase, "CaptioningTransformer": CaptioningTransformer,
           "CaptioningTransformerWithLabels": mg._WithLabelsTransformer}


def rows64(logits, cap):
    lp = torch.log_softmax(logits[:, :O.L].double(), -1).gather(-1, cap.unsqueeze(-1)).squeeze(-1)
    return lp.masked_fill(cap == E.PAD, 0.0)


def encode(model, kind, images, labels):
    """The reference's encoder -> (start, spatial or None)."""
    if kind == "CaptioningTransformerWithLabels":
        return model._start(images, labels)
    if kind == "CaptioningLSTMWithLabels":
        return model.encoder(images=images, labels=labels), None
    out = model.encoder(images)
    return out if isinstance(out, tuple) else (out, None)


def decode(model, kind, start, spatial, x):
    if "LSTM" in kind:
        return model.decoder(start, x, None)
    if spatial is None:
        return model.decoder(x, start_emb=start)
    return model.decoder(x, enc_out=spatial, start_emb=start)


def main():
    torch.set_num_threads(4)
    images, cap, lengths, index, labels = O.inputs(synth_images(E.N_TEMPLATES, seed=0))
    n = cap.shape[0]
    pick = torch.tensor(O.TEMPLATES)
    real = T.real_mask(lengths, O.L - 1).numpy()
    for kind in (sys.argv[1:] or E.KINDS):
        model = load_synthetic(CLASSES[kind](**E.HP[kind]).eval(), seed=E.SEED)
        fix = {"seed": np.int64(E.SEED), "captions": cap.numpy(), "lengths": lengths.numpy(), "template_index": index.numpy(),
               "templates": np.asarray(O.TEMPLATES, dtype=np.int64), "labels": labels.numpy()}
        with torch.no_grad():
            start3, spatial3 = encode(model, kind, images[:3], labels[:3])
        start, spatial = start3[pick], None if spatial3 is None else spatial3[pick]
        for name, fill_id in T.FILLS:
            caption, region, x = T.history_inputs(cap, lengths, fill_id)
            base = np.zeros(n)
            drop = np.zeros((n, O.L - 1))
            tokens = np.zeros((n, O.L, O.L - 1))
            for i in range(n):
                mine = (caption == i).nonzero().squeeze(1)
                t, k = int(index[i]), mine.shape[0]
                with torch.no_grad():
                    logits = decode(model, kind, start[t:t + 1].expand(k, -1), None if spatial is None else spatial[t:t + 1].expand(k, -1, -1), x[mine])
                assert logits.shape[0] == k and logits.shape[1] >= O.L and logits.shape[2] == E.V, tuple(logits.shape)
                rows = rows64(logits, cap[i:i + 1].expand(k, -1)).numpy()
                assert int(region[mine[0]]) == -1
                base[i] = rows[0].sum()
                for q in range(1, k):
                    j = int(region[mine[q]])
                    m = np.array([1.0 if j < p < int(lengths[i]) else 0.0 for p in range(O.L)])
                    drop[i, j] = (rows[0] * m).sum() - (rows[q] * m).sum()
                    tokens[i, :, j] = (rows[0] - rows[q]) * m
                    assert np.array_equal(rows[q][:j + 1], rows[0][:j + 1]), (kind, name, i, j)     # the reference is causal
            if "base" in fix:
                assert np.array_equal(fix["base"], base)
            fix["base"], fix[f"hist_{name}_drop"], fix[f"hist_{name}_tokens"] = base, drop, tokens
            d = np.abs(drop[real])
            print(kind, f"history fill={name}: base from", float(base.min()), "to", float(base.max()), "| real |drop| from", float(d.min()),
                  "to", float(d.max()), "median", float(np.median(d)))
        if kind in T.LABEL_KINDS:
            l = labels.shape[1]
            rows = np.zeros((n, 1 + l, O.L))
            for t in sorted(set(O.TEMPLATES)):
                variants = T.label_rows(labels[t], T.UNK)
                with torch.no_grad():
                    st, sp = encode(model, kind, images[t:t + 1].expand(1 + l, -1, -1, -1), variants)
                for i in range(n):
                    if O.TEMPLATES[int(index[i])] != t:
                        continue
                    with torch.no_grad():
                        logits = decode(model, kind, st, sp, cap[i:i + 1, :-1].expand(1 + l, -1))
                    rows[i] = rows64(logits, cap[i:i + 1].expand(1 + l, -1)).numpy()
            sums = rows.sum(-1)
            fix["label_base"], fix["label_drop"] = sums[:, 0], sums[:, :1] - sums[:, 1:]
            fix["label_tokens"] = (rows[:, :1] - rows[:, 1:]).transpose(0, 2, 1)
            d = np.abs(fix["label_drop"])
            print(kind, "label fill=unk: base apart from the history level's by", float(np.abs(fix["label_base"] - fix["base"]).max()),
                  "| |drop| from", float(d.min()), "to", float(d.max()), "median", float(np.median(d)))
        np.savez_compressed(os.path.join(OUT, f"g29_text_occlusion_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
