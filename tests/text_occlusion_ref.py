"""What the ``text_occlusion`` tests share (test_text_occlusion_cpu.py, test_text_occlusion_gpu.py): the variant builder stated
independently of the product, a torch-CPU fp32 restatement of both levels that shares no code with the product, the inputs of golden
G29 (``tests/golden/g29_text_occlusion_<kind>.npz``, recorded from the real reference by ``tools/make_text_occlusion_golden.py``), the
margin helpers and the measured values.  Plain module, no GPU use.

The inputs are ``occlusion_ref.inputs``: 4 templates (the fourth a copy of the first), 3 captions of 7 positions with lengths 7, 4 and
2, every caption under every template = 12 rows, labels ``[4, 3]``.

The restatement, by definition:
  ``history_inputs``   caption ``i`` has one real region per column ``j <= lengths[i] - 2``; variant ``(i, j)`` is ``captions[i, :-1]``
                       with column ``j`` replaced by the fill id -- built with python loops, caption-major, base first;
  ``label_rows``       the label row, then one copy per column with that column replaced by the fill id;
  ``history_level``    ``oracle.ref_path``'s decoder on the base and the variants of one caption, fp64 log-softmax and gather against the
                       ORIGINAL targets, the row rounded to fp32 (what the product's kernels hand back); then, with ``m[p] = 1`` for
                       ``j < p < lengths[i]``: ``token_drop = float32(float64(b) - float64(v))`` where ``m``, ``drop = float32(sum64(b m) -
                       sum64(v m))``, ``base = float32(sum64(b))``;
  ``label_level``      the trunk once per distinct template, ``ref_path``'s label mean and combine for the ``l + 1`` label rows, the
                       decoder on every variant; ``OcclusionScores``' definitions over all positions;
  ``real_mask``        bool ``[n, R]``: which (caption, region) entries are real."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import explain_ref as E
import occlusion_ref as O
from oracle import ref_path as R

GOLDEN = E.GOLDEN
L = O.L
UNK = 1
FILLS = (("pad", E.PAD), ("unk", UNK))     # (name in G29, token id)
LABEL_KINDS = ("CaptioningLSTMWithLabels", "CaptioningTransformerWithLabels")
inputs = O.inputs


def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g29_text_occlusion_{kind}.npz"))


# ---- the variants -------------------------------------------------------------------------------------------------------------------
def history_inputs(cap, lengths, fill_id):
    """-> (caption [N], region [N] (-1: the base), inputs int64 [N, L - 1]) as python-built tensors, caption-major."""
    caption, region, rows = [], [], []
    for i in range(cap.shape[0]):
        row = [int(t) for t in cap[i, :-1]]
        caption.append(i), region.append(-1), rows.append(list(row))
        for j in range(int(lengths[i]) - 1):                                 # the tokens in front of <eos>
            edited = list(row)
            edited[j] = int(fill_id)
            caption.append(i), region.append(j), rows.append(edited)
    return torch.tensor(caption), torch.tensor(region), torch.tensor(rows, dtype=torch.int64)


def label_rows(row, fill_id):
    row = [int(t) for t in row]
    out = [list(row)]
    for k in range(len(row)):
        edited = list(row)
        edited[k] = int(fill_id)
        out.append(edited)
    return torch.tensor(out, dtype=torch.int64)


def real_mask(lengths, n_regions):
    return torch.tensor([[j <= int(n) - 2 for j in range(n_regions)] for n in lengths])


# ---- the two levels -----------------------------------------------------------------------------------------------------------------
def _decode(kind, sd, n_heads, start, enc, x, pad_index):
    if "LSTM" in kind:
        return R.lstm_decoder_forward(sd, "decoder", start, x, None)
    return R.transformer_forward(sd, "decoder", x, enc, start, pad_index, n_heads)


def encode3(kind, sd, images, labels):
    """``ref_path``'s encoder on the three distinct templates, indexed out to the four -> (start [4, D], enc [4, S, D] or None)."""
    pick = torch.tensor(O.TEMPLATES)
    with torch.no_grad():
        start, enc = R._encode(kind, sd, images[:3], labels[:3] if "WithLabels" in kind else None)
    return start[pick], None if enc is None else enc[pick]


def history_rows(kind, sd, n_heads, start, enc, cap, lengths, index, fill_id, pad_index=E.PAD):
    """-> (caption [N], region [N], rows fp32 [N, L]): the per-token rows of every sequence against its original caption."""
    caption, region, x = history_inputs(cap, lengths, fill_id)
    rows = torch.zeros((x.shape[0], cap.shape[1]), dtype=torch.float32)
    with torch.no_grad():
        for i in range(cap.shape[0]):
            mine = (caption == i).nonzero().squeeze(1)
            t = int(index[i])
            k = mine.shape[0]
            logits = _decode(kind, sd, n_heads, start[t:t + 1].repeat(k, 1), None if enc is None else enc[t:t + 1].repeat(k, 1, 1), x[mine], pad_index)
            rows[mine] = E.token_logprobs(logits, cap[i:i + 1].repeat(k, 1), pad_index).float()
    return caption, region, rows


def history_scores(caption, region, rows, lengths):
    """The definitions on the fp32 rows -> (base fp32 [n], drop fp32 [n, L - 1], token_drop fp32 [n, L, L - 1])."""
    n, l = int(caption.max()) + 1, rows.shape[1]
    base = torch.zeros(n, dtype=torch.float32)
    drop = torch.zeros((n, l - 1), dtype=torch.float32)
    tokens = torch.zeros((n, l, l - 1), dtype=torch.float32)
    where = {(int(c), int(r)): k for k, (c, r) in enumerate(zip(caption, region))}
    for i in range(n):
        b = rows[where[(i, -1)]].double()
        base[i] = b.sum().float()
        for j in range(int(lengths[i]) - 1):
            v = rows[where[(i, j)]].double()
            m = torch.tensor([1.0 if j < p < int(lengths[i]) else 0.0 for p in range(l)], dtype=torch.float64)
            drop[i, j] = ((b * m).sum() - (v * m).sum()).float()
            for p in range(j + 1, int(lengths[i])):
                tokens[i, p, j] = (b[p] - v[p]).float()
    return base, drop, tokens


def history_level(kind, sd, n_heads, images, labels, cap, lengths, index, fill_id, pad_index=E.PAD, encoded=None):
    start, enc = encoded if encoded is not None else encode3(kind, sd, images, labels)
    caption, region, rows = history_rows(kind, sd, n_heads, start, enc, cap, lengths, index, fill_id, pad_index)
    return history_scores(caption, region, rows, lengths)


def label_level(kind, sd, n_heads, images, labels, cap, index, fill_id, pad_index=E.PAD):
    """-> (base fp32 [n], drop fp32 [n, l], token_drop fp32 [n, L, l]); ``images`` / ``labels``: the four templates."""
    assert kind in LABEL_KINDS
    spatial = "Transformer" in kind
    n, l = cap.shape[0], labels.shape[1]
    with torch.no_grad():
        out = R.image_encoder(sd, "encoder.image_encoder", images[:3], spatial)
        emb, enc = out if spatial else (out, None)
        pick = torch.tensor(O.TEMPLATES)
        emb, enc = emb[pick], None if enc is None else enc[pick]
        rows = torch.zeros((n, 1 + l, cap.shape[1]), dtype=torch.float32)
        for i in range(n):
            t = int(index[i])
            variants = label_rows(labels[t], fill_id)
            both = torch.cat([emb[t:t + 1].repeat(1 + l, 1), R.label_encoder(sd, "encoder.label_encoder", variants)], dim=1)
            start = F.linear(both, sd["encoder.linear.weight"], sd["encoder.linear.bias"])
            logits = _decode(kind, sd, n_heads, start, None if enc is None else enc[t:t + 1].repeat(1 + l, 1, 1), cap[i:i + 1, :-1].repeat(1 + l, 1), pad_index)
            rows[i] = E.token_logprobs(logits, cap[i:i + 1].repeat(1 + l, 1), pad_index).float()
    sums = rows.sum(-1, dtype=torch.float64)
    return sums[:, 0].float(), (sums[:, :1] - sums[:, 1:]).float(), (rows[:, :1].double() - rows[:, 1:].double()).float().transpose(1, 2)


# ---- margins ------------------------------------------------------------------------------------------------------------------------
def passing(drop, real, tol):
    """bool like ``drop``: the real entries whose ``|drop|`` in the reference exceeds ``2 * tol`` -- only there is a sign compared."""
    return np.asarray(real) & (np.abs(np.asarray(drop, dtype=np.float64)) > 2 * tol)


def share_passing(drop, real, tol):
    return float(passing(drop, real, tol).sum()) / float(np.asarray(real).sum())


def top_gaps(drop, real):
    """Per caption the distance between its largest drop and the runner-up among its real regions (inf with fewer than two)."""
    d = np.where(np.asarray(real), np.asarray(drop, dtype=np.float64), -np.inf)
    s = np.sort(d, axis=1)
    gap = s[:, -1] - s[:, -2] if d.shape[1] > 1 else np.full(d.shape[0], np.inf)
    return np.where(np.isfinite(gap), gap, np.inf)


# ---- gates --------------------------------------------------------------------------------------------------------------------------
CEILING = L * 2e-3                         # twice the contract's 1e-3 logit parity per token, L tokens (occlusion_ref.CEILING)
# (|base - want|, |drop - want|, |token_drop - want|) seen on an MI355X per (kind, level, fill name, want), want = golden G29 or the
# restatement above on the model's own weights: the fp32 product, the worst over both settings of f32_split -- measured against the
# reference, never against the product (the tests print what they see; profiles/text_occlusion/errors.txt).  test_text_occlusion_gpu.py
# gates fp32 at 1.25 x these and at CEILING.  The 16-bit types print what they measure: their weights are rounded, their binding check
# is the bit equalities.  The base log-probs reach -78 (an fp32 ulp there is 7.6e-6) and sum up to 7 tokens.
_L, _LL, _B, _T, _TL = E.KINDS
WORST = {
    (_L, "history", "pad", "g29"): (2.573e-05, 2.636e-05, 1.354e-05),
    (_L, "history", "pad", "restatement"): (2.289e-05, 3.242e-05, 1.431e-05),
    (_L, "history", "unk", "g29"): (2.573e-05, 4.347e-05, 1.677e-05),
    (_L, "history", "unk", "restatement"): (2.289e-05, 3.624e-05, 1.812e-05),
    (_LL, "history", "pad", "g29"): (8.860e-06, 1.496e-05, 8.599e-06),
    (_LL, "history", "pad", "restatement"): (1.907e-05, 1.407e-05, 1.335e-05),
    (_LL, "history", "unk", "g29"): (8.860e-06, 1.347e-05, 9.227e-06),
    (_LL, "history", "unk", "restatement"): (1.907e-05, 1.287e-05, 1.287e-05),
    (_LL, "label", "unk", "g29"): (8.860e-06, 9.759e-06, 1.037e-05),
    (_LL, "label", "unk", "restatement"): (1.144e-05, 9.537e-06, 8.583e-06),
    (_T, "history", "pad", "g29"): (7.850e-06, 7.301e-06, 5.953e-06),
    (_T, "history", "pad", "restatement"): (7.629e-06, 5.722e-06, 4.768e-06),
    (_T, "history", "unk", "g29"): (7.850e-06, 5.514e-06, 3.987e-06),
    (_T, "history", "unk", "restatement"): (7.629e-06, 7.629e-06, 4.768e-06),
    (_B, "history", "pad", "g29"): (5.890e-06, 8.094e-06, 6.709e-06),
    (_B, "history", "pad", "restatement"): (7.629e-06, 9.060e-06, 4.768e-06),
    (_B, "history", "unk", "g29"): (5.890e-06, 8.018e-06, 6.505e-06),
    (_B, "history", "unk", "restatement"): (7.629e-06, 1.144e-05, 6.199e-06),
    (_TL, "history", "pad", "g29"): (1.133e-05, 8.565e-06, 4.495e-06),
    (_TL, "history", "pad", "restatement"): (7.629e-06, 7.629e-06, 4.292e-06),
    (_TL, "history", "unk", "g29"): (1.133e-05, 7.677e-06, 3.650e-06),
    (_TL, "history", "unk", "restatement"): (7.629e-06, 9.537e-06, 4.292e-06),
    (_TL, "label", "unk", "g29"): (1.133e-05, 8.567e-06, 6.490e-06),
    (_TL, "label", "unk", "restatement"): (7.629e-06, 8.583e-06, 4.768e-06),
}
WORST_16 = {                               # against G29: (kind, level, fill name) -> {type: (base, drop, token_drop)}
    (_L, "history", "pad"): {"f16": (8.903e-03, 3.326e-02, 1.767e-02), "bf16": (7.408e-02, 1.142e-01, 9.681e-02)},
    (_L, "history", "unk"): {"f16": (8.903e-03, 2.196e-02, 1.696e-02), "bf16": (7.408e-02, 1.179e-01, 8.320e-02)},
    (_LL, "history", "pad"): {"f16": (1.201e-02, 1.703e-02, 1.210e-02), "bf16": (9.497e-02, 1.144e-01, 8.424e-02)},
    (_LL, "history", "unk"): {"f16": (1.201e-02, 2.267e-02, 1.478e-02), "bf16": (9.497e-02, 8.975e-02, 7.084e-02)},
    (_LL, "label", "unk"): {"f16": (1.201e-02, 8.666e-03, 7.983e-03), "bf16": (9.497e-02, 1.132e-01, 5.323e-02)},
    (_T, "history", "pad"): {"f16": (1.347e-02, 8.539e-03, 7.129e-03), "bf16": (9.775e-02, 6.461e-02, 6.005e-02)},
    (_T, "history", "unk"): {"f16": (1.347e-02, 1.074e-02, 1.074e-02), "bf16": (9.775e-02, 7.565e-02, 4.636e-02)},
    (_B, "history", "pad"): {"f16": (8.552e-03, 6.853e-03, 5.712e-03), "bf16": (1.072e-01, 6.440e-02, 5.037e-02)},
    (_B, "history", "unk"): {"f16": (8.552e-03, 8.846e-03, 5.950e-03), "bf16": (1.072e-01, 7.678e-02, 4.739e-02)},
    (_TL, "history", "pad"): {"f16": (4.057e-03, 4.745e-03, 4.332e-03), "bf16": (5.145e-02, 5.411e-02, 5.411e-02)},
    (_TL, "history", "unk"): {"f16": (4.057e-03, 7.725e-03, 7.725e-03), "bf16": (5.145e-02, 5.258e-02, 5.208e-02)},
    (_TL, "label", "unk"): {"f16": (4.057e-03, 9.704e-03, 5.298e-03), "bf16": (5.145e-02, 3.912e-02, 2.731e-02)},
}
gate = lambda worst: 1.25 * worst          # noqa: E731
