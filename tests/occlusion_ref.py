"""What the ``occlusion_maps`` tests share (test_occlusion_cpu.py, test_occlusion_gpu.py): a torch-CPU restatement that shares no
code with the product, the inputs of golden G27 (``tests/golden/g27_occlusion_<kind>.npz``, recorded from the real reference by
``tools/make_occlusion_golden.py``) and the measured values.  Plain module, no GPU use.

The restatement, by definition:
  ``edges`` / ``regions``  region ``(a, b)`` of a ``gh x gw`` grid covers pixel rows ``[a * H // gh, (a + 1) * H // gh)`` and columns
                         likewise, index ``a * gw + b``;
  ``occlude``            the image with ``fill`` (per channel) written into one region;
  ``patch_level``        ``oracle.ref_path``'s decoder forward on ``enc_out`` with row ``s`` zeroed -- the start embedding untouched;
  ``pixel_level``        ``oracle.ref_path``'s full model on every occluded image;
  both                   fp64 sums of ``explain_ref.token_logprobs``: ``base [n]``, ``drop [n, R] = base - occluded``, and the per-token
                         ``token_drop [n, L, R]``;
  ``margin``             the smallest ``|drop|`` that is not exactly 0: a comparison of signs or ranks is only meaningful above it."""
import os

import numpy as np
import torch

import explain_ref as E
import pairs_ref as P
from oracle import ref_path as R

GOLDEN = E.GOLDEN
TEMPLATES = P.TEMPLATES                    # rows of synth_images(3, seed=0): the fourth template is a second copy of the first
L = 7
LENGTHS = (7, 4, 2)                        # no pad, three pads, five pads
GRIDS = ((1, 1), (2, 2), (3, 2))
GOLDEN_GRID = (2, 2)
FILL = (0.0, 0.25, -0.5)                   # per channel, in the normalised input space


def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g27_occlusion_{kind}.npz"))


def captions():
    """Three captions of 7 positions -> (captions int64 [3, 7], lengths [3])."""
    g = np.random.Generator(np.random.Philox(key=[E.SEED, 27]))
    cap = torch.zeros((len(LENGTHS), L), dtype=torch.int64)
    for r, n in enumerate(LENGTHS):
        cap[r, :n - 1] = torch.from_numpy(g.integers(6, E.V, size=(n - 1,)).astype(np.int64))
        cap[r, n - 1] = E.EOS
    return cap, torch.tensor(LENGTHS)


def inputs(images3):
    """``images3``: ``synth_images(3, seed=0)`` -> (images [4, ...], captions int64 [12, 7], lengths [12], template_index [12],
    labels [4, 3]): every one of the three captions under every one of the four templates, caption-major -- row ``4 c + t`` is caption
    ``c`` under template ``t``, so the captions of a template are never neighbours."""
    cap, lengths = captions()
    _, _, _, labels = E.captions()
    pick = torch.tensor(TEMPLATES)
    index = torch.arange(len(TEMPLATES)).repeat(len(LENGTHS))
    return images3[pick.to(images3.device)], cap.repeat_interleave(len(TEMPLATES), 0), lengths.repeat_interleave(len(TEMPLATES)), index, labels[pick]


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def edges(size, parts):
    return [(a * size) // parts for a in range(parts + 1)]


def regions(h, w, grid):
    """[(y0, y1, x0, x1)] in index order."""
    gh, gw = grid
    ys, xs = edges(h, gh), edges(w, gw)
    return [(ys[a], ys[a + 1], xs[b], xs[b + 1]) for a in range(gh) for b in range(gw)]


def occlude(image, box, fill):
    """``image [C, H, W]`` with ``fill`` (one number per channel) inside ``box``."""
    y0, y1, x0, x1 = box
    out = image.clone()
    for c in range(image.shape[0]):
        out[c, y0:y1, x0:x1] = fill[c]
    return out


def fill_list(fill, channels=3):
    return [float(fill)] * channels if isinstance(fill, (int, float)) else [float(v) for v in fill]


# ---- the two levels -----------------------------------------------------------------------------------------------------------------
def _scores(rows, n, n_regions):
    """rows fp64 [n, 1 + R, L] (variant 0 unoccluded) -> (base [n], drop [n, R], token_drop [n, L, R])."""
    sums = rows.sum(-1)
    return sums[:, 0], sums[:, :1] - sums[:, 1:], (rows[:, :1] - rows[:, 1:]).transpose(1, 2)


def patch_level(sd, n_heads, start, enc_out, cap, index, pad_index=E.PAD):
    """``start [T, D]``, ``enc_out [T, S, D]`` (fp32, CPU): the encoder's two outputs; ``cap [n, L]``, ``index [n]``."""
    n, s = cap.shape[0], enc_out.shape[1]
    rows = torch.zeros((n, 1 + s, cap.shape[1]), dtype=torch.float64)
    with torch.no_grad():
        for i in range(n):
            t = int(index[i])
            enc = enc_out[t:t + 1].repeat(1 + s, 1, 1)
            for r in range(s):
                enc[1 + r, r] = 0.0
            logits = R.transformer_forward(sd, "decoder", cap[i:i + 1, :-1].repeat(1 + s, 1), enc, start[t:t + 1].repeat(1 + s, 1), pad_index, n_heads)
            rows[i] = E.token_logprobs(logits, cap[i:i + 1].repeat(1 + s, 1), pad_index)
    return _scores(rows, n, s)


def pixel_level(kind, sd, n_heads, images, labels, cap, index, grid, fill, pad_index=E.PAD):
    """The full model on the occluded images; equal template images are encoded once."""
    boxes = regions(images.shape[2], images.shape[3], grid)
    fill = fill_list(fill, images.shape[1])
    n = cap.shape[0]
    rows = torch.zeros((n, 1 + len(boxes), cap.shape[1]), dtype=torch.float64)
    encoded = {}
    with torch.no_grad():
        for i in range(n):
            t = int(index[i])
            key = next((k for k in encoded if torch.equal(images[k], images[t]) and torch.equal(labels[k], labels[t])), t)
            if key not in encoded:
                variants = torch.stack([images[t]] + [occlude(images[t], box, fill) for box in boxes])
                encoded[key] = R._encode(kind, sd, variants, labels[t:t + 1].repeat(len(variants), 1) if "WithLabels" in kind else None)
            start, enc = encoded[key]
            x = cap[i:i + 1, :-1].repeat(1 + len(boxes), 1)
            if "LSTM" in kind:
                logits = R.lstm_decoder_forward(sd, "decoder", start, x, None)
            else:
                logits = R.transformer_forward(sd, "decoder", x, enc, start, pad_index, n_heads)
            rows[i] = E.token_logprobs(logits, cap[i:i + 1].repeat(1 + len(boxes), 1), pad_index)
    return _scores(rows, n, len(boxes))


def margin(drop):
    """The smallest ``|drop|`` among the entries that are not exactly 0 (a masked patch)."""
    d = np.abs(np.asarray(drop, dtype=np.float64))
    return float(d[d > 0].min())


def top_gap(drop):
    """The smallest distance, over the captions, between the largest drop and the runner-up: the margin of ``argmax``."""
    d = np.sort(np.asarray(drop, dtype=np.float64), axis=1)
    return float((d[:, -1] - d[:, -2]).min())


# ---- gates --------------------------------------------------------------------------------------------------------------------------
CEILING = L * 2e-3                         # twice the contract's 1e-3 logit parity per token, L tokens
# (|base - want|, |drop - want|) seen on an MI355X per (kind, level, want), want = the restatement above on the model's own weights or
# golden G27 (the tests print what they see; profiles/occlusion/errors.txt).  fp32, the worst over both settings of f32_split, is gated
# at 1.25 x these and at CEILING.  The 16-bit types are recorded only (WORST_16): their weights are rounded, their binding check is bit
# equality with the single-sequence pass.  The base log-probs reach -78 (an fp32 ulp there is 7.6e-6) and sum up to 7 tokens.
_T, _TL = "CaptioningTransformer", "CaptioningTransformerWithLabels"
WORST = {
    (_T, "patch", "restatement"): (4.472e-06, 9.319e-06), (_T, "patch", "g27"): (7.850e-06, 1.017e-05),
    (_TL, "patch", "restatement"): (6.285e-06, 1.007e-05), (_TL, "patch", "g27"): (1.133e-05, 1.219e-05),
    ("CaptioningLSTM", "pixel", "restatement"): (3.163e-05, 3.347e-05), ("CaptioningLSTM", "pixel", "g27"): (1.962e-05, 3.230e-05),
    ("CaptioningLSTMWithLabels", "pixel", "restatement"): (1.057e-05, 2.699e-05), ("CaptioningLSTMWithLabels", "pixel", "g27"): (8.860e-06, 1.927e-05),
    ("CaptioningTransformerBase", "pixel", "restatement"): (7.894e-06, 1.556e-05), ("CaptioningTransformerBase", "pixel", "g27"): (5.890e-06, 1.218e-05),
    (_T, "pixel", "restatement"): (6.990e-06, 1.161e-05), (_T, "pixel", "g27"): (7.850e-06, 1.585e-05),
    (_TL, "pixel", "restatement"): (5.234e-06, 1.098e-05), (_TL, "pixel", "g27"): (1.133e-05, 1.121e-05),
}
WORST_16 = {                               # against G27: (kind, level) -> {type: (base, drop)}
    (_T, "patch"): {"f16": (1.347e-02, 1.361e-02), "bf16": (9.775e-02, 8.303e-02)},
    (_TL, "patch"): {"f16": (4.057e-03, 8.741e-03), "bf16": (5.145e-02, 6.535e-02)},
    ("CaptioningLSTM", "pixel"): {"f16": (8.903e-03, 1.915e-02), "bf16": (7.408e-02, 1.333e-01)},
    ("CaptioningLSTMWithLabels", "pixel"): {"f16": (1.201e-02, 9.446e-03), "bf16": (9.497e-02, 8.757e-02)},
    ("CaptioningTransformerBase", "pixel"): {"f16": (8.552e-03, 7.609e-03), "bf16": (1.072e-01, 7.583e-02)},
    (_T, "pixel"): {"f16": (1.347e-02, 1.137e-02), "bf16": (9.775e-02, 7.229e-02)},
    (_TL, "pixel"): {"f16": (4.057e-03, 6.506e-03), "bf16": (5.145e-02, 9.783e-02)},
}
gate = lambda worst: 1.25 * worst          # noqa: E731
