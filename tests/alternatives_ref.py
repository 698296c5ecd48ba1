"""What the ``token_alternatives`` tests share (test_alternatives_cpu.py, test_alternatives_gpu.py): the torch-CPU restatement of what
the function returns on given fp32 logits, the inputs of golden G28 (``tests/golden/g28_alternatives_<kind>.npz``, recorded from the
real reference by ``tools/make_alternatives_golden.py``), the tiny models and captions of the GPU tests and the measured gates.  Plain
module, no GPU use.

The restatement (``alternatives``), per row of fp32 logits ``x [V]``:
  values   ``log_softmax(x / T)`` in fp64 over every column, ``unk`` included;
  order    on the fp32 ``x`` itself, largest first, equal logits (``-0.0 == +0.0``) to the lower index: a stable descending sort;
  picks    the first ``top`` columns of that order that are not ``unk`` and are ``> -inf``; the slots behind them are dead: token 0 at
           ``-inf``;
  rank     the slot of a live pick that equals the target, -1 without one;
  pads     a row whose target is the pad: tokens -1, values 0.0, rank -1."""
import os

import numpy as np
import torch

import explain_ref as E
import occlusion_ref as O

GOLDEN = E.GOLDEN
KINDS = E.KINDS
G28_TOP = 8
GAP = 2e-3                                 # twice the 1e-3 fp32 logits tolerance the project is judged by
GAP_SHARE = 0.9                            # the fixture's condition: this share of its (position, rank) entries has a gap above GAP


def alternatives(logits, targets, top, temperature=1.0, unk=None, pad_index=0):
    """``logits`` fp32 ``[rows, V]``, ``targets`` int64 ``[rows]`` -> ``(tokens int64 [rows, top], values fp64 [rows, top], rank int64
    [rows])``."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and targets.shape == logits.shape[:1]
    rows, v = logits.shape
    values = torch.log_softmax(logits.double() / temperature, -1)
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices
    tokens = torch.zeros((rows, top), dtype=torch.int64)
    out = torch.full((rows, top), -float("inf"), dtype=torch.float64)
    rank = torch.full((rows,), -1, dtype=torch.int64)
    for r in range(rows):
        if int(targets[r]) == pad_index:
            tokens[r], out[r] = -1, 0.0
            continue
        cols = order[r]
        live = logits[r, cols] > -float("inf")
        if unk is not None:
            live &= cols != unk
        cols = cols[live][:top]
        tokens[r, :cols.numel()] = cols
        out[r, :cols.numel()] = values[r, cols]
        at = (cols == targets[r]).nonzero()
        if at.numel():
            rank[r] = int(at[0])
    return tokens, out, rank


# ---- golden G28 ---------------------------------------------------------------------------------------------------------------------
def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g28_alternatives_{kind}.npz"))


def g28_inputs(images3):
    """G27's inputs: 4 templates (the fourth a second copy of the first) x 3 captions of 7 positions -> (images [4, ...], captions int64
    [12, 7], lengths [12], template_index [12], labels [4, 3])."""
    return O.inputs(images3)


def gap_share(g):
    """Share of the fixture's (non-pad position, rank) entries whose logit gap to the next rank below exceeds GAP."""
    real = g["captions"] != E.PAD
    return float((g["gaps"][real] > GAP).mean())


# ---- the GPU tests' models and captions ------------------------------------------------------------------------------------------------
V = 301                                    # V % 64 != 0 and V % 4 != 0: the classifier's dense fp32 rows start off a 16-byte boundary; the sweep's tail runs
L = 25
HP = {kind: dict(hp, num_tokens=V) for kind, hp in E.HP.items()}
N_TEMPLATES = 3


def captions(n, seed=28):
    """``n`` captions of 25 positions, lengths 25, 1, 2 ... (one without a pad, one that is only ``<eos>``) over 3 templates
    -> (captions int64 [n, 25], lengths [n], template_index [n], labels [3, 3])."""
    g = np.random.Generator(np.random.Philox(key=[E.SEED, seed]))
    lengths = [L if r == 0 else 1 + (7 * (r - 1)) % L for r in range(n)]
    cap = torch.zeros((n, L), dtype=torch.int64)
    for r, k in enumerate(lengths):
        cap[r, :k - 1] = torch.from_numpy(g.integers(6, V, size=(k - 1,)).astype(np.int64))
        cap[r, k - 1] = E.EOS
    index = torch.arange(n) % N_TEMPLATES
    labels = torch.from_numpy(g.integers(6, V, size=(N_TEMPLATES, 3)).astype(np.int64))
    return cap, torch.tensor(lengths), index, labels


# ---- gates: 1.25 x the worst value seen on an MI355X (the tests print what they see; profiles/alternatives/errors.txt) -----------------
RESTATEMENT_CEILING = 2e-5                 # beam_best.hip's stated bound at |x / T| <= 32
REFERENCE_CEILING = 1e-3                   # fp32 logits / log-probs against the reference and against explain_captions
WORST = {
    "restatement": {"f32": 2.639e-06, "f16": 2.222e-06, "bf16": 1.831e-06},   # values vs the fp64 restatement on the model's own logits, five
    #                                                                            kinds, top 1 / 5 / 64, temperature 0.7 (the worst case), 525 / 500 rows
    "explain": {"f32": 4.768e-07, "f16": 5.960e-07, "bf16": 5.960e-07},       # logprobs[..., rank] vs explain_captions' logprobs
    "generation": {"f32": 0.0, "f16": 3.090e-04, "bf16": 0.0},                # vs generate_batch(return_logprobs=True): fp32 and bf16 the same bits
    #                                                                            (a gate of 1.25 x 0 is equality); fp16: CaptioningTransformerBase
    "g28": 1.287e-05,                                                          # fp32 values vs G28, both settings of f32_split (CaptioningLSTM, option off)
}
WORST_16_G28 = {"f16": (1.231e-02, 10), "bf16": (9.836e-02, 54)}              # recorded, not gated: (values, ids that differ among ~413 sure ones)
gate = lambda worst: 1.25 * worst          # noqa: E731
