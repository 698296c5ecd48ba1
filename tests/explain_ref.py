"""What the ``explain_captions`` tests share (test_explain_cpu.py, test_explain_gpu.py): the fp64 restatement of what the function
returns, the tiny models and captions of golden G25 (``tests/golden/g25_explain_<kind>.npz``, recorded from the real reference by
``tools/make_explain_golden.py``), the shapes of the fp32 ``dh_vocab_logprob`` kernel test and the measured gates.  Plain module, no
GPU use.

The restatement is the arithmetic, stated plainly in fp64:
  ``token_logprobs``     ``log_softmax(logits[i, p])[captions[i, p]]``, exactly 0 where the caption holds the pad;
  ``perplexity``         ``exp(-sum_p logprobs[i, p] / lengths[i])`` (deephumor/experiments/metrics.py:4-9, per sequence);
  ``head_mean_softmax``  softmax over the keys with the reference's ``-1e8`` fill on masked keys (transformers.py:110-112), mean over heads;
  ``caption_maps``       the maps of the caption's positions, zero on pad rows.
The whole-decoder fp64 forward that feeds them is ``attention_maps_ref.teacher_forced_maps`` (pinned to G23 and to the oracle)."""
import os

import numpy as np
import torch

from vocab_ref import SPIKE, logits_ref, logprob_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")
CROSS_KINDS = KINDS[3:]
SEED = 4321
V = 300
N_KEYS = 49
# tiny models: every decoder width 128 (dh_vocab_logprob's K >= 128; 2 heads of 64: the prefill form applies)
HP = {
    "CaptioningLSTM": dict(num_tokens=V, emb_dim=64, hidden_size=128, num_layers=2),
    "CaptioningLSTMWithLabels": dict(num_tokens=V, emb_dim=64, hidden_size=128, num_layers=1),
    "CaptioningTransformerBase": dict(num_tokens=V, hid_dim=128, n_layers=1, n_heads=2, pf_dim=256),
    "CaptioningTransformer": dict(num_tokens=V, hid_dim=128, n_layers=2, n_heads=2, pf_dim=256),
    "CaptioningTransformerWithLabels": dict(num_tokens=V, hid_dim=128, n_layers=1, n_heads=2, pf_dim=256),
}
PAD, EOS = 0, 3
N_TEMPLATES, L = 3, 9


def captions():
    """7 captions of lengths 1 .. 9 over 3 templates: one that is only ``<eos>``, one without padding (length 9 = L)
    -> (captions int64 [7, 9], lengths [7], template_index [7], labels [3, 3])."""
    g = np.random.Generator(np.random.Philox(key=[SEED, 25]))
    lengths = [1, 9, 4, 2, 7, 5, 3]
    cap = torch.zeros((len(lengths), L), dtype=torch.int64)
    for r, n in enumerate(lengths):
        cap[r, :n - 1] = torch.from_numpy(g.integers(6, V, size=(n - 1,)).astype(np.int64))
        cap[r, n - 1] = EOS
    index = torch.tensor([0, 1, 2, 2, 0, 1, 1])
    labels = torch.from_numpy(g.integers(6, V, size=(N_TEMPLATES, 3)).astype(np.int64))
    return cap, torch.tensor(lengths), index, labels


def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g25_explain_{kind}.npz"))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def token_logprobs(logits, caps, pad_index=PAD):
    """logits [n, >= L, V], caps int64 [n, L] -> fp64 [n, L]."""
    lp = torch.log_softmax(logits[:, :caps.shape[1]].double(), -1).gather(-1, caps.unsqueeze(-1)).squeeze(-1)
    return lp.masked_fill(caps == pad_index, 0.0)


def perplexity(logprobs, caps, lengths, pad_index=PAD):
    lp = (logprobs.double() / lengths.double().unsqueeze(1)).masked_fill(caps == pad_index, 0.0)
    return (-lp.sum(-1)).exp()


def head_mean_softmax(energy, masked):
    """energy [bs, H, L, S], masked bool broadcastable to it -> fp64 [bs, L, S]."""
    return torch.softmax(energy.double().masked_fill(masked, -1e8), -1).mean(1)


def caption_maps(maps, caps, pad_index=PAD):
    """maps [n, >= L, >= 49] of all positions -> the caption's [n, L, 49], zero on pad rows."""
    out = maps[:, :caps.shape[1], :N_KEYS].double().clone()
    out[caps == pad_index] = 0.0
    return out


# ---- the fp32 dh_vocab_logprob kernel test ----------------------------------------------------------------------------------------
KERNEL_M = (1, 37, 129, 300, 513)          # tile edges in M and the 16-bit route's switch point
KERNEL_V = (100, 129, 1000, 36541)         # a partial last group, one column into a second group, the real size
KERNEL_K = (128, 192, 512)
TARGET_EDGES = lambda v: [0, v - 1, -1, v, v - 2]      # noqa: E731  column 0, the last real column, outside (-> 0.0) twice


class KernelCase:
    """One fp32 call: ``a`` is a [m, k] view of a [m, k + 8] buffer (lda > K), targets as vocab_ref.LogprobCase -- rows 0 .. 4
    take TARGET_EDGES (rotated by ``rot``, so that M = 1 meets every one of them over the cases); ``spike``: column 0 of every
    row holds 4 and weight row V / 2 holds SPIKE / 4 there, one logit about 60 above the rest, asked for by row 5."""

    def __init__(self, m, v, k, zero_bias=False, spike=False, rot=0):
        self.m, self.v, self.k, self.zero_bias, self.spike = m, v, k, zero_bias, spike
        g = torch.Generator().manual_seed(15485863 + 7919 * m + 131 * v + k)
        buf = torch.randn(m, k + 8, generator=g)
        w = torch.randn(v, k, generator=g) / k ** 0.5
        if spike:
            buf[:, 0], w[v // 2, 0] = 4.0, SPIKE / 4.0
        self.buf, self.w = buf, w
        self.bias = torch.zeros(v) if zero_bias else torch.randn(v, generator=g)
        t = torch.randint(0, v, (m,), generator=g)
        edges = TARGET_EDGES(v)
        edges = edges[rot % 5:] + edges[:rot % 5]
        t[:min(m, 5)] = torch.tensor(edges[:min(m, 5)])
        if spike and m > 5:
            t[t == v // 2] = v // 2 + 1
            t[5] = v // 2
        self.targets = t
        self._want = None

    @property
    def a(self):
        return self.buf[:, :self.k]

    def what(self):
        return dict(m=self.m, v=self.v, k=self.k, zero_bias=self.zero_bias, spike=self.spike)

    def want(self):
        if self._want is None:
            self._want = logprob_ref(logits_ref(self.a, self.w, self.bias), self.targets)
        return self._want


def kernel_cases(v):
    """Every M at vocabulary ``v``; K, the bias kind and the spike rotate so that over the four vocabularies every (M, K) and
    (V, K) pair, both bias kinds and spike rows at every K occur."""
    vi = KERNEL_V.index(v)
    for mi, m in enumerate(KERNEL_M):
        k = KERNEL_K[(mi + vi) % 3]
        yield KernelCase(m, v, k, zero_bias=(mi + vi) % 2 == 0, spike=False, rot=mi + vi)
        if m >= 37 and (mi + vi) % 2 == 1:
            yield KernelCase(m, v, KERNEL_K[(mi + vi + 1) % 3], zero_bias=False, spike=True, rot=mi)


# ---- gates: 4 x the worst value seen on an MI355X (the tests print what they see; profiles/explain/errors.txt) ----------------------
F32X_LOGP_WORST = 4.054e-05                 # fp32 dh_vocab_logprob vs fp64 over kernel_cases: M = 513, V = 36541, K = 512, spike rows (log-probs of
#                                             -60: an fp32 ulp there is 3.8e-6); without spikes 1.552e-06.  The exact-fp32 logits route
#                                             (dh_linear -> dh_token_logprob) on the same inputs: 9.698e-05 / 3.360e-06
F32X_LOGP_ATOL = 4.0 * F32X_LOGP_WORST
