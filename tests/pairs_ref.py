"""What the ``score_pairs`` tests share (test_pairs_cpu.py, test_pairs_gpu.py): fp64 numpy restatements of the three readers of
the matrix ``log p(caption i | template t)``, the inputs of golden G26 (``tests/golden/g26_pairs_<kind>.npz``, recorded from the real
reference by ``tools/make_pairs_golden.py``) and the measured gates.  Plain module, no GPU use.

The restatements are the definitions, stated with python loops and ``sorted`` (stable) on fp64 numbers:
  ``rank_templates``   key = logprob + log(prior / sum prior); largest first, ties to the lower index; probability = softmax of the key
                       over all templates;
  ``rank_captions``    key = logprob | logprob / length | logprob - log mean_t' exp(logprob[i, t']); per template, largest first,
                       ties to the lower caption index;
  ``template_accuracy`` share of captions whose true template is in the first k ranks."""
import os

import numpy as np
import torch

import explain_ref as E

GOLDEN = E.GOLDEN
TEMPLATES = (0, 1, 2, 0)                   # rows of synth_images(3, seed=0): the fourth template is a second copy of the first
N_CAPTIONS, N_TEMPLATES = 7, 4


def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g26_pairs_{kind}.npz"))


def inputs(images3):
    """``images3``: ``synth_images(3, seed=0)`` -> (images [4, ...], captions int64 [7, 9], lengths [7], labels [4, 3])."""
    cap, lengths, _, labels = E.captions()
    pick = torch.tensor(TEMPLATES)
    return images3[pick.to(images3.device)], cap, lengths, labels[pick]


# ---- the restatements -------------------------------------------------------------------------------------------------------------
def _order(keys):
    """Indices of ``keys`` by descending value, equal values by ascending index."""
    return sorted(range(len(keys)), key=lambda j: (-keys[j], j))


def rank_templates(logprob, top, prior=None):
    lp = np.asarray(logprob, dtype=np.float64)
    n, t = lp.shape
    p = np.full(t, 1.0 / t) if prior is None else np.asarray(prior, dtype=np.float64) / np.sum(np.asarray(prior, dtype=np.float64))
    key = lp + np.log(p)[None, :]
    index = np.zeros((n, top), dtype=np.int64)
    score = np.zeros((n, top))
    prob = np.zeros((n, top))
    for i in range(n):
        order = _order(list(key[i]))[:top]
        w = np.exp(key[i] - key[i].max())
        w = w / w.sum()
        index[i], score[i], prob[i] = order, key[i][order], w[order]
    return index, score, prob


def caption_keys(logprob, lengths, normalize=None):
    lp = np.asarray(logprob, dtype=np.float64)
    if normalize == "length":
        return lp / np.asarray(lengths, dtype=np.float64)[:, None]
    if normalize == "pmi":
        m = lp.max(1, keepdims=True)
        return lp - (m + np.log(np.exp(lp - m).mean(1, keepdims=True)))
    assert normalize is None
    return lp


def rank_captions(logprob, lengths, top, normalize=None):
    key = caption_keys(logprob, lengths, normalize)
    n, t = key.shape
    index = np.zeros((t, top), dtype=np.int64)
    score = np.zeros((t, top))
    for j in range(t):
        order = _order(list(key[:, j]))[:top]
        index[j], score[j] = order, key[:, j][order]
    return index, score


def template_accuracy(index, true_index, ks):
    return {k: sum(int(true_index[i]) in [int(v) for v in index[i][:k]] for i in range(len(true_index))) / len(true_index) for k in ks}


def ulps32(got, want):
    """Largest distance of fp32 ``got`` from fp64 ``want`` in units of ``want``'s fp32 spacing."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)))


# ---- gates: 4 x the worst value seen on an MI355X (the tests print what they see; profiles/pairs/errors.txt) -----------------------
# |logprob - G26| per kind, fp32 over both settings of f32_split; 16-bit types against the same fp64 values of the fp32 reference
# (their binding check is bit equality with explain_captions on the single pair).
# The largest pair log-prob is -94 (an fp32 ulp there is 7.6e-6) and sums up to 9 tokens, each within G25's 8.8e-6.
_K = E.KINDS
WORST_LOGPROB = {
    **dict(zip(((k, "f32") for k in _K), (1.667e-05, 1.487e-05, 6.460e-06, 7.368e-06, 7.054e-06))),     # f32_split on: 1.427e-05 at most
    **dict(zip(((k, "f16") for k in _K), (1.214e-02, 1.393e-02, 5.824e-03, 1.257e-02, 8.787e-03))),
    **dict(zip(((k, "bf16") for k in _K), (2.212e-01, 9.973e-02, 6.888e-02, 9.511e-02, 6.920e-02))),
}
WORST_PERPLEXITY_REL = {                   # |perplexity / G26 - 1|
    **dict(zip(((k, "f32") for k in _K), (2.234e-06, 3.271e-06, 2.110e-06, 3.178e-06, 3.654e-06))),
    **dict(zip(((k, "f16") for k in _K), (3.029e-03, 5.560e-03, 4.700e-03, 3.636e-03, 4.881e-03))),
    **dict(zip(((k, "bf16") for k in _K), (4.523e-02, 4.389e-02, 2.774e-02, 2.718e-02, 2.448e-02))),
}
gate = lambda worst: 4.0 * worst           # noqa: E731
