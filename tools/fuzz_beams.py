"""Randomised sweep of n-best output (``generate_batch(..., return_beams=True)``) on the GPU: model kind, storage type, beam size,
top_k, max_len, dense prefix or per-image prompts and ``pad_index`` are drawn at random; every case must (a) give a ``best()``
bit-identical to the plain call of the same seed and (b) hold the invariants of ``check_beams`` (permutation, order, lengths by
the first-``<eos>`` rule restated in plain torch, padding).  ``tests/test_beams_gpu.py`` runs one seed of it.

    python tools/fuzz_beams.py [--seed S] [--cases N]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EOS = 3
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")


def own_lengths(tokens, row_lengths, first_cols, eos=EOS):
    """The first-``<eos>`` rule in plain torch: per beam row, the column after its first ``eos`` among columns
    ``first_cols[i] <= c < row_lengths[i]``, or ``row_lengths[i]`` without one.  ``tokens [N, B, T]``."""
    n, b, t = tokens.shape
    col = torch.arange(t, device=tokens.device)[None, None, :]
    live = (col >= first_cols[:, None, None]) & (col < row_lengths[:, None, None]) & (tokens == eos)
    first = torch.where(live, col.expand(n, b, t), torch.full((), t, device=tokens.device)).min(-1).values
    return torch.where(first < t, first + 1, row_lengths[:, None].expand(n, b))


def check_beams(beams, plain, pad_index, first_cols, eos=EOS, tag=""):
    """Checks 2 and 3 of the n-best contract for one call: ``best()`` against the plain call's pair, and the invariants."""
    toks, lens = plain
    bt, bl = beams.best()
    assert torch.equal(bt, toks) and torch.equal(bl, lens), ("best() differs from the plain call", tag)
    n, b, t = beams.tokens.shape
    assert beams.tokens.dtype == beams.lengths.dtype == beams.beam_index.dtype == beams.drawn.dtype == torch.int64
    assert beams.scores.dtype == torch.float32 and tuple(beams.scores.shape) == (n, b) and t == toks.shape[1]
    assert torch.equal(beams.beam_index.sort(1).values, torch.arange(b, device=toks.device).expand(n, b)), ("not a permutation", tag)
    s = torch.nan_to_num(beams.scores, nan=float("-inf"), neginf=-3e38)
    assert bool((s[:, 1:] <= s[:, :-1]).all()), ("scores increase along the slots", tag)
    assert bool((beams.lengths <= beams.row_lengths[:, None]).all()) and bool((beams.lengths >= 0).all())
    first_cols = torch.as_tensor(first_cols, device=toks.device).expand(n)
    assert torch.equal(beams.lengths, own_lengths(beams.tokens, beams.row_lengths, first_cols, eos)), ("own lengths", tag)
    col = torch.arange(t, device=toks.device)[None, None, :]
    tail = col >= beams.row_lengths[:, None, None]
    assert bool((beams.tokens[tail.expand(n, b, t)] == pad_index).all()), ("columns past the row length are not <pad>", tag)
    assert bool(((beams.drawn >= 0) & (beams.drawn < b)).all())


def build(kind, dtype, pad_index=0, v=1000):
    import deephumor_amd.models as M
    from deephumor_amd.synth import load_synthetic
    kw = dict(pad_index=pad_index) if "Transformer" in kind else {}
    return load_synthetic(getattr(M, kind)(v, **kw), seed=1234).eval().to(dtype).cuda()


def with_eos(g, caption):
    """A few ``<eos>`` tokens inside the teacher-forced columns (about one position in four): they are prompt, not a beam's end,
    so a wrong first generated column shows in the own lengths."""
    hit = torch.from_numpy(g.random(size=tuple(caption.shape)) < 0.25)
    return torch.where(hit, torch.full_like(caption, EOS), caption)


def run(seed=0, cases=12, verbose=False):
    from deephumor_amd.synth import synth_images
    g = np.random.Generator(np.random.Philox(key=[seed, 19]))
    images = synth_images(4, seed=0).cuda()
    labels = torch.from_numpy(g.integers(6, 1000, size=(4, 3)).astype(np.int64)).cuda()
    models = {}
    for case in range(cases):
        kind = KINDS[int(g.integers(len(KINDS)))]
        dtype = (torch.float32, torch.bfloat16, torch.float16)[int(g.integers(3))]
        pad = int(g.choice([0, 0, 7])) if "Transformer" in kind else 0
        beam = int(g.choice([1, 2, 3, 5, 8, 17]))
        top_k = beam + int(g.integers(0, 30))
        max_len = int(g.integers(4, 20))
        n = int(g.integers(1, 5))
        mode = int(g.integers(3))                     # 0 no prompt, 1 dense prefix, 2 per-image prompts
        kw = dict(max_len=max_len, beam_size=beam, top_k=top_k, temperature=float(g.uniform(0.7, 1.6)), seed=int(g.integers(1 << 30)),
                  streams=int(g.integers(1, 3)))
        first = torch.zeros(n, dtype=torch.int64)
        if mode == 1:
            p = int(g.integers(1, max(2, max_len - 2)))
            kw["caption"] = with_eos(g, torch.from_numpy(g.integers(6, 1000, size=(n, p)).astype(np.int64))).cuda()
            first[:] = p
        elif mode == 2 and max_len >= 4:
            p = int(g.integers(1, max_len - 2))
            kw["caption"] = with_eos(g, torch.from_numpy(g.integers(6, 1000, size=(n, p)).astype(np.int64))).cuda()
            first = torch.from_numpy(g.integers(0, p + 1, size=(n,)).astype(np.int64))
            kw["caption_lengths"] = first.clone()
        key = (kind, dtype, pad)
        if key not in models:
            models[key] = build(kind, dtype, pad)
        model = models[key]
        args = (images[:n], labels[:n]) if "WithLabels" in kind else (images[:n],)
        with torch.no_grad():
            plain = model.generate_batch(*args, **kw)
            beams = model.generate_batch(*args, return_beams=True, **kw)
        tag = (case, kind, str(dtype), pad, beam, top_k, max_len, n, mode)
        if verbose:
            print(tag)
        check_beams(beams, plain, pad, first.cuda(), tag=tag)
    return cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cases", type=int, default=40)
    a = ap.parse_args()
    print("cases passed:", run(a.seed, a.cases, verbose=True))
