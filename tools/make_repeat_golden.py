"""Records golden G21 (``tests/golden/g21_repeat_<kind>.npz``): the caption the reference's ``generate`` samples under
``torch.manual_seed`` when every row's logits first pass through the history edits of ``no_repeat_ngram_size`` /
``repetition_penalty`` -- what ``generate_batch(..., no_repeat_ngram_size=n, repetition_penalty=p, rng="torch")`` must return.

Build-container only, like ``oracle/make_golden.py``: it imports the real reference (``oracle/_standin`` supplies the ResNet-50
definition) and commits nothing but arrays.  The reference has neither control; its ``BeamSearchHelper.process_logits`` is wrapped
at run time so that ``logits`` pass through ``tests/repeat_ref.edit_logits`` with ``sample_seq`` as the rows' history before the
reference's own code runs.  The wrapper supplies the history LENGTH itself (the Transformer's ``sample_seq`` is ``max_len`` wide
and pad-filled): no prefix is used, so call number ``c`` of a ``generate`` sees ``1 + c`` tokens, and the first draw -- empty
history -- needs no wrapper.  Everything else is the reference's own.

Synthetic weights and images as G19 / G20, two images per model kind, ``top_k = 50``, beam 3, T 1.3, max_len 12 (6 for the two
cross-attention models, as G20), two configurations: ``no_repeat_ngram_size = 2``, and ``repetition_penalty = 1.3`` with
``no_repeat_ngram_size = 3``.  A slot is kept only if its caption does not move when the reference's logits are perturbed: 8 runs
of the same seed with every logit in front of the wrapper (and of the first draw) multiplied by ``1 + 1e-4 * u``, ``u`` uniform in
``[-1, 1]`` from a private generator that does not touch the global one.  The project's fp32 logits agree with the reference's to
about 1e-3 absolute; the perturbation stands in for that disagreement, so a near-tie of the sampling race never becomes a
fixture.  The seed walks on from ``100 + i`` until that holds.  CPU and reference only: the kernels are not consulted.

    python tools/make_repeat_golden.py [kind ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as mg                                                   # noqa: E402  (puts the reference on sys.path)
from deephumor.models.beam import BeamSearchHelper                         # noqa: E402
from deephumor_amd.synth import synth_images                               # noqa: E402
from repeat_ref import edit_logits, repeated_ngrams                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
MAX_LEN = {"CaptioningTransformer": 6, "CaptioningTransformerWithLabels": 6}
CONFIGS = ((2, 1.0), (3, 1.3))            # (no_repeat_ngram_size, repetition_penalty)
N_PERTURBED, REL = 8, 1e-4
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")


class _Edits:
    """Wrapper of ``BeamSearchHelper.process_logits`` (history edits) and ``filter_top_k`` (perturbation of the first draw)."""

    def __init__(self, ngram, penalty, perturb=None):
        self.ngram, self.penalty, self.gen = ngram, penalty, perturb
        self.calls, self.edited, self.inside = 0, 0, False
        self.orig, self.orig_filter = BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k

    def _perturbed(self, logits):
        if self.gen is not None:
            logits.mul_(1.0 + REL * (2.0 * torch.rand(logits.shape, generator=self.gen) - 1.0))

    def __enter__(self):
        rec = self

        def process_logits(helper, logits, sample_seq, sample_val):
            rec._perturbed(logits)
            length = 1 + rec.calls
            rec.calls += 1
            if rec.ngram > 0 or rec.penalty != 1.0:
                out, _, stored = edit_logits(logits, sample_seq, length, rec.ngram, rec.penalty)
                logits.copy_(out)
                rec.edited += int(stored.sum())
            rec.inside = True
            try:
                return rec.orig(helper, logits, sample_seq, sample_val)
            finally:
                rec.inside = False

        def filter_top_k(helper, logits):
            if not rec.inside:
                rec._perturbed(logits)
            return rec.orig_filter(helper, logits)
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = process_logits, filter_top_k
        return self

    def __exit__(self, *exc):
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = self.orig, self.orig_filter


def run(model, args, seed, ngram, penalty, kw, perturb=None):
    torch.manual_seed(seed)
    with _Edits(ngram, penalty, perturb) as rec, torch.no_grad():
        ids = model.generate(*args, **kw)
    return ids.reshape(-1).numpy().astype(np.int64), rec.edited


def encode_once(model):
    """The seed walk re-runs ``generate`` on the same image many times: the encoder's result is kept per input tensor."""
    forward, cache = model.encoder.forward, {}

    def cached(*args, **kw):
        key = tuple(a.data_ptr() for a in args) + tuple(v.data_ptr() for v in kw.values())
        if key not in cache:
            cache[key] = forward(*args, **kw)
        return cache[key]
    model.encoder.forward = cached


def stable(model, args, seed, ngram, penalty, kw, out):
    gen = torch.Generator().manual_seed(20211 + seed)          # private: the global generator is re-seeded by every run anyway
    for _ in range(N_PERTURBED):
        got, _ = run(model, args, seed, ngram, penalty, kw, perturb=gen)
        if got.tolist() != out.tolist():
            return False
    return True


def main():
    torch.set_num_threads(4)
    images = synth_images(4, seed=0)
    _, _, labels = mg.captions_and_lengths(mg.V_SMALL)
    differs = 0
    for kind in (sys.argv[1:] or KINDS):
        kw = dict(KW, max_len=MAX_LEN.get(kind, KW["max_len"]))
        model = mg.build(kind, mg.V_SMALL)
        encode_once(model)
        wl = "WithLabels" in kind
        fix = {"max_len": np.int64(kw["max_len"]), "n_configs": np.int64(len(CONFIGS))}
        for c, (ngram, penalty) in enumerate(CONFIGS):
            fix[f"ngram_{c}"], fix[f"penalty_{c}"] = np.int64(ngram), np.float32(penalty)
            for slot in range(2):
                i = slot
                args = (images[i:i + 1], labels[i:i + 1]) if wl else (images[i:i + 1],)
                seed = 100 + i
                while True:
                    out, edited = run(model, args, seed, ngram, penalty, kw)
                    if stable(model, args, seed, ngram, penalty, kw, out):
                        break
                    seed += 1
                    assert seed < 10000
                plain, _ = run(model, args, seed, 0, 1.0, kw)
                assert not repeated_ngrams(out.tolist(), ngram), (kind, c, slot, out.tolist())
                differs += out.tolist() != plain.tolist()
                pre = f"c{c}_"
                fix[pre + f"out_{slot}"], fix[pre + f"seed_{slot}"], fix[pre + f"image_{slot}"] = out, np.int64(seed), np.int64(i)
                fix[pre + f"plain_{slot}"] = plain               # the same seed without the controls
                fix[pre + f"edited_{slot}"] = np.int64(edited)   # columns the edits stored to, all rows, all steps
                print(kind, "config", (ngram, penalty), "image", i, "seed", seed, "edited", edited, "out", out.tolist(),
                      "" if out.tolist() != plain.tolist() else "(== plain)")
        np.savez_compressed(os.path.join(OUT, f"g21_repeat_{kind}.npz"), **fix)
    print("captions that differ from the plain caption of the same seed:", differs)       # (tests/test_repeat_cpu.py asserts >= 1)


if __name__ == "__main__":
    main()
