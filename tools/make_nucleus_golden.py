"""Records golden G20 (``tests/golden/g20_nucleus_<kind>.npz``): the caption the reference's ``generate`` samples under
``torch.manual_seed`` when every row draw runs over the NUCLEUS of its top-k survivors -- what
``generate_batch(..., top_p=0.8, rng="torch")`` must return.

Build-container only, like ``oracle/make_golden.py``: it imports the real reference (``oracle/_standin`` supplies the ResNet-50
definition) and commits nothing but arrays.  The reference has no top-p; its ``BeamSearchHelper.filter_top_k`` is wrapped at run
time so that its result additionally carries the nucleus rule as an in-place ``-inf`` mask (``tests/nucleus_ref.nucleus_filter_``:
survivors by ``p = softmax(survivors / T)`` descending, equal ``p`` by index; position ``j`` stays iff its exclusive prefix of ``p`` is
``< top_p`` or ``j < beam_size``).  Everything else -- the multinomial draws, the candidate step, the final draw -- is the
reference's own.

Synthetic weights and images as G19, two of the four images per model kind (the first two whose FIRST row, which no seed moves,
keeps the margin below), ``top_p = 0.8``, ``top_k = 50``, beam 3, T 1.3, max_len 12 (6 for the two cross-attention models).  Per
image the recorder also keeps the smallest ``|exclusive prefix - top_p|`` met at any row of any step: the seed walks on from
``100 + i`` until that margin is at least 1e-3 (a boundary closer than the fp32 disagreement of two logits computations would make
the fixture a coin toss), and margin and seed are part of the fixture.

    python tools/make_nucleus_golden.py [kind ...]
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
from nucleus_ref import nucleus_filter_                                    # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TOP_P = 0.8
KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
# the cross-attention models re-run 49 + positions per token on the CPU and draw 3 more rows per step: their walk is over shorter
# captions (fewer rows per trial that all have to keep the margin); max_len is part of every fixture
MAX_LEN = {"CaptioningTransformer": 6, "CaptioningTransformerWithLabels": 6}
MIN_MARGIN = 1e-3
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")


class _Nucleus:
    """Wrapper of ``BeamSearchHelper.filter_top_k``: appends the nucleus mask and records every call's margin and kept counts."""

    def __init__(self, top_p):
        self.top_p, self.margins, self.kept = top_p, [], []
        self.orig = BeamSearchHelper.filter_top_k

    def __enter__(self):
        rec = self

        def wrapped(helper, logits):
            out = rec.orig(helper, logits)
            survivors = int(torch.isfinite(out).sum())
            _, margin = nucleus_filter_(out, helper.temperature, rec.top_p, helper.beam_size)
            rec.margins.append(margin)
            rec.kept.append((int(torch.isfinite(out).sum()), survivors))
            return out
        BeamSearchHelper.filter_top_k = wrapped
        return self

    def __exit__(self, *exc):
        BeamSearchHelper.filter_top_k = self.orig


def run(model, args, seed, top_p, kw):
    torch.manual_seed(seed)
    if top_p >= 1.0:
        with torch.no_grad():
            return model.generate(*args, **kw).reshape(-1).numpy().astype(np.int64), None
    with _Nucleus(top_p) as rec, torch.no_grad():
        ids = model.generate(*args, **kw)
    return ids.reshape(-1).numpy().astype(np.int64), rec


def encode_once(model):
    """The seed walk re-runs ``generate`` on the same image hundreds of times: the encoder's result is kept per input tensor (the
    encoder is deterministic in eval mode; only the decoder loop consumes random numbers)."""
    forward, cache = model.encoder.forward, {}

    def cached(*args, **kw):
        key = tuple(a.data_ptr() for a in args) + tuple(v.data_ptr() for v in kw.values())
        if key not in cache:
            cache[key] = forward(*args, **kw)
        return cache[key]
    model.encoder.forward = cached


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
        fix = {"top_p": np.float32(TOP_P), "max_len": np.int64(kw["max_len"])}
        slot = 0
        for i in range(4):
            if slot == 2:
                break
            args = (images[i:i + 1], labels[i:i + 1]) if wl else (images[i:i + 1],)
            seed = 100 + i
            out, rec = run(model, args, seed, TOP_P, kw)
            if rec.margins[0] < MIN_MARGIN:
                # the first draw's logits depend on the image alone: no seed moves its boundary -- the next image
                print(kind, "image", i, "skipped: the boundary of its first row lies", rec.margins[0], "from top_p")
                continue
            while min(rec.margins) < MIN_MARGIN:
                seed += 1
                assert seed < 100000
                out, rec = run(model, args, seed, TOP_P, kw)
            plain, _ = run(model, args, seed, 1.0, kw)
            differs += out.tolist() != plain.tolist()
            kept, surv = sum(k for k, _ in rec.kept), sum(s for _, s in rec.kept)
            fix[f"out_{slot}"], fix[f"seed_{slot}"], fix[f"margin_{slot}"] = out, np.int64(seed), np.float32(min(rec.margins))
            fix[f"image_{slot}"] = np.int64(i)
            fix[f"plain_{slot}"] = plain                     # the same seed without the nucleus (top_p = 1)
            fix[f"kept_{slot}"] = np.array([kept, surv], dtype=np.int64)    # tokens the nucleus kept / top-k survivors, all rows, all steps
            slot += 1
            print(kind, "image", i, "seed", seed, "margin", min(rec.margins), "kept", kept, "of", surv, "out", out.tolist(),
                  "" if out.tolist() != plain.tolist() else "(== top_p 1)")
        assert slot == 2, "fewer than two of the four images have a usable first row"
        np.savez_compressed(os.path.join(OUT, f"g20_nucleus_{kind}.npz"), **fix)
    print("captions that differ from the top_p = 1 caption of the same seed:", differs)       # (tests/test_nucleus_cpu.py asserts >= 1)


if __name__ == "__main__":
    main()
