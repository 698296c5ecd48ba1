"""Records golden G24 (``tests/golden/g24_sequence_bias_<kind>.npz``): the caption the reference's ``generate`` samples under
``torch.manual_seed`` when every row's logits first pass through the biases of ``sequence_bias`` -- what
``generate_batch(..., sequence_bias=S, rng="torch")`` must return.

Build-container only, like ``tools/make_constraints_golden.py``, whose pattern this follows: it imports the real reference and
commits nothing but arrays.  The reference has no such control.  Its ``BeamSearchHelper.process_logits`` is wrapped at run time so
that ``logits`` pass through ``tests/bias_ref.bias_logits`` with ``sample_seq`` as the rows' history (call number ``c`` of a
``generate`` sees ``1 + c`` tokens), and so is its ``filter_top_k`` outside ``process_logits`` -- the FIRST draw, which is edited too
here: empty history, the single-id biases.  Everything else is the reference's own.

Synthetic weights and images, ``top_k``, beam, temperature, ``max_len`` and the perturbation-stability seed walk are G22's.  Per kind
and slot (images 0 and 1) the PLAIN caption of the seed is recorded first and the list is derived from it, in this order:

* ``([boost], +size)``: a positive single-id bias on a token the plain caption does NOT hold -- the smallest id from 10 on that is
  not in it.  ``size`` is found here: the smallest of ``LADDER`` with which the assertions below pass and the slot is stable; it is
  written into the fixture (``boost_size_<slot>``);
* ``([plain[0]], -4.0)``: a negative bias on the plain caption's first token;
* ``([plain[1], plain[2]], +3.0)``: a two-id phrase taken from it (none if it is shorter).

Asserted here, on the CPU: the recorded caption differs from the plain one and holds the boosted token.  A slot is kept only if 8
runs with every logit multiplied by ``1 + 1e-4 * u`` return the same caption; where no size of the ladder gives that, the seed walks
on from ``100 + i`` (the plain caption and the list are then those of the new seed).

    python tools/make_bias_golden.py [kind ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden as mg                                                   # noqa: E402  (puts the reference on sys.path)
from deephumor.models.beam import BeamSearchHelper                         # noqa: E402
from deephumor_amd.synth import synth_images                               # noqa: E402
from bias_ref import bias_logits                                           # noqa: E402
from make_constraints_golden import KINDS, KW, MAX_LEN, N_PERTURBED, REL, encode_once      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LADDER = (2.0, 4.0, 8.0, 16.0, 32.0)
FIRST_BIAS, PHRASE_BIAS = -4.0, 3.0
N_SLOTS = 2


class _Edits:
    """Wrapper of ``BeamSearchHelper.process_logits`` (the biases at positions >= 1) and ``filter_top_k`` (outside
    ``process_logits``: the first draw -- its perturbation and its biases at position 0)."""

    def __init__(self, pairs, perturb=None):
        self.pairs, self.gen = pairs, perturb
        self.calls, self.edited, self.inside = 0, 0, False
        self.orig, self.orig_filter = BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k

    def _perturbed(self, logits):
        if self.gen is not None:
            logits.mul_(1.0 + REL * (2.0 * torch.rand(logits.shape, generator=self.gen) - 1.0))

    def _biased(self, logits, history, pos):
        if self.pairs:
            out, _, stored = bias_logits(logits, history, pos, self.pairs)
            logits.copy_(out)
            self.edited += int(stored.sum())

    def __enter__(self):
        rec = self

        def process_logits(helper, logits, sample_seq, sample_val):
            rec._perturbed(logits)
            length = 1 + rec.calls
            rec.calls += 1
            rec._biased(logits, sample_seq, length)
            rec.inside = True
            try:
                return rec.orig(helper, logits, sample_seq, sample_val)
            finally:
                rec.inside = False

        def filter_top_k(helper, logits):
            if not rec.inside:
                rec._perturbed(logits)
                rec._biased(logits, torch.zeros((logits.shape[0], 0), dtype=torch.int64), 0)
            return rec.orig_filter(helper, logits)
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = process_logits, filter_top_k
        return self

    def __exit__(self, *exc):
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = self.orig, self.orig_filter


def run(model, args, seed, pairs, kw, perturb=None):
    torch.manual_seed(seed)
    with _Edits(pairs, perturb) as rec, torch.no_grad():
        ids = model.generate(*args, **kw)
    return ids.reshape(-1).numpy().astype(np.int64), rec.edited


def boosted_token(plain):
    """The smallest id from 10 on that the plain caption (a list of ints) does not hold."""
    return next(t for t in range(10, 10 + len(plain) + 1) if t not in plain)


def derived_pairs(plain, size):
    """The list derived from the plain caption (a list of ints) as the module docstring says."""
    pairs = [([boosted_token(plain)], float(size)), ([plain[0]], FIRST_BIAS)]
    if len(plain) >= 3:
        pairs.append(([plain[1], plain[2]], PHRASE_BIAS))
    return pairs


def fixture_ok(out, plain, pairs, max_len):
    """The tool's assertions (tests/test_sequence_bias_cpu.py repeats them on the committed files)."""
    return 1 <= len(out) <= max_len and out != plain and pairs[0][0][0] in out and pairs[0][0][0] not in plain


def stable(model, args, seed, pairs, kw, out):
    gen = torch.Generator().manual_seed(20211 + seed)          # private: the global generator is re-seeded by every run anyway
    for _ in range(N_PERTURBED):
        got, _ = run(model, args, seed, pairs, kw, perturb=gen)
        if got.tolist() != out.tolist():
            return False
    return True


def main():
    torch.set_num_threads(4)
    images = synth_images(4, seed=0)
    _, _, labels = mg.captions_and_lengths(mg.V_SMALL)
    for kind in (sys.argv[1:] or KINDS):
        kw = dict(KW, max_len=MAX_LEN.get(kind, KW["max_len"]))
        model = mg.build(kind, mg.V_SMALL)
        encode_once(model)
        wl = "WithLabels" in kind
        fix = {"max_len": np.int64(kw["max_len"]), "n_slots": np.int64(N_SLOTS)}
        for slot in range(N_SLOTS):
            i = slot
            args = (images[i:i + 1], labels[i:i + 1]) if wl else (images[i:i + 1],)
            seed, found = 100 + i, None
            while found is None:
                plain, _ = run(model, args, seed, [], kw)                # the seed's caption without the list
                for size in LADDER:
                    pairs = derived_pairs(plain.tolist(), size)
                    out, edited = run(model, args, seed, pairs, kw)
                    if fixture_ok(out.tolist(), plain.tolist(), pairs, kw["max_len"]) and stable(model, args, seed, pairs, kw, out):
                        found = (size, pairs, out, edited)
                        break
                else:
                    seed += 1
                    assert seed < 10000
            size, pairs, out, edited = found
            assert fixture_ok(out.tolist(), plain.tolist(), pairs, kw["max_len"])
            offs = np.cumsum([0] + [len(w) for w, _ in pairs]).astype(np.int32)
            fix[f"out_{slot}"], fix[f"seed_{slot}"], fix[f"image_{slot}"] = out, np.int64(seed), np.int64(i)
            fix[f"plain_{slot}"], fix[f"boost_{slot}"], fix[f"boost_size_{slot}"] = plain, np.int64(pairs[0][0][0]), np.float64(size)
            fix[f"words_{slot}"] = np.array([t for w, _ in pairs for t in w], dtype=np.int32)     # the phrases flat, list order
            fix[f"offsets_{slot}"] = offs                                                        # n + 1 offsets
            fix[f"bias_{slot}"] = np.array([b for _, b in pairs], dtype=np.float64)
            fix[f"edited_{slot}"] = np.int64(edited)                                             # columns stored to, all rows, all steps
            print(kind, "slot", slot, "image", i, "seed", seed, "size", size, "pairs", pairs, "edited", edited, "plain", plain.tolist(),
                  "out", out.tolist())
        np.savez_compressed(os.path.join(OUT, f"g24_sequence_bias_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
