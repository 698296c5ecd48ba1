"""Records golden G22 (``tests/golden/g22_constraints_<kind>.npz``): the caption the reference's ``generate`` samples under
``torch.manual_seed`` when every row's logits first pass through the bans of ``min_len`` / ``bad_words_ids`` -- what
``generate_batch(..., min_len=m, bad_words_ids=W, rng="torch")`` must return.

Build-container only, like ``tools/make_repeat_golden.py``, whose pattern this follows: it imports the real reference and commits
nothing but arrays.  The reference has neither control.  Its ``BeamSearchHelper.process_logits`` is wrapped at run time so that
``logits`` pass through ``tests/constraints_ref.constrain_logits`` with ``sample_seq`` as the rows' history (call number ``c`` of a
``generate`` sees ``1 + c`` tokens), and so is its ``filter_top_k`` outside ``process_logits`` -- the FIRST draw, which is edited
too here: empty history, the ``<eos>`` ban while ``0 < min_len``, the single-id bans.  Everything else is the reference's own.

Synthetic weights and images, ``top_k``, beam, temperature, ``max_len`` and the perturbation-stability seed walk are G21's.  Per
kind and slot the PLAIN caption of the seed is recorded first and the controls are derived from it (a caption's length counts its
``<eos>``; the reference returns the whole row, pads included, so the length is taken at the first ``<eos>``):

* ``min_len`` = the plain caption's length + 2 where it ended early (it is shorter than ``max_len``), capped at ``max_len - 1``;
  0 where it did not;
* ``bad_words_ids`` = the plain caption's first token as a single, one bigram taken from it (its second and third token; none if it
  is shorter), and one phrase that cannot fire (``<unk>`` is never drawn, so ``[<unk>, 5]`` never has its prefix in a history).

Slots 0 and 1 are images 0 and 1 with the reference's ``eos_index`` (3).  The synthetic models hardly ever draw that token (one of
1,000, rarely among the top-k), so their plain captions do not end early and ``min_len`` stays 0 there.  Slots 2 and 3 are the same
two images with ``eos_index`` = the THIRD token of the seed's caption under the default ``eos_index``: the plain caption of that
``eos_index`` ends early and ``min_len`` bites.  The single is left out of their lists (a banned first token sends the caption
somewhere else at once, and that ``<eos>`` is never met again): the recorded caption follows the plain one for two tokens, is
refused its ``<eos>`` -- by ``min_len`` and by the bigram, which ends in it -- and must run on past ``min_len``.

Asserted here, on the CPU: the recorded caption holds no banned phrase and no ``<eos>`` below ``min_len``, and differs from the
plain one.  A slot is kept only if 8 runs with every logit multiplied by ``1 + 1e-4 * u`` return the same caption; the seed walks
on from ``100 + i`` until that holds (the plain caption and the controls are then those of the new seed).

    python tools/make_constraints_golden.py [kind ...]
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
from constraints_ref import EOS, UNK, banned_phrase_in, constrain_logits, eos_below, flatten      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
MAX_LEN = {"CaptioningTransformer": 6, "CaptioningTransformerWithLabels": 6}
N_PERTURBED, REL = 8, 1e-4
KINDS = ("CaptioningLSTM", "CaptioningLSTMWithLabels", "CaptioningTransformerBase", "CaptioningTransformer",
         "CaptioningTransformerWithLabels")


class _Edits:
    """Wrapper of ``BeamSearchHelper.process_logits`` (the bans at positions >= 1) and ``filter_top_k`` (outside
    ``process_logits``: the first draw -- its perturbation and its bans at position 0)."""

    def __init__(self, min_len, phrases, eos, perturb=None):
        self.min_len, self.phrases, self.eos, self.gen = min_len, phrases, eos, perturb
        self.calls, self.edited, self.inside = 0, 0, False
        self.orig, self.orig_filter = BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k

    def _perturbed(self, logits):
        if self.gen is not None:
            logits.mul_(1.0 + REL * (2.0 * torch.rand(logits.shape, generator=self.gen) - 1.0))

    def _banned(self, logits, history, pos):
        if self.min_len > 0 or self.phrases:
            out, _, stored = constrain_logits(logits, history, pos, self.phrases, self.min_len, self.eos)
            logits.copy_(out)
            self.edited += int(stored.sum())

    def __enter__(self):
        rec = self

        def process_logits(helper, logits, sample_seq, sample_val):
            rec._perturbed(logits)
            length = 1 + rec.calls
            rec.calls += 1
            rec._banned(logits, sample_seq, length)
            rec.inside = True
            try:
                return rec.orig(helper, logits, sample_seq, sample_val)
            finally:
                rec.inside = False

        def filter_top_k(helper, logits):
            if not rec.inside:
                rec._perturbed(logits)
                rec._banned(logits, torch.zeros((logits.shape[0], 0), dtype=torch.int64), 0)
            return rec.orig_filter(helper, logits)
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = process_logits, filter_top_k
        return self

    def __exit__(self, *exc):
        BeamSearchHelper.process_logits, BeamSearchHelper.filter_top_k = self.orig, self.orig_filter


def run(model, args, seed, min_len, phrases, kw, perturb=None):
    torch.manual_seed(seed)
    with _Edits(min_len, phrases, kw.get("eos_index", EOS), perturb) as rec, torch.no_grad():
        ids = model.generate(*args, **kw)
    return ids.reshape(-1).numpy().astype(np.int64), rec.edited


def caption_length(tokens, eos):
    """Up to and including the first ``eos``; all of ``tokens`` (a list of ints) without one."""
    return tokens.index(eos) + 1 if eos in tokens else len(tokens)


def controls(plain, max_len, eos=EOS, single=True):
    """``(min_len, phrases)`` derived from the plain caption (a list of ints) as the module docstring says."""
    n = caption_length(plain, eos)
    min_len = min(n + 2, max_len - 1) if n < max_len else 0
    phrases = [[plain[0]]] if single else []
    if len(plain) >= 3:
        phrases.append([plain[1], plain[2]])
    phrases.append([UNK, 5])
    return min_len, phrases


def check_fixture(out, plain, min_len, phrases, max_len, eos=EOS):
    """The tool's assertions (tests/test_constraints_cpu.py repeats them on the committed files)."""
    assert 1 <= len(out) <= max_len
    assert banned_phrase_in(out[:caption_length(out, eos)], phrases) is None, (out, phrases)
    assert not eos_below(out, min_len, eos), (out, min_len)
    assert out != plain, (out, plain)


def encode_once(model):
    """The seed walk re-runs ``generate`` on the same image many times: the encoder's result is kept per input tensor."""
    forward, cache = model.encoder.forward, {}

    def cached(*args, **kw):
        key = tuple(a.data_ptr() for a in args) + tuple(v.data_ptr() for v in kw.values())
        if key not in cache:
            cache[key] = forward(*args, **kw)
        return cache[key]
    model.encoder.forward = cached


def stable(model, args, seed, min_len, phrases, kw, out):
    gen = torch.Generator().manual_seed(20211 + seed)          # private: the global generator is re-seeded by every run anyway
    for _ in range(N_PERTURBED):
        got, _ = run(model, args, seed, min_len, phrases, kw, perturb=gen)
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
        fix = {"max_len": np.int64(kw["max_len"]), "n_slots": np.int64(4)}
        for slot in range(4):
            i = slot % 2
            args = (images[i:i + 1], labels[i:i + 1]) if wl else (images[i:i + 1],)
            seed = 100 + i
            while True:
                eos, first = EOS, None
                if slot >= 2:                                            # an <eos> the model does draw: see the module docstring
                    first = run(model, args, seed, 0, [], kw)[0].tolist()
                    eos = first[2]
                skw = dict(kw, eos_index=eos)
                plain, _ = run(model, args, seed, 0, [], skw)            # the seed's caption without the controls
                min_len, phrases = controls(plain.tolist(), kw["max_len"], eos, single=slot < 2)
                out, edited = run(model, args, seed, min_len, phrases, skw)
                if (slot < 2 or (eos not in first[:2] and min_len > 0)) and stable(model, args, seed, min_len, phrases, skw, out):
                    break
                seed += 1
                assert seed < 10000
            check_fixture(out.tolist(), plain.tolist(), min_len, phrases, kw["max_len"], eos)
            words, offs = flatten(phrases)
            fix[f"out_{slot}"], fix[f"seed_{slot}"], fix[f"image_{slot}"] = out, np.int64(seed), np.int64(i)
            fix[f"plain_{slot}"], fix[f"min_len_{slot}"], fix[f"eos_{slot}"] = plain, np.int64(min_len), np.int64(eos)
            fix[f"words_{slot}"], fix[f"offsets_{slot}"] = words.numpy(), offs.numpy()     # the phrases flat + n + 1 offsets
            fix[f"edited_{slot}"] = np.int64(edited)                                       # columns the bans stored to, all rows, all steps
            print(kind, "slot", slot, "image", i, "seed", seed, "eos", eos, "min_len", min_len, "phrases", phrases, "edited", edited,
                  "plain", plain.tolist(), "out", out.tolist())
        np.savez_compressed(os.path.join(OUT, f"g22_constraints_{kind}.npz"), **fix)


if __name__ == "__main__":
    main()
