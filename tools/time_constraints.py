"""Times what ``min_len`` and ``bad_words_ids`` cost the BASELINE C2 and C3 steps on the GPU: ``generate_batch`` of 256 images,
V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with

    min_len = 4                                      one launch of dh_beam_constrain_logits at positions 0 .. 3 only
    a 200-phrase list                                one launch (1,280 workgroups) in front of each of the 32 row draws
    both, with no_repeat_ngram_size = 3              two dependent edit launches in front of every row draw
    (and the list's 150 multi-token phrases alone    the launch and the list walk without the singles' stores and repairs)

against the same call without the keywords, on the same tree, in the same process, the settings alternated.

    python tools/time_constraints.py c2|c3 [report.txt]      one model: host clock around device-synchronised calls
    python tools/time_constraints.py all DIR                 both models, one fresh child process each

``all`` starts one child per model, every child under its own ``timeout``, in a chain: a step that fails, faults or runs out of
time ends the chain and nothing starts after it.  Reports land in DIR (``time_constraints_<model>.txt``).  Information, not a gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, REPEATS, MIN_LEN, N_PHRASES, NGRAM = 256, 36541, 10, 4, 200, 3
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}


def phrase_list():
    """200 phrases over the vocabulary: 50 singles, 100 bigrams, 50 trigrams, ids from a seeded generator (above the specials)."""
    import torch
    g = torch.Generator().manual_seed(2024)
    return [torch.randint(6, V, (l,), generator=g).tolist() for l in [1] * 50 + [2] * 100 + [3] * 50]


def measure(which, report=None, repeats=REPEATS):
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.models.beam import compile_bad_words
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).bfloat16()
    images = synth_images(N, seed=0).to(dev)
    kw = dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)
    bad = compile_bad_words(phrase_list(), V, dev)                   # uploaded once, outside the clock
    assert len(bad) == N_PHRASES
    multi = compile_bad_words([w for w in phrase_list() if len(w) > 1], V, dev)
    variants = [("without", {}), (f"min_len = {MIN_LEN}", {"min_len": MIN_LEN}), (f"{N_PHRASES} phrases", {"bad_words_ids": bad}),
                (f"both + no_repeat {NGRAM}", {"min_len": MIN_LEN, "bad_words_ids": bad, "no_repeat_ngram_size": NGRAM}),
                # not one of the three settings, but what tells their cost apart: the list without its 50 singles edits (almost) no
                # column, so this is the launch and the list walk alone -- the rest of the "200 phrases" line is the 50 stores and
                # the ~50 group maxima every row recomputes
                (f"{len(multi)} multi-token only", {"bad_words_ids": multi})]
    times = {}
    with torch.no_grad():
        for _ in range(3):
            for name, extra in variants:
                model.generate_batch(images, **kw, **extra)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, extra in variants:                    # alternated inside every repeat
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.generate_batch(images, **kw, **extra)
                torch.cuda.synchronize()
                times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        a = model.generate_batch(images, **kw)
        differ = {name: int((a[0] != model.generate_batch(images, **kw, **extra)[0]).any(1).sum()) for name, extra in variants[1:]}
    lines = [f"min_len / bad_words_ids: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the settings alternated inside each repeat; ms per {N} images",
             "captions that differ from the call without the keywords: " + ", ".join(f"{k}: {n} of {N}" for k, n in differ.items()), ""]
    for name, ts in times.items():
        lines.append(f"  {name:24s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    base = statistics.median(times["without"])
    for name, _ in variants[1:]:
        on = statistics.median(times[name])
        lines.append(f"  {name:24s} - without, medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)


def chain(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    for which in KINDS:
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_constraints_{which}.txt")]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", "240"] + cmd).returncode
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
    if mode == "all":
        sys.exit(chain(sys.argv[2] if len(sys.argv) > 2 else "."))
    measure(mode, sys.argv[2] if len(sys.argv) > 2 else None)
