"""Times what ``sequence_bias`` costs the BASELINE C2 and C3 steps on the GPU: ``generate_batch`` of 256 images, V = 36,541, bf16,
beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with

    1 bias                                           one launch of dh_beam_bias_logits (1,280 workgroups) in front of each row draw,
                                                     one column and one group of every row edited
    50 single-id biases                              the same launch; 50 columns, ~50 groups of every row re-read at every position
    a 200-phrase list                                50 singles, 100 bigrams, 50 trigrams: tools/time_constraints.py's list, with biases
    (the same 200 phrases as bad_words_ids           the sibling launch, for comparison)

against the same call without the keyword, on the same tree, in the same process, the settings alternated.

    python tools/time_bias.py c2|c3 [report.txt]             one model: host clock around device-synchronised calls
    python tools/time_bias.py all DIR                        both models, one fresh child process each
    python tools/time_bias.py plain c2|c3 [TREE]             the call WITHOUT the keyword alone, on TREE's package (default: this tree)
    python tools/time_bias.py versus TREE DIR                the plain call of this tree against TREE's (a checkout of the parent
                                                             commit, built), fresh processes in turn, ROUNDS rounds per model

``all`` and ``versus`` start their children one at a time, every child under its own ``timeout``, in a chain: a step that fails,
faults or runs out of time ends the chain and nothing starts after it.  Reports land in DIR (``time_bias_<model>.txt``,
``plain_vs_parent.txt``).  Information, not a gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, V, REPEATS, N_PHRASES, ROUNDS = 256, 36541, 10, 200, 3
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}
KW = dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)


def phrase_list():
    """200 phrases over the vocabulary: 50 singles, 100 bigrams, 50 trigrams, ids from a seeded generator (above the specials) --
    ``tools/time_constraints.py``'s list -- and a bias in ``[-4, 4)`` for each."""
    import torch
    g = torch.Generator().manual_seed(2024)
    phrases = [torch.randint(6, V, (l,), generator=g).tolist() for l in [1] * 50 + [2] * 100 + [3] * 50]
    return [(w, float(torch.rand(1, generator=g)) * 8.0 - 4.0) for w in phrases]


def load(which, tree=ROOT):
    sys.path.insert(0, tree)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    return model.to(dev).bfloat16(), synth_images(N, seed=0).to(dev), dev


def timed(model, images, variants, repeats):
    import torch
    times = {}
    with torch.no_grad():
        for _ in range(3):
            for name, extra in variants:
                model.generate_batch(images, **KW, **extra)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, extra in variants:                    # alternated inside every repeat
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.generate_batch(images, **KW, **extra)
                torch.cuda.synchronize()
                times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
    return times


def measure(which, report=None, repeats=REPEATS):
    import torch
    model, images, dev = load(which)
    from deephumor_amd.models.beam import compile_bad_words, compile_sequence_bias
    pairs = phrase_list()
    full = compile_sequence_bias(pairs, V, dev)                      # uploaded once, outside the clock
    assert len(full) == N_PHRASES
    one = compile_sequence_bias(pairs[:1], V, dev)
    singles = compile_sequence_bias(pairs[:50], V, dev)
    bad = compile_bad_words([w for w, _ in pairs], V, dev)
    variants = [("without", {}), ("1 bias", {"sequence_bias": one}), ("50 single-id biases", {"sequence_bias": singles}),
                (f"{N_PHRASES}-phrase list", {"sequence_bias": full}), (f"{N_PHRASES} phrases banned", {"bad_words_ids": bad})]
    times = timed(model, images, variants, repeats)
    with torch.no_grad():
        a = model.generate_batch(images, **KW)
        differ = {name: int((a[0] != model.generate_batch(images, **KW, **extra)[0]).any(1).sum()) for name, extra in variants[1:]}
    lines = [f"sequence_bias: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the settings alternated inside each repeat; ms per {N} images",
             "captions that differ from the call without the keyword: " + ", ".join(f"{k}: {n} of {N}" for k, n in differ.items()), ""]
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


def plain(which, tree=ROOT):
    """The median of the call without the keyword on ``tree``'s package, as one line ``PLAIN <model> <ms>``."""
    model, images, _ = load(which, os.path.abspath(tree))
    ts = timed(model, images, [("without", {})], REPEATS)["without"]
    print(f"PLAIN {which} {statistics.median(ts):.4f}", flush=True)


def child(args, limit=240):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, text=True)
    print(p.stdout, end="", flush=True)
    return p.returncode, p.stdout


def chain(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for which in KINDS:
        rc, _ = child([which, os.path.join(out_dir, f"time_bias_{which}.txt")])
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


def versus(tree, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    got = {(w, t): [] for w in KINDS for t in ("this", "parent")}
    for which in KINDS:
        for _ in range(ROUNDS):
            for name, where in (("this", ROOT), ("parent", tree)):          # fresh processes in turn
                rc, out = child(["plain", which, where])
                if rc != 0:
                    print(f"step ended with status {rc}: nothing further is started", flush=True)
                    return rc
                got[(which, name)].append(float([l for l in out.splitlines() if l.startswith("PLAIN ")][-1].split()[2]))
    lines = [f"the call without the keyword, this tree against the parent commit's: V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50; "
             f"{ROUNDS} rounds per model, a fresh process per tree and round in turn, each the median of {REPEATS} calls; ms per {N} images", ""]
    for which in KINDS:
        a, b = got[(which, "this")], got[(which, "parent")]
        lines.append(f"  {which}: this tree {statistics.median(a):.3f} (rounds {min(a):.3f} .. {max(a):.3f}), parent {statistics.median(b):.3f} "
                     f"(rounds {min(b):.3f} .. {max(b):.3f}); difference of medians {statistics.median(a) - statistics.median(b):+.3f} ms, "
                     f"spread between rounds {max(max(a) - min(a), max(b) - min(b)):.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out_dir, "plain_vs_parent.txt"), "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
    if mode == "all":
        sys.exit(chain(sys.argv[2] if len(sys.argv) > 2 else "."))
    if mode == "versus":
        sys.exit(versus(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "."))
    if mode == "plain":
        plain(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ROOT)
    else:
        measure(mode, sys.argv[2] if len(sys.argv) > 2 else None)
