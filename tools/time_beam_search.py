"""Times what the deterministic search (``search="beam"``) costs the BASELINE C2 and C3 steps on the GPU: ``generate_batch`` of 256
images, V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with ``search="beam"`` against ``search="sample"``
from the same process -- 1,280 rows x 36,541 logits per row step, all of them read for the log-sum-exp --, the two new launches by the
library's own event profiler, and the plain call of ANOTHER checkout (the parent commit, built) to show the default is unchanged.

    python tools/time_beam_search.py c2|c3 [report.txt]            one model: host clock around device-synchronised calls
    python tools/time_beam_search.py plain-c2|plain-c3 [TREE]      the call without the keyword, with the package of TREE (default: this one)
    python tools/time_beam_search.py all DIR [PARENT_TREE]         both models, then the plain call of this tree and of PARENT_TREE

``all`` starts one fresh child process per step, every child under its own ``timeout``, in a chain: a step that fails, faults or runs
out of time ends the chain and nothing starts after it.  Reports land in DIR (``time_beam_search_<model>.txt``).  Information, not a
gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, V, REPEATS = 256, 36541, 10
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}
KW = dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)


def setup(which, tree):
    sys.path.insert(0, tree)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    return torch, model.to(dev).bfloat16(), synth_images(N, seed=0).to(dev)


def timed(torch, model, images, variants, repeats):
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


def line(name, ts):
    return f"  {name:26s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}"


def measure(which, report=None, repeats=REPEATS):
    torch, model, images = setup(which, ROOT)
    from deephumor_amd import hip
    variants = [('search="sample"', {}), ('search="beam"', {"search": "beam"})]
    times = timed(torch, model, images, variants, repeats)
    with torch.no_grad():
        a = model.generate_batch(images, **KW, search="beam", return_beams=True)
        b = model.generate_batch(images, **dict(KW, seed=8), search="beam", return_beams=True)
        same = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        launches = {}
        for name, extra in variants:
            with hip.profile() as prof:
                model.generate_batch(images, **KW, **extra)
            launches[name] = {k: r for k, r in prof.summary().items() if k.split("[")[0].startswith("dh_beam_")}
    lines = [f"deterministic search: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the two settings alternated inside each repeat; ms per {N} images",
             f"two seeds give the same beams and scores: {same}; mean best score {float(a.scores[:, 0].mean()):.3f}, mean length "
             f"{float(a.lengths[:, 0].float().mean()):.2f}", ""]
    for name, ts in times.items():
        lines.append(line(name, ts))
    base, best = (statistics.median(times[n]) for n, _ in variants)
    lines.append(f"  difference of the medians: {best - base:+.3f} ms = {100 * (best - base) / base:+.2f} %")
    lines.append("")
    lines.append("beam launches of one call, event-timed inside the library (one call each, profiler on):")
    for name, recs in launches.items():
        for key, r in sorted(recs.items()):
            per = 1e3 * r["ms"] / max(r["calls"], 1) if "ms" in r else float("nan")
            lines.append(f"  {name:16s} {key:34s} calls {r['calls']:4d}  {per:9.2f} us per launch")
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)


def plain(which, tree, report=None, repeats=REPEATS):
    """The call without the keyword on the package found in ``tree``: run for this tree and for a checkout of the parent commit, the
    two medians show whether the default path moved."""
    torch, model, images = setup(which, tree)
    import deephumor_amd
    where = os.path.relpath(os.path.dirname(deephumor_amd.__file__), ROOT)            # (relative to this tree: "deephumor_amd" is its own)
    ts = timed(torch, model, images, [("plain call", {})], repeats)["plain call"]
    text = f"{KINDS[which]} ({which.upper()}) plain call, package at {where}:\n" + line("no keyword", ts) + "\n"
    print(text)
    if report:
        with open(report, "a") as f:
            f.write("\n" + text)


def chain(out_dir, parent_tree=None):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    steps = []
    for which in KINDS:
        report = os.path.join(out_dir, f"time_beam_search_{which}.txt")
        steps.append((300, [sys.executable, me, which, report]))
        for tree in (ROOT, parent_tree):
            if tree:
                steps.append((240, [sys.executable, me, "plain-" + which, os.path.abspath(tree), report]))
    for limit, cmd in steps:
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
    if mode == "all":
        sys.exit(chain(sys.argv[2] if len(sys.argv) > 2 else ".", sys.argv[3] if len(sys.argv) > 3 else None))
    if mode.startswith("plain-"):
        plain(mode[6:], sys.argv[2] if len(sys.argv) > 2 else ROOT, sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        measure(mode, sys.argv[2] if len(sys.argv) > 2 else None)
