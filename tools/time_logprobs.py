"""Times what ``return_logprobs=True`` costs the BASELINE C2 / C3 steps on the GPU: ``generate_batch`` of 256 images with
``CaptioningLSTM`` / ``CaptioningTransformer``, V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with

    return_logprobs = True                           dh_beam_pick_logprobs in front of and dh_beam_record_logprobs behind every
                                                     select, the n-best final draw and one dh_beam_gather_logprobs
    return_logprobs + return_beams                   the same launches; every slot's values are returned, no slot is sliced
    search="beam" (+ return_logprobs)                the pick launch copies pick_val instead of sweeping the row

against the same call without the keyword, on the same tree, in the same process, the settings alternated; the three new launches
alone from the library's event profiler; and -- with ``--parent DIR``, a built checkout of the parent commit -- the call WITHOUT the
keyword on this tree against the parent's, in fresh child processes started in turn (this, parent, this, parent, ...), so that the
difference can be held against the spread between rounds of one and the same tree on that box.

    python tools/time_logprobs.py c2 [report.txt] [--parent DIR]      host clock around device-synchronised calls
    python tools/time_logprobs.py all DIR [--parent DIR]              one fresh child process per model under its own ``timeout``

Prediction from the code: the pick launch reads every logits row once more (dh_beam_row_best does that sweep plus a selection in
51.5 us per 1,280 rows), 32 / 33 times: on the order of +1 ms on C2's 7 ms and C3's 20 ms; the tables are 8 bytes x 33 x 1,280 rows =
338 KB.  Reports land in DIR (``time_logprobs_<model>.txt``).  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, V, REPEATS, ROUNDS = 256, 36541, 10, 3
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}
NEW = ("dh_beam_pick_logprobs", "dh_beam_record_logprobs", "dh_beam_gather_logprobs")


def setup(which, root):
    sys.path.insert(0, root)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    return torch, model.to(dev).bfloat16(), synth_images(N, seed=0).to(dev), dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)


def timed(torch, model, images, kw, variants, repeats):
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
    return times


def plain_only(which, root):
    """Child process: the call without the keyword on the tree at ``root``; one JSON line."""
    torch, model, images, kw = setup(which, root)
    ts = timed(torch, model, images, kw, [("without", {})], REPEATS)["without"]
    import deephumor_amd
    print("PLAIN " + json.dumps({"median": statistics.median(ts), "min": min(ts), "max": max(ts), "package": os.path.dirname(deephumor_amd.__file__)}),
          flush=True)


def against_parent(which, parent):
    """``ROUNDS`` child processes per tree, started in turn -> report lines."""
    me = os.path.abspath(__file__)
    meds = {"this": [], "parent": []}
    for _ in range(ROUNDS):
        for tag, root in (("this", ROOT), ("parent", os.path.abspath(parent))):
            p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, me, "plain", which, root], capture_output=True, text=True)
            if p.returncode != 0:
                return [f"  the {tag} tree's child ended with status {p.returncode}: nothing further is started", p.stderr[-500:]], p.returncode
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("PLAIN ")][-1][6:])
            assert os.path.realpath(rec["package"]).startswith(os.path.realpath(root)), rec["package"]      # each tree ran its own package
            meds[tag].append(rec["median"])
    this, par = statistics.median(meds["this"]), statistics.median(meds["parent"])
    spread = max(max(v) - min(v) for v in meds.values())
    return ["", f"the call WITHOUT the keyword, this tree against the parent commit ({ROUNDS} fresh processes each, started in turn; median ms of "
            f"{REPEATS} calls per process):",
            "  this tree   " + "  ".join(f"{m:8.3f}" for m in meds["this"]) + f"   median {this:8.3f}",
            "  parent      " + "  ".join(f"{m:8.3f}" for m in meds["parent"]) + f"   median {par:8.3f}",
            f"  this - parent: {this - par:+.3f} ms = {100 * (this - par) / par:+.2f} %; largest spread between rounds of one tree: {spread:.3f} ms; "
            f"inside it: {abs(this - par) <= spread}"], 0


def measure(which, report=None, parent=None):
    torch, model, images, kw = setup(which, ROOT)
    from deephumor_amd import hip
    variants = [("without", {}), ("return_logprobs", {"return_logprobs": True}), ("return_beams", {"return_beams": True}),
                ("return_logprobs + beams", {"return_logprobs": True, "return_beams": True}), ("search=beam", {"search": "beam"}),
                ("search=beam + logprobs", {"search": "beam", "return_logprobs": True})]
    times = timed(torch, model, images, kw, variants, REPEATS)
    with torch.no_grad():
        a = model.generate_batch(images, **kw)
        b = model.generate_batch(images, **kw, return_logprobs=True)
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        kernels = {}
        for tag, extra in (("sampled", {}), ('search="beam"', {"search": "beam"})):       # (there the pick launch copies pick_val: no sweep)
            with hip.profile(watch=set(NEW) | {"dh_beam_row_best"}) as prof:
                model.generate_batch(images, **kw, return_logprobs=True, **extra)
            kernels[tag] = prof.summary()
    lines = [f"return_logprobs: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {REPEATS} repeats, the settings alternated inside each repeat; ms per {N} images",
             f"tokens and lengths with the keyword equal the call without it: {same}; logprobs {tuple(b[2].shape)} fp32", ""]
    for name, ts in times.items():
        lines.append(f"  {name:26s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    for on_name, base_name in (("return_logprobs", "without"), ("return_beams", "without"), ("return_logprobs + beams", "return_beams"),
                               ("search=beam + logprobs", "search=beam")):
        on, base = statistics.median(times[on_name]), statistics.median(times[base_name])
        lines.append(f"  {on_name:26s} - {base_name}, medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")
    for tag, summary in kernels.items():
        lines += ["", f"the new launches of one {tag} call with the keyword (HIP events inside the library, around each launch"
                  + ("; dh_beam_row_best, the same sweep plus a selection, beside them):" if "beam" in tag else "):")]
        for key, rec in summary.items():
            lines.append(f"  {key:34s} {rec['calls']:4d} calls  {1e3 * rec['ms'] / max(rec['calls'], 1):8.2f} us each  {rec['ms']:8.3f} ms")
    rc = 0
    if parent:
        del model, images
        torch.cuda.empty_cache()
        more, rc = against_parent(which, parent)
        lines += more
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    return rc


def chain(out_dir, parent):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    for which in KINDS:
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_logprobs_{which}.txt")] + (["--parent", parent] if parent else [])
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", "540"] + cmd).returncode
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        at = args.index("--parent")
        parent = args[at + 1]
        del args[at:at + 2]
    mode = args[0] if args else "c3"
    if mode == "plain":
        plain_only(args[1], args[2])
    elif mode == "all":
        sys.exit(chain(args[1] if len(args) > 1 else ".", parent))
    else:
        sys.exit(measure(mode, args[1] if len(args) > 1 else None, parent))
