"""Times what ``num_beam_groups`` costs the BASELINE C2 / C3 steps on the GPU: ``generate_batch`` of 256 images with
``CaptioningLSTM`` / ``CaptioningTransformer``, V = 36,541, bf16, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) at beam 6 -- the
smallest beam that 2, 3 and 6 groups all divide -- with

    search="beam", num_beam_groups=G, diversity_penalty=0.5      dh_beam_select_groups in place of dh_beam_select_best, G in 2, 3, 6

against ``search="beam"`` without them, on the same tree, in the same process, the settings alternated; the select launches alone from
the library's event profiler, ``dh_beam_select_best_norm`` (``length_penalty=1.0``) beside them in the same run; and -- with ``--parent
DIR``, a built checkout of the parent commit -- the call WITHOUT the keywords (bench.py's own: sampled, beam 5) on this tree against
the parent's, in fresh child processes started in turn (this, parent, this, parent, ...), so that the difference can be held against
the spread between rounds of one and the same tree on that box.

    python tools/time_beam_groups.py c2 [report.txt] [--parent DIR]      host clock around device-synchronised calls
    python tools/time_beam_groups.py all DIR [--parent DIR]              one fresh child process per model under its own ``timeout``

Expectation from the code: the select is a ~10 us single-wave launch on a latency-bound chain; the groups add a short sequential loop
inside that wave (per group a count, a rank over the group's candidates and three wave-local hand-overs), so a cost of the order of
``length_penalty``'s.  Reports land in DIR (``time_beam_groups_<model>.txt``).  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, V, REPEATS, ROUNDS, BEAM, LAM = 256, 36541, 10, 3, 6, 0.5
GROUPS = (2, 3, 6)
CHILD_LIMIT = 150                                   # seconds for one fresh child of ``against_parent``
MODEL_LIMIT = 300 + 2 * ROUNDS * CHILD_LIMIT        # one model's own timing runs, then 2 * ROUNDS children one after the other
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}
SELECTS = ("dh_beam_select_best", "dh_beam_select_best_norm", "dh_beam_select_groups")


def setup(which, root, beam):
    sys.path.insert(0, root)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    return torch, model.to(dev).bfloat16(), synth_images(N, seed=0).to(dev), dict(max_len=32, beam_size=beam, top_k=50, temperature=1.0, seed=7)


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
    """Child process: the call without the keywords (sampled, beam 5) on the tree at ``root``; one JSON line."""
    torch, model, images, kw = setup(which, root, 5)
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
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, me, "plain", which, root], capture_output=True, text=True)
            if p.returncode != 0:
                return [f"  the {tag} tree's child ended with status {p.returncode}: nothing further is started", p.stderr[-500:]], p.returncode
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("PLAIN ")][-1][6:])
            assert os.path.realpath(rec["package"]).startswith(os.path.realpath(root)), rec["package"]      # each tree ran its own package
            meds[tag].append(rec["median"])
    this, par = statistics.median(meds["this"]), statistics.median(meds["parent"])
    spread = max(max(v) - min(v) for v in meds.values())
    return ["", f"the call WITHOUT the keywords (sampled, beam 5), this tree against the parent commit ({ROUNDS} fresh processes each, started in "
            f"turn; median ms of {REPEATS} calls per process):",
            "  this tree   " + "  ".join(f"{m:8.3f}" for m in meds["this"]) + f"   median {this:8.3f}",
            "  parent      " + "  ".join(f"{m:8.3f}" for m in meds["parent"]) + f"   median {par:8.3f}",
            f"  this - parent: {this - par:+.3f} ms = {100 * (this - par) / par:+.2f} %; largest spread between rounds of one tree: {spread:.3f} ms; "
            f"inside it: {abs(this - par) <= spread}"], 0


def measure(which, report=None, parent=None):
    torch, model, images, kw = setup(which, ROOT, BEAM)
    from deephumor_amd import hip
    groups_kw = lambda g: {"search": "beam", "num_beam_groups": g, "diversity_penalty": LAM}
    variants = [("search=beam", {"search": "beam"}), ("search=beam + 1 group", {"search": "beam", "num_beam_groups": 1})]
    variants += [(f"search=beam + {g} groups", groups_kw(g)) for g in GROUPS]
    variants += [("search=beam + penalty 1.0", {"search": "beam", "length_penalty": 1.0})]
    times = timed(torch, model, images, kw, variants, REPEATS)
    facts = []
    with torch.no_grad():
        a = model.generate_batch(images, **kw, search="beam", return_beams=True)
        one = model.generate_batch(images, **kw, search="beam", return_beams=True, num_beam_groups=1)
        one_same = all(bool(torch.equal(x, y)) for x, y in zip(a, one))
        for g in GROUPS:
            b = model.generate_batch(images, **kw, return_beams=True, **groups_kw(g))
            bg = BEAM // g
            # distinct first words among the best beam of every group, against the plain n-best list's first g rows
            order = torch.argsort(b.beam_index // bg, dim=1, stable=True)[:, ::bg]              # each group's first (best) slot
            firsts = torch.gather(b.tokens[:, :, 0], 1, order)
            distinct = sum(len(set(r)) for r in firsts.tolist()) / N
            plain_distinct = sum(len(set(r)) for r in a.tokens[:, :g, 0].tolist()) / N
            moved = int((a.tokens[:, 0] != b.tokens[:, 0]).any(-1).sum())
            facts.append(f"  {g} groups: distinct first tokens among the groups' best beams {distinct:.2f} of {g} per image (the plain list's first "
                         f"{g} rows: {plain_distinct:.2f}); slot 0 differs from the plain search in {moved} / {N} images; any <eos> written: "
                         f"{bool((b.lengths < b.row_lengths[:, None]).any())}")
        kernels = {}
        for tag, extra in [('search="beam"', {"search": "beam"}), ('search="beam", length_penalty=1.0', {"search": "beam", "length_penalty": 1.0})] + \
                [(f'search="beam", num_beam_groups={g}', groups_kw(g)) for g in GROUPS]:
            with hip.profile(watch=set(SELECTS) | {"dh_beam_row_best"}) as prof:
                model.generate_batch(images, **kw, **extra)
            kernels[tag] = prof.summary()
    lines = [f"num_beam_groups: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam {BEAM}, max_len 32, top_k 50, diversity_penalty {LAM}",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {REPEATS} repeats, the settings alternated inside each repeat; ms per {N} images",
             f"num_beam_groups=1 returns the bits of the call without it: {one_same}"] + facts + [""]
    for name, ts in times.items():
        lines.append(f"  {name:28s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    base = statistics.median(times["search=beam"])
    for name in times:
        if name != "search=beam":
            on = statistics.median(times[name])
            lines.append(f"  {name:28s} - search=beam, medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")
    for tag, summary in kernels.items():
        lines += ["", f"the select launch of one {tag} call (HIP events inside the library, around each launch; dh_beam_row_best beside it):"]
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
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_beam_groups_{which}.txt")] + (["--parent", parent] if parent else [])
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", str(MODEL_LIMIT)] + cmd).returncode
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
