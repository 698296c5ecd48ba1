"""Times what ``early_stopping`` costs -- and where it can pay -- on the BASELINE C2 / C3 steps on the GPU: ``generate_batch`` of 256
images with ``CaptioningLSTM`` / ``CaptioningTransformer``, V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings)
with

    search="beam", early_stopping=True / False       dh_beam_select_pool in place of the select at every position, dh_beam_finalize_pool
                                                      at the end

against ``search="beam"`` without it, on the same tree, in the same process, the settings alternated; ``dh_beam_select_pool`` per launch
beside ``dh_beam_select_best_norm`` from the library's event profiler in the same run; the same on weights with the ``<eos>`` bias
raised (``<eos>`` ``BOOST_ABOVE`` logits above the rows' best token where it comes closest), with and without ``early_stop_every`` --
the only case where stopping early can pay, reported as measured on THOSE weights --; and, with ``--parent DIR``, a built checkout of
the parent commit, the call WITHOUT the keyword on this tree against the parent's, in fresh child processes started in turn (this,
parent, this, parent, ...), so that the difference can be held against the spread between rounds of one and the same tree on that box.

    python tools/time_early_stopping.py c2 [report.txt] [--parent DIR]      host clock around device-synchronised calls
    python tools/time_early_stopping.py all DIR [--parent DIR]              one fresh child process per model under its own ``timeout``

On the benchmark's synthetic weights no beam meets ``<eos>`` within 32 tokens: there the run times the launches, not a change of
captions.  Reports land in DIR (``time_early_stopping_<model>.txt``).  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, V, REPEATS, ROUNDS, EOS = 256, 36541, 10, 3, 3
BOOST_ABOVE = 0.5                                   # (3.0 ends every caption at its first token: nothing left to time)
POLL = 4                                            # early_stop_every of the boosted runs
CHILD_LIMIT = 150                                   # seconds for one fresh child of ``against_parent``
MODEL_LIMIT = 300 + 2 * ROUNDS * CHILD_LIMIT        # one model's own timing runs, then 2 * ROUNDS children one after the other
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}
SELECTS = ("dh_beam_select_best", "dh_beam_select_best_norm", "dh_beam_select_pool", "dh_beam_finalize_beams", "dh_beam_finalize_pool")


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
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, me, "plain", which, root], capture_output=True, text=True)
            if p.returncode != 0:
                return [f"  the {tag} tree's child ended with status {p.returncode}: nothing further is started", p.stderr[-500:]], p.returncode
            rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("PLAIN ")][-1][6:])
            assert os.path.realpath(rec["package"]).startswith(os.path.realpath(root)), rec["package"]      # each tree ran its own package
            meds[tag].append(rec["median"])
    this, par = statistics.median(meds["this"]), statistics.median(meds["parent"])
    spread = max(max(v) - min(v) for v in meds.values())
    return ["", f"the call WITHOUT the keyword, this tree against the parent commit ({ROUNDS} fresh processes each, started in turn; median ms "
            f"of {REPEATS} calls per process):",
            "  this tree   " + "  ".join(f"{m:8.3f}" for m in meds["this"]) + f"   median {this:8.3f}",
            "  parent      " + "  ".join(f"{m:8.3f}" for m in meds["parent"]) + f"   median {par:8.3f}",
            f"  this - parent: {this - par:+.3f} ms = {100 * (this - par) / par:+.2f} %; largest spread between rounds of one tree: {spread:.3f} ms; "
            f"inside it: {abs(this - par) <= spread}"], 0


def table(lines, times, pairs):
    for name, ts in times.items():
        lines.append(f"  {name:40s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    for on_name, base_name in pairs:
        on, base = statistics.median(times[on_name]), statistics.median(times[base_name])
        lines.append(f"  {on_name:40s} - {base_name}, medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")


def measure(which, report=None, parent=None):
    torch, model, images, kw = setup(which, ROOT)
    from deephumor_amd import hip
    beam = {"search": "beam"}
    variants = [("without", {}), ("search=beam", beam), ("search=beam + early_stopping=True", dict(beam, early_stopping=True)),
                ("search=beam + early_stopping=False", dict(beam, early_stopping=False)),
                ("search=beam + early_stopping=None", dict(beam, early_stopping=None))]
    times = timed(torch, model, images, kw, variants, REPEATS)
    with torch.no_grad():
        a = model.generate_batch(images, **kw, search="beam", return_beams=True)
        z = model.generate_batch(images, **kw, search="beam", return_beams=True, early_stopping=None)
        same = {m: all(bool(torch.equal(x, y)) for x, y in zip(a, model.generate_batch(images, **kw, search="beam", return_beams=True, early_stopping=m)))
                for m in (True, False)}
        none_same = all(bool(torch.equal(x, y)) for x, y in zip(a, z))
        kernels = {}
        for tag, extra in (('search="beam", length_penalty=1.0', {"length_penalty": 1.0}),
                           ('search="beam", length_penalty=1.0, early_stopping=False', {"length_penalty": 1.0, "early_stopping": False})):
            with hip.profile(watch=set(SELECTS) | {"dh_beam_row_best"}) as prof:
                model.generate_batch(images, **kw, search="beam", **extra)
            kernels[tag] = prof.summary()
    lines = [f"early_stopping: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {REPEATS} repeats, the settings alternated inside each repeat; ms per {N} images",
             f"early_stopping=None returns the bits of the call without it: {none_same}; no beam meets <eos> on these weights "
             f"({int((a.tokens == EOS).sum())} <eos> tokens returned), so True / False return the bits of search=\"beam\": {same[True]} / {same[False]}", ""]
    table(lines, times, (("search=beam + early_stopping=True", "search=beam"), ("search=beam + early_stopping=False", "search=beam"),
                         ("search=beam + early_stopping=None", "search=beam"), ("search=beam", "without")))
    for tag, summary in kernels.items():
        lines += ["", f"the select and final launches of one {tag} call (HIP events inside the library, around each launch; dh_beam_row_best beside them):"]
        for key, rec in summary.items():
            lines.append(f"  {key:34s} {rec['calls']:4d} calls  {1e3 * rec['ms'] / max(rec['calls'], 1):8.2f} us each  {rec['ms']:8.3f} ms")
    # ---- weights with the <eos> bias raised: the only case where stopping early can pay
    seen = []
    with torch.no_grad():
        model.generate_batch(images, **kw, search="beam", logits_hook=lambda pos, lg: seen.append(float((lg.float().max(1).values - lg[:, EOS].float()).median())))
        gap = min(seen)
        bias = model.decoder.classifier.bias
        bias[EOS] += gap + BOOST_ABOVE                     # (in place: the version counter moves, the weight plan is rebuilt)
    boosted = [("boosted: search=beam", beam), ("boosted: + early_stopping=True", dict(beam, early_stopping=True)),
               (f"boosted: + True, early_stop_every={POLL}", dict(beam, early_stopping=True, early_stop_every=POLL)),
               ("boosted: + early_stopping=False", dict(beam, early_stopping=False)),
               (f"boosted: + False, early_stop_every={POLL}", dict(beam, early_stopping=False, early_stop_every=POLL))]
    btimes = timed(torch, model, images, kw, boosted, REPEATS)
    with torch.no_grad():
        facts = {}
        for name, extra in boosted:
            got = model.generate_batch(images, **kw, return_beams=True, **{k: v for k, v in extra.items() if k != "early_stop_every"})
            facts[name] = (float(got.lengths[:, 0].float().mean()), int((got.beam_index[:, 0] < 0).sum()))
        polled = model.generate_batch(images, **kw, return_beams=True, search="beam", early_stopping=True, early_stop_every=POLL)
        plain = model.generate_batch(images, **kw, return_beams=True, search="beam", early_stopping=True)
        poll_same = all(bool(torch.equal(x, y)) for x, y in zip(polled, plain))
    lines += ["", f"the same on weights with the <eos> bias raised by {gap + BOOST_ABOVE:.3f} (<eos> {BOOST_ABOVE} logits above the rows' best token where it "
              f"comes closest; measured on THESE weights, not a headline).  The poll returns the bits of the call without it: {poll_same}"]
    table(lines, btimes, ((boosted[1][0], boosted[0][0]), (boosted[2][0], boosted[0][0]), (boosted[2][0], boosted[1][0]),
                          (boosted[3][0], boosted[0][0]), (boosted[4][0], boosted[3][0])))
    for name, (ln, pooled) in facts.items():
        lines.append(f"  {name:40s} mean length of slot 0: {ln:6.2f}; slot 0 came from the pool in {pooled} / {N} images")
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
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_early_stopping_{which}.txt")] + (["--parent", parent] if parent else [])
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
