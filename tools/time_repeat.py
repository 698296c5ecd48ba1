"""Times what ``no_repeat_ngram_size`` costs the BASELINE C2 and C3 steps on the GPU: ``generate_batch`` of 256 images, V = 36,541,
bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with ``no_repeat_ngram_size = 3`` against the same call without the
keyword on the same tree -- one extra launch of ``dh_beam_history_logits`` (1,280 workgroups) in front of each of the 32 row draws.

    python tools/time_repeat.py c2|c3 [report.txt]           one model: host clock around device-synchronised calls
    python tools/time_repeat.py all DIR                      both models, one fresh child process each

``all`` starts one child per model, every child under its own ``timeout``, in a chain: a step that fails, faults or runs out of
time ends the chain and nothing starts after it.  Reports land in DIR (``time_repeat_<model>.txt``).  Information, not a gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, REPEATS, NGRAM = 256, 36541, 10, 3
KINDS = {"c2": "CaptioningLSTM", "c3": "CaptioningTransformer"}


def measure(which, report=None, repeats=REPEATS):
    import torch
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).bfloat16()
    images = synth_images(N, seed=0).to(dev)
    kw = dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)
    variants = [("without", {}), (f"no_repeat = {NGRAM}", {"no_repeat_ngram_size": NGRAM})]
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
        b = model.generate_batch(images, **kw, no_repeat_ngram_size=NGRAM)
        differ = int((a[0] != b[0]).any(1).sum())
    lines = [f"no_repeat_ngram_size = {NGRAM}: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the two settings alternated inside each repeat; ms per {N} images",
             f"captions that differ between the two settings: {differ} of {N}", ""]
    for name, ts in times.items():
        lines.append(f"  {name:14s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    base, on = (statistics.median(times[n]) for n, _ in variants)
    lines.append(f"  difference of the medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)


def chain(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    for which in KINDS:
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_repeat_{which}.txt")]
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
