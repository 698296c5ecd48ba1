"""Times what nucleus filtering (``top_p < 1``) costs the BASELINE C2 and C3 steps on the GPU: ``generate_batch`` of 256 images,
V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with ``top_p = 0.9`` against ``top_p = 1.0`` of the same
tree -- 1,280 rows x 36,541 logits per row draw, the group-guided sampler with and without the rank sort and the block scan.

    python tools/time_nucleus.py c2|c3 [report.txt]          one model: host clock around device-synchronised calls
    python tools/time_nucleus.py all DIR                     both models, then each again under rocprofv3 for the row sampler alone

``all`` starts one fresh child process per step (``c2``, ``c3``, then ``rocprofv3 --kernel-trace --stats`` around each), every
child under its own ``timeout``, in a chain: a step that fails, faults or runs out of time ends the chain and nothing starts after
it.  Reports land in DIR (``time_nucleus_<model>.txt``, ``rocprof_<model>/``); the row-sampler lines of the kernel statistics are
appended to the model's report.  Information, not a gate."""
import glob
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, REPEATS, TOP_P = 256, 36541, 10, 0.9
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
    variants = [("top_p = 1.0", {}), (f"top_p = {TOP_P}", {"top_p": TOP_P})]
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
        b = model.generate_batch(images, **kw, top_p=TOP_P)
        differ = int((a[0] != b[0]).any(1).sum())
    lines = [f"nucleus filtering: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the two settings alternated inside each repeat; ms per {N} images",
             f"captions that differ between the two settings: {differ} of {N}", ""]
    for name, ts in times.items():
        lines.append(f"  {name:14s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    base, nuc = (statistics.median(times[n]) for n, _ in variants)
    lines.append(f"  difference of the medians: {nuc - base:+.3f} ms = {100 * (nuc - base) / base:+.2f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)


def chain(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    steps = []
    for which in KINDS:
        steps.append((240, [sys.executable, me, which, os.path.join(out_dir, f"time_nucleus_{which}.txt")], None))
    for which in KINDS:
        prof = os.path.join(out_dir, f"rocprof_{which}")
        steps.append((420, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", sys.executable, me,
                            which + "-short"], (which, prof)))
    for limit, cmd, after in steps:
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
        if after is not None:
            which, prof = after
            rows = []
            for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    head = f.readline().strip()
                    rows = [head] + [ln.strip() for ln in f if "beam_row_sample" in ln]
            with open(os.path.join(out_dir, f"time_nucleus_{which}.txt"), "a") as f:
                f.write("\nrow-sampler kernels under rocprofv3 --kernel-trace --stats (3 warm-up + 3 timed calls of each setting):\n")
                f.write("\n".join(rows) + "\n" if rows else "no kernel statistics were written\n")
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
    if mode == "all":
        sys.exit(chain(sys.argv[2] if len(sys.argv) > 2 else "."))
    if mode.endswith("-short"):
        measure(mode[:-6], repeats=3)
    else:
        measure(mode, sys.argv[2] if len(sys.argv) > 2 else None)
