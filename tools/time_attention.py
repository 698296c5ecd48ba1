"""Times what ``return_attention=True`` costs the BASELINE C3 step on the GPU: ``generate_batch`` of 256 images with
``CaptioningTransformer``, V = 36,541, bf16, beam 5, ``top_k`` 50, ``max_len`` 32 (bench.py's settings) with

    return_attention = True                          one launch of dh_attn_cross_weights behind the last layer's fc_q at each of
                                                     the 33 positions, the n-best final draw and one dh_beam_gather_attention
    return_attention + return_beams                  the same launches; every slot's maps are returned, no slot is sliced

against the same call without the keyword (and against ``return_beams=True`` alone), on the same tree, in the same process, the
settings alternated.

    python tools/time_attention.py c3 [report.txt]         host clock around device-synchronised calls
    python tools/time_attention.py all DIR                 one fresh child process under its own ``timeout``

Prediction from the code: 33 + 1 dependent launches at a launch floor of ~8 us, ~+0.3 ms on ~20 ms, and a map buffer of
33 x 1,280 x 49 fp32 = 8.3 MB.  Reports land in DIR (``time_attention_<model>.txt``).  Information, not a gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, REPEATS = 256, 36541, 10
KINDS = {"c3": "CaptioningTransformer"}


def measure(which, report=None, repeats=REPEATS):
    import torch
    import deephumor_amd.models as M
    from deephumor_amd import hip
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, KINDS[which])(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).bfloat16()
    images = synth_images(N, seed=0).to(dev)
    kw = dict(max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)
    variants = [("without", {}), ("return_attention", {"return_attention": True}), ("return_beams", {"return_beams": True}),
                ("return_attention + beams", {"return_attention": True, "return_beams": True})]
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
        b = model.generate_batch(images, **kw, return_attention=True)
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # the two new launches by themselves, from the library's own event profiler
        with hip.profile(watch={"dh_attn_cross_weights", "dh_beam_gather_attention", "dh_attn_cross_decode"}) as prof:
            model.generate_batch(images, **kw, return_attention=True)
        kernels = prof.summary()
    lines = [f"return_attention: {KINDS[which]} ({which.upper()}), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"device: {torch.cuda.get_device_name(0)}; date: {time.strftime('%Y-%m-%d')}; host clock around device-synchronised "
             f"generate_batch calls; 3 warm-up rounds, {repeats} repeats, the settings alternated inside each repeat; ms per {N} images",
             f"tokens and lengths with the keyword equal the call without it: {same}; maps {tuple(b[2].shape)} fp32 = "
             f"{b[2].numel() * 4 / 1e6:.1f} MB", ""]
    for name, ts in times.items():
        lines.append(f"  {name:26s} median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}")
    for on_name, base_name in (("return_attention", "without"), ("return_beams", "without"), ("return_attention + beams", "return_beams")):
        on, base = statistics.median(times[on_name]), statistics.median(times[base_name])
        lines.append(f"  {on_name:26s} - {base_name}, medians: {on - base:+.3f} ms = {100 * (on - base) / base:+.2f} %")
    lines += ["", "launches of one call with the keyword (HIP events inside the library, around each launch):"]
    for key, rec in kernels.items():
        lines.append(f"  {key:34s} {rec['calls']:4d} calls  {1e3 * rec['ms'] / max(rec['calls'], 1):8.2f} us each  {rec['ms']:8.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text)


def chain(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    me = os.path.abspath(__file__)
    for which in KINDS:
        cmd = [sys.executable, me, which, os.path.join(out_dir, f"time_attention_{which}.txt")]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(["timeout", "-k", "10", "240"] + cmd).returncode
        if rc != 0:
            print(f"step ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "c3"
    if mode == "all":
        sys.exit(chain(sys.argv[2] if len(sys.argv) > 2 else "."))
    measure(mode, sys.argv[2] if len(sys.argv) > 2 else None)
