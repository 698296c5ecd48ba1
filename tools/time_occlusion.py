"""Times ``experiments.occlusion_maps`` on the GPU at the workload's own size: 300 templates x 16 captions of 25 positions, V = 36,541,
hidden size 512 (``CaptioningTransformer`` at its defaults), synthetic weights; bf16, and fp32 with ``f32_split``.

    copied      level="patch" as it ships: one K|V projection and one packed layout per template, copied on the device for the variants
                of a pass, the hidden rows on the key mask (``_forward``'s ``enc_hide``)
    pervariant  level="patch" with the private switch ``scoring._COPY_VARIANT_KEYS`` off: the variants' features with their rows zeroed,
                projected and packed per variant
    expanded    the same 300 x 50 variants expanded by hand through ``explain_captions``: their features (the zeroed rows written out)
                behind a stand-in encoder, template_index = every variant 16 times
    pixel       level="pixel", grid (7, 7): the encoder on 300 x 50 images, then the same decoder passes
    bench       ``bench.py --gpus 1 --steps 20 --warmup 5``, the default leg, this tree or the parent's (captions/s)

    python tools/time_occlusion.py one DTYPE         every measurement in ONE process, the variants in turn inside every repeat: lines
                                                     ``TIME <what> <median ms>``
    python tools/time_occlusion.py all PARENT DIR    ROUNDS rounds, a fresh child process per type and round in turn, then bench.py of
                                                     this tree and of PARENT (a checkout of the parent commit, built) -> DIR/timing.txt

The children start one at a time, each under its own ``timeout``, in a chain: a step that fails, faults or runs out of time ends the
chain and nothing starts after it.  Host clock around device-synchronised calls.  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, L, V, S, GRID, REPEATS, ROUNDS = 300, 16, 25, 36541, 49, (7, 7), 3, 3
DTYPES = ("bf16", "f32")


def one(dtype):
    sys.path.insert(0, ROOT)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd import experiments as X, hip
    from deephumor_amd.experiments import scoring
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = M.CaptioningTransformer(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    fp32 = dtype == "f32"
    model = model.to(dev) if fp32 else model.to(dev).bfloat16()
    images = synth_images(T, seed=0).to(dev)
    images = images if fp32 else images.bfloat16()
    with torch.no_grad(), hip.option_scope(**(dict(f32_split=1) if fp32 else {})):
        g = torch.Generator().manual_seed(11 + N)
        lengths = torch.randint(2, L + 1, (N,), generator=g)
        lengths[0] = L
        cap = torch.randint(6, V, (N, L), generator=g)
        cap[torch.arange(L)[None, :] >= lengths[:, None]] = 0
        cap[torch.arange(N), lengths - 1] = 3
        cap, lengths = cap.repeat(T, 1).to(dev), lengths.repeat(T).to(dev)           # template-major: 16 captions per template
        index = torch.arange(T, device=dev).repeat_interleave(N)

        def patch(copied):
            scoring._COPY_VARIANT_KEYS = copied
            try:
                return X.occlusion_maps(model, images, index, cap, lengths)
            finally:
                scoring._COPY_VARIANT_KEYS = True

        # the hand expansion: variant v of template t is pseudo-template t * 50 + v; its captions are the template's 16
        feats, spatial = model.encoder(images)
        hide = torch.cat([torch.zeros((1, S), dtype=torch.bool, device=dev), torch.eye(S, dtype=torch.bool, device=dev)])
        feats_x = feats.repeat_interleave(1 + S, 0)
        spatial_x = spatial.repeat_interleave(1 + S, 0).masked_fill(hide.repeat(T, 1).unsqueeze(-1), 0.0)
        stand_in = types.SimpleNamespace(encoder=lambda _: (feats_x, spatial_x), decoder=model.decoder)
        index_x = torch.arange(T * (1 + S), device=dev).repeat_interleave(N)
        cap_x = cap.view(T, 1, N, L).expand(T, 1 + S, N, L).reshape(-1, L)
        len_x = lengths.view(T, 1, N).expand(T, 1 + S, N).reshape(-1)
        dummy = torch.empty((T * (1 + S), 1), device=dev)
        calls = {"copied": lambda: patch(True), "pervariant": lambda: patch(False),
                 "expanded": lambda: X.explain_captions(stand_in, dummy, index_x, cap_x, len_x),
                 "pixel": lambda: X.occlusion_maps(model, images, index, cap, lengths, level="pixel", grid=GRID)}
        a, b, c = calls["copied"](), calls["pervariant"](), calls["expanded"]()
        assert torch.equal(a.base, b.base) and torch.equal(a.drop, b.drop)            # the same bits on both routes
        sums = c.logprobs.sum(-1, dtype=torch.float64).view(T, 1 + S, N)
        assert torch.equal(a.drop.view(T, N, S), (sums[:, :1] - sums[:, 1:]).float().transpose(1, 2))     # and by hand
        del a, b, c, sums
        ts = {k: [] for k in calls}
        for rep in range(1 + REPEATS):                                               # 1 warm-up, then the variants in turn
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if rep >= 1:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        for k, v in ts.items():
            print(f"TIME {k} {statistics.median(v):.3f}", flush=True)


def child(cmd, limit, cwd=None):
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, text=True, cwd=cwd)
    print(p.stdout, end="", flush=True)
    return p.returncode, p.stdout


def everything(parent, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ms, bench = {}, {"this": [], "parent": []}
    for _ in range(ROUNDS):
        for dtype in DTYPES:
            rc, out = child([sys.executable, os.path.abspath(__file__), "one", dtype], 300)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            for line in out.splitlines():
                if line.startswith("TIME "):
                    _, what, med = line.split()
                    ms.setdefault((dtype, what), []).append(float(med))
        for where, tree in (("this", ROOT), ("parent", parent)):
            rc, out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 300, cwd=tree)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            bench[where].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])
    lines = [f"occlusion_maps: CaptioningTransformer, V={V}, hidden 512, {T} templates x {N} captions of {L} positions, batch_size 256; patch level "
             f"{S} regions, pixel level grid {GRID}; {ROUNDS} rounds, a fresh process per type and round in turn; in a process every variant runs in "
             f"turn inside each of {REPEATS} repeats after 1 warm-up, median; ms per call, encoder included", ""]
    med = lambda k: statistics.median(ms[k])                                 # noqa: E731
    for key in sorted(ms):
        a = ms[key]
        lines.append(f"  {key[0]:5s} {key[1]:10s} median {statistics.median(a):10.2f}  rounds {min(a):10.2f} .. {max(a):10.2f}  spread {max(a) - min(a):8.2f}")
    lines.append("")
    for dtype in DTYPES:
        c, p, e = (med((dtype, w)) for w in ("copied", "pervariant", "expanded"))
        lines.append(f"  {dtype}: copied - pervariant {c - p:+.2f} ms; copied - hand expansion {c - e:+.2f} ms")
    lines += ["", "  bench.py --gpus 1 --steps 20 --warmup 5 (default leg, captions/s):"]
    for where in ("this", "parent"):
        a = bench[where]
        lines.append(f"    {where:7s} median {statistics.median(a):10.1f}  rounds {min(a):10.1f} .. {max(a):10.1f}  spread {max(a) - min(a):8.1f}")
    lines.append(f"    this / parent {statistics.median(bench['this']) / statistics.median(bench['parent']):.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out_dir, "timing.txt"), "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "all":
        sys.exit(everything(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else "."))
    one(sys.argv[2])
