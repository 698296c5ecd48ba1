"""Times ``experiments.score_pairs`` on the GPU at the workload's own size: 300 templates x 1 and x 16 captions of 25 positions,
V = 36,541, hidden size 512 (``CaptioningTransformer`` at its defaults), synthetic weights; bf16, and fp32 with ``f32_split``.

    shared      score_pairs as it ships: one K|V projection and one packed layout per template of a pass (``_forward``'s ``enc_share``)
    gathered    score_pairs with the private switch ``scoring._SHARE_TEMPLATE_KEYS`` off: the spatial features gathered per pair
    expanded    the same pairs expanded by hand through ``explain_captions`` (template_index = every template ``n`` times, the captions
                repeated 300 times) -- this tree or the parent's
    bench       ``bench.py --gpus 1 --steps 20 --warmup 5``, the default leg, this tree or the parent's (captions/s)

    python tools/time_pairs.py one DTYPE [TREE]      every measurement TREE's package has (default: this tree), in ONE process, the
                                                     variants of a size in turn inside every repeat: lines ``TIME <what> <n> <median ms>``
    python tools/time_pairs.py all PARENT DIR        this tree and PARENT (a checkout of the parent commit, built) in turn, ROUNDS
                                                     rounds, a fresh child process per tree, type and round -> DIR/timing.txt

With one caption per template a pass holds 256 templates of one caption each: nothing is shared and ``shared`` and ``gathered`` are the
same launches (the two lines show the noise of the measurement).  The children start one at a time, each under its own ``timeout``,
in a chain: a step that fails, faults or runs out of time ends the chain and nothing starts after it.  Host clock around
device-synchronised calls.  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, L, V, SIZES, REPEATS, ROUNDS = 300, 25, 36541, (1, 16), 7, 3
DTYPES = ("bf16", "f32")


def one(dtype, tree=ROOT):
    sys.path.insert(0, os.path.abspath(tree))
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
    have_pairs = hasattr(X, "score_pairs")
    with torch.no_grad(), hip.option_scope(**(dict(f32_split=1) if fp32 else {})):
        for n in SIZES:
            g = torch.Generator().manual_seed(11 + n)
            lengths = torch.randint(2, L + 1, (n,), generator=g)
            lengths[0] = L
            cap = torch.randint(6, V, (n, L), generator=g)
            cap[torch.arange(L)[None, :] >= lengths[:, None]] = 0
            cap[torch.arange(n), lengths - 1] = 3
            cap, lengths = cap.to(dev), lengths.to(dev)
            index = torch.arange(T, device=dev).repeat_interleave(n)
            cap_x, len_x = cap.repeat(T, 1), lengths.repeat(T)

            def pairs(shared):
                scoring._SHARE_TEMPLATE_KEYS = shared
                try:
                    return X.score_pairs(model, images, cap, lengths)
                finally:
                    scoring._SHARE_TEMPLATE_KEYS = True
            calls = {"expanded": lambda: X.explain_captions(model, images, index, cap_x, len_x)}
            if have_pairs:
                calls["shared"] = lambda: pairs(True)
                calls["gathered"] = lambda: pairs(False)
                a, b, c = calls["shared"](), calls["gathered"](), calls["expanded"]()
                assert torch.equal(a.perplexity, b.perplexity) and torch.equal(a.logprob, b.logprob)
                assert torch.equal(a.perplexity, c.perplexity.view(T, n).t())           # the same pairs, the same bits
            ts = {k: [] for k in calls}
            for rep in range(2 + REPEATS):                                           # 2 warm-ups, then the variants in turn
                for k, call in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
            for k, v in ts.items():
                print(f"TIME {k} {n} {statistics.median(v):.4f}", flush=True)


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
            for where, tree in (("this", ROOT), ("parent", parent)):             # fresh processes in turn
                rc, out = child([sys.executable, os.path.abspath(__file__), "one", dtype, tree], 420)
                if rc != 0:
                    print(f"step ended with status {rc}: nothing further is started", flush=True)
                    return rc
                for line in out.splitlines():
                    if line.startswith("TIME "):
                        _, what, n, med = line.split()
                        ms.setdefault((dtype, int(n), what, where), []).append(float(med))
        for where, tree in (("this", ROOT), ("parent", parent)):
            rc, out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 420, cwd=tree)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            bench[where].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
    lines = [f"score_pairs: CaptioningTransformer, V={V}, hidden 512, {T} templates x n captions of {L} positions, batch_size 256; {ROUNDS} rounds, "
             f"a fresh process per tree, type and round in turn; in a process every variant of a size runs in turn inside each of {REPEATS} "
             f"repeats after 2 warm-ups, median; ms per call, encoder included", ""]
    med = lambda k: statistics.median(ms[k])                                 # noqa: E731
    for key in sorted(ms):
        a = ms[key]
        lines.append(f"  {key[0]:5s} n={key[1]:<3d} {key[2]:9s} {key[3]:7s} median {statistics.median(a):9.3f}  rounds {min(a):9.3f} .. {max(a):9.3f}"
                     f"  spread {max(a) - min(a):7.3f}")
    lines.append("")
    for dtype in DTYPES:
        for n in SIZES:
            s, g_, e, p = (med((dtype, n, w, t)) for w, t in (("shared", "this"), ("gathered", "this"), ("expanded", "this"), ("expanded", "parent")))
            lines.append(f"  {dtype} n={n}: shared - gathered {s - g_:+.3f} ms; score_pairs - hand expansion {s - e:+.3f} ms (this tree), {s - p:+.3f} ms "
                         f"(the parent's explain_captions); explain_captions this - parent {e - p:+.3f} ms")
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
    one(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ROOT)
