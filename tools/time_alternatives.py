"""Times ``experiments.token_alternatives`` on the GPU at the workload's own size: 256 captions of 25 positions over 16 templates,
V = 36,541, hidden size 512 (``CaptioningTransformer`` at its defaults), synthetic weights; bf16, and fp32 with ``f32_split``.

    explain     ``explain_captions`` on the same inputs (the fused routes: no ``[rows, V]`` logits in memory)
    whole       ``token_alternatives(top=5)`` as it ships: the pass's 6,400 logits rows, ONE ``dh_beam_row_best`` launch
    chunk2048   the same with the private ``alternatives._ROW_CHUNK`` at 2,048 / 1,024 / 512 rows per launch
    chunk1024
    chunk512
    bench       ``bench.py --gpus 1 --steps 20 --warmup 5``, the default leg, this tree or the parent's (captions/s)

``group_max`` against NULL is not measured: ``forward``'s classifier (``hip.linear``) leaves no 64-column maxima, so there is nothing to
pass.  Every variant must return the same bits as ``whole`` (asserted), and the first three captions scored alone, one per pass, are
compared with their rows of the full pass: ``BITS same`` / ``BITS differ`` says whether the classifier's choice of kernel by row count
changes a value at this size.

    python tools/time_alternatives.py one DTYPE      every variant in ONE process, in turn inside every repeat: lines ``TIME <what> <median ms>``
    python tools/time_alternatives.py all PARENT DIR ROUNDS rounds, a fresh child process per type and round, then bench.py in this tree and
                                                     in PARENT (a checkout of the parent commit, built) in turn -> DIR/timing.txt

The children start one at a time, each under its own ``timeout``, in a chain: a step that fails, faults or runs out of time ends the
chain and nothing starts after it.  Host clock around device-synchronised calls.  Information, not a gate."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, L, V, REPEATS, ROUNDS = 16, 256, 25, 36541, 7, 3
DTYPES = ("bf16", "f32")
CHUNKS = (2048, 1024, 512)


def one(dtype):
    sys.path.insert(0, ROOT)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd import experiments as X, hip
    from deephumor_amd.experiments import alternatives
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = M.CaptioningTransformer(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    fp32 = dtype == "f32"
    model = model.to(dev) if fp32 else model.to(dev).bfloat16()
    images = synth_images(T, seed=0).to(dev)
    images = images if fp32 else images.bfloat16()
    g = torch.Generator().manual_seed(28)
    lengths = torch.randint(2, L + 1, (N,), generator=g)
    lengths[0] = L
    cap = torch.randint(6, V, (N, L), generator=g)
    cap[torch.arange(L)[None, :] >= lengths[:, None]] = 0
    cap[torch.arange(N), lengths - 1] = 3
    cap, lengths = cap.to(dev), lengths.to(dev)
    index = (torch.arange(N) % T).to(dev)

    def alts(chunk=None, **kw):
        alternatives._ROW_CHUNK = chunk
        try:
            return X.token_alternatives(model, images, kw.pop("index", index), kw.pop("cap", cap), kw.pop("lengths", lengths), top=5, **kw)
        finally:
            alternatives._ROW_CHUNK = None
    calls = {"explain": lambda: X.explain_captions(model, images, index, cap, lengths), "whole": alts}
    for c in CHUNKS:
        calls[f"chunk{c}"] = lambda c=c: alts(c)
    with torch.no_grad(), hip.option_scope(**(dict(f32_split=1) if fp32 else {})):
        whole = alts()
        for c in CHUNKS:
            assert all(torch.equal(a, b) for a, b in zip(whole, alts(c))), c
        alone = alts(index=index[:3], cap=cap[:3], lengths=lengths[:3], batch_size=1)
        same = all(torch.equal(a[:3], b) for a, b in zip(whole, alone))
        apart = float((whole.logprobs[:3] - alone.logprobs).abs().max())
        print(f"BITS {'same' if same else 'differ'} {apart:.3e}", flush=True)
        lp = X.explain_captions(model, images, index, cap, lengths).logprobs
        found = whole.rank >= 0
        mine = whole.logprobs.gather(-1, whole.rank.clamp(min=0).unsqueeze(-1)).squeeze(-1)
        print(f"NOTE top-1 {float((whole.rank == 0).sum()) / float((cap != 0).sum()):.4f} top-5 {float(found.sum()) / float((cap != 0).sum()):.4f} "
              f"vs-explain {float((mine - lp)[found].abs().max()) if bool(found.any()) else 0.0:.3e}", flush=True)
        ts = {k: [] for k in calls}
        for rep in range(2 + REPEATS):                                               # 2 warm-ups, then the variants in turn
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        for k, v in ts.items():
            print(f"TIME {k} {statistics.median(v):.4f}", flush=True)


def child(cmd, limit, cwd=None):
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, text=True, cwd=cwd)
    print(p.stdout, end="", flush=True)
    return p.returncode, p.stdout


def everything(parent, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ms, notes, bench = {}, {}, {"this": [], "parent": []}
    for _ in range(ROUNDS):
        for dtype in DTYPES:                                                         # fresh processes in turn
            rc, out = child([sys.executable, os.path.abspath(__file__), "one", dtype], 420)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            for line in out.splitlines():
                if line.startswith("TIME "):
                    _, what, med = line.split()
                    ms.setdefault((dtype, what), []).append(float(med))
                elif line.startswith(("BITS ", "NOTE ")):
                    notes.setdefault(dtype, set()).add(line)
        for where, tree in (("this", ROOT), ("parent", parent)):
            rc, out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 420, cwd=tree)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            bench[where].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
    lines = [f"token_alternatives(top=5) and explain_captions: CaptioningTransformer, V={V}, hidden 512, {N} captions of {L} positions over {T} "
             f"templates, batch_size 256 (one pass of {N * L} rows); {ROUNDS} rounds, a fresh process per type and round in turn; in a process "
             f"every variant runs in turn inside each of {REPEATS} repeats after 2 warm-ups, median; ms per call, encoder included", ""]
    med = lambda k: statistics.median(ms[k])                                     # noqa: E731
    for key in sorted(ms):
        a = ms[key]
        lines.append(f"  {key[0]:5s} {key[1]:10s} median {statistics.median(a):9.3f}  rounds {min(a):9.3f} .. {max(a):9.3f}  spread {max(a) - min(a):7.3f}")
    lines.append("")
    for dtype in DTYPES:
        w, e = med((dtype, "whole")), med((dtype, "explain"))
        lines.append(f"  {dtype}: whole - explain {w - e:+.3f} ms ({(w / e - 1) * 100:+.1f} %); "
                     + "; ".join(f"chunk{c} - whole {med((dtype, f'chunk{c}')) - w:+.3f} ms" for c in CHUNKS))
        for note in sorted(notes.get(dtype, ())):
            lines.append(f"  {dtype}: {note}")
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
