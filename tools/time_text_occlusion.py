"""Times ``experiments.text_occlusion(level="history")`` on the GPU at the workload's own size: 256 captions of 25 positions over 16
templates, V = 36,541 (``CaptioningTransformer`` and ``CaptioningLSTM`` at their defaults), synthetic weights; bf16, and fp32 with
``f32_split``.

    history     ``text_occlusion(level="history", return_tokens=True)`` as it ships: the base sequences and the real variants in passes
                of 256 sequences, decoder inputs edited, targets the original captions
    by_hand     the yardstick that exists without this feature: the same variants written out by hand as edited captions (built with
                the same tensor operations, inside the timed call) through ``explain_captions``, then the differences taken from its rows
    bench       ``bench.py --gpus 1 --steps 20 --warmup 5``, the default leg, this tree or the parent's (captions/s)

``by_hand`` must give the same bits as ``history`` behind every region (asserted).  ``NOTE redundant``: the share of the computed
(sequence, position) rows that causality makes redundant -- positions ``p <= j`` of variant ``j``, which equal the base row; what a
prefix-sharing route could save.

    python tools/time_text_occlusion.py one KIND DTYPE   both variants in ONE process, in turn inside every repeat: lines ``TIME <what> <median ms>``
    python tools/time_text_occlusion.py all PARENT DIR   ROUNDS rounds, a fresh child process per kind, type and round, then bench.py in this tree
                                                         and in PARENT (a checkout of the parent commit, built) in turn -> DIR/timing.txt

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
KINDS = ("CaptioningTransformer", "CaptioningLSTM")
DTYPES = ("bf16", "f32")


def one(kind, dtype):
    sys.path.insert(0, ROOT)
    import torch
    import deephumor_amd.models as M
    from deephumor_amd import experiments as X, hip
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = getattr(M, kind)(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    fp32 = dtype == "f32"
    model = model.to(dev) if fp32 else model.to(dev).bfloat16()
    images = synth_images(T, seed=0).to(dev)
    images = images if fp32 else images.bfloat16()
    g = torch.Generator().manual_seed(29)
    lengths = torch.randint(2, L + 1, (N,), generator=g)
    lengths[0] = L
    cap = torch.randint(6, V, (N, L), generator=g)
    cap[torch.arange(L)[None, :] >= lengths[:, None]] = 0
    cap[torch.arange(N), lengths - 1] = 3
    cap, lengths = cap.to(dev), lengths.to(dev)
    index = (torch.arange(N) % T).to(dev)

    def history():
        return X.text_occlusion(model, images, index, cap, lengths, return_tokens=True)

    def by_hand():
        """Every sequence as a caption of its own: caption i, then its copies with column j < lengths[i] - 1 set to the pad."""
        owner = torch.repeat_interleave(torch.arange(N, device=dev), lengths)
        region = torch.arange(owner.shape[0], device=dev) - (torch.cumsum(lengths, 0) - lengths)[owner] - 1
        edited = cap[owner].clone()
        rows = (region >= 0).nonzero().squeeze(1)
        edited[rows, region[rows]] = 0
        lp = X.explain_captions(model, images, index[owner], edited, lengths[owner]).logprobs
        base = lp[region < 0]
        diff = (base[owner[rows]].double() - lp[rows].double()).float()                # [variants, L]; positions p <= j are not meaningful
        return owner[rows], region[rows], diff

    with torch.no_grad(), hip.option_scope(**(dict(f32_split=1) if fp32 else {})):
        got = history()
        owner, region, diff = by_hand()
        behind = (torch.arange(L, device=dev)[None, :] > region[:, None]) & (torch.arange(L, device=dev)[None, :] < lengths[owner][:, None])
        same = torch.equal(got.token_drop[owner, :, region][behind], diff[behind])
        assert same, "by_hand and history differ"
        n_seq = int(lengths.sum())
        redundant = int((region + 1).sum())
        print(f"NOTE sequences {n_seq} passes {(n_seq + 255) // 256} redundant {redundant / (n_seq * L):.4f} of {n_seq * L} rows (pads "
              f"{1 - int((lengths * lengths).sum()) / (n_seq * L):.4f})", flush=True)
        calls = {"history": history, "by_hand": by_hand}
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
        for kind in KINDS:
            for dtype in DTYPES:                                                     # fresh processes in turn
                rc, out = child([sys.executable, os.path.abspath(__file__), "one", kind, dtype], 300)
                if rc != 0:
                    print(f"step ended with status {rc}: nothing further is started", flush=True)
                    return rc
                for line in out.splitlines():
                    if line.startswith("TIME "):
                        _, what, med = line.split()
                        ms.setdefault((kind, dtype, what), []).append(float(med))
                    elif line.startswith("NOTE "):
                        notes.setdefault((kind, dtype), set()).add(line)
        for where, tree in (("this", ROOT), ("parent", parent)):
            rc, out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 420, cwd=tree)
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            bench[where].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
    lines = [f'text_occlusion(level="history", return_tokens=True) and the same variants by hand through explain_captions: V={V}, {N} captions '
             f"of {L} positions over {T} templates, batch_size 256; {ROUNDS} rounds, a fresh process per kind, type and round in turn; in a "
             f"process both variants run in turn inside each of {REPEATS} repeats after 2 warm-ups, median; ms per call, encoder included", ""]
    med = lambda k: statistics.median(ms[k])                                     # noqa: E731
    for key in sorted(ms):
        a = ms[key]
        lines.append(f"  {key[0]:22s} {key[1]:5s} {key[2]:8s} median {statistics.median(a):9.3f}  rounds {min(a):9.3f} .. {max(a):9.3f}  "
                     f"spread {max(a) - min(a):7.3f}")
    lines.append("")
    for kind in KINDS:
        for dtype in DTYPES:
            h, b = med((kind, dtype, "history")), med((kind, dtype, "by_hand"))
            lines.append(f"  {kind} {dtype}: history - by_hand {h - b:+.3f} ms ({(h / b - 1) * 100:+.1f} %)")
            for note in sorted(notes.get((kind, dtype), ())):
                lines.append(f"  {kind} {dtype}: {note}")
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
    one(sys.argv[2], sys.argv[3])
