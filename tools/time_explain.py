"""Times ``experiments.explain_captions`` on the GPU: 256 captions of L = 25 positions over 8 templates, V = 36,541, hidden size 512
(``CaptioningTransformer`` at its defaults), synthetic weights.

    fp32-fused     explain_captions, fp32, option f32_split on: hidden states -> dh_vocab_logprob(DH_F32), no logits in memory
    fp32-logits    the same call forced onto the logits route (forward, split classifier included, -> dh_token_logprob)
    fp32-score     fp32 score_captions (option f32_split on), this tree or the parent's
    bf16 / bf16-attn   explain_captions in bf16 without / with return_attention
    score / generate   the plain calls in bf16: score_captions on the same captions; generate_batch of 256 images, beam 5, max_len 32

    python tools/time_explain.py one WHAT [TREE]     one measurement in this process on TREE's package (default: this tree): a line
                                                     ``TIME <what> <median ms> <peak allocated bytes>``
    python tools/time_explain.py all PARENT DIR      everything, this tree and PARENT (a checkout of the parent commit, built) in
                                                     turn, ROUNDS rounds, a fresh child process per measurement -> DIR/timing.txt

The children start one at a time, each under its own ``timeout``, in a chain: a step that fails, faults or runs out of time ends the
chain and nothing starts after it.  Host clock around device-synchronised calls; peak = ``torch.cuda.max_memory_allocated`` over
the timed calls.  Information, not a gate."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, T, V, REPEATS, ROUNDS = 256, 25, 8, 36541, 10, 3
PLAN = (("fp32-fused", "this"), ("fp32-logits", "this"), ("fp32-score", "parent"), ("bf16", "this"),
        ("bf16-attn", "this"), ("score", "this"), ("score", "parent"), ("generate", "this"), ("generate", "parent"))


def one(what, tree=ROOT):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import deephumor_amd.models as M
    from deephumor_amd import experiments as X, hip
    from deephumor_amd.synth import synth_images, synth_state_dict
    dev = torch.device("cuda", 0)
    model = M.CaptioningTransformer(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    fp32 = what.startswith("fp32")
    model = model.to(dev) if fp32 else model.to(dev).bfloat16()
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(2, L + 1, (N,), generator=g)
    lengths[0] = L
    cap = torch.randint(6, V, (N, L), generator=g)
    cap[torch.arange(L)[None, :] >= lengths[:, None]] = 0
    cap[torch.arange(N), lengths - 1] = 3
    cap, lengths, index = cap.to(dev), lengths.to(dev), (torch.arange(N) % T).to(dev)
    images = synth_images(N if what == "generate" else T, seed=0).to(dev)
    images = images if fp32 else images.bfloat16()
    if what == "fp32-logits":
        class LogitsRoute(dict):               # explain_captions asks `"cls_w_x" in plan`; forward reads plan.get("cls_w_x"): every
            def __contains__(self, key):       # kernel as on the fused route (the split classifier too), but the logits are written
                return key != "cls_w_x" and dict.__contains__(self, key)
        get_plan = model.decoder._get_plan
        model.decoder._get_plan = lambda: LogitsRoute(get_plan())
    if what in ("fp32-fused", "fp32-logits"):
        call = lambda: X.explain_captions(model, images, index, cap, lengths)                                  # noqa: E731
    elif what == "fp32-score" or what == "score":
        call = lambda: X.score_captions(model, images, index, cap, lengths)                                    # noqa: E731
    elif what == "bf16":
        call = lambda: X.explain_captions(model, images, index, cap, lengths)                                  # noqa: E731
    elif what == "bf16-attn":
        call = lambda: X.explain_captions(model, images, index, cap, lengths, return_attention=True)           # noqa: E731
    elif what == "generate":
        call = lambda: model.generate_batch(images, max_len=32, beam_size=5, top_k=50, temperature=1.0, seed=7)  # noqa: E731
    else:
        raise SystemExit(f"unknown measurement {what!r}")
    ts = []
    with torch.no_grad(), hip.option_scope(**(dict(f32_split=1) if fp32 else {})):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    print(f"TIME {what} {statistics.median(ts):.4f} {torch.cuda.max_memory_allocated()}", flush=True)


def child(args, limit=240):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, text=True)
    print(p.stdout, end="", flush=True)
    return p.returncode, p.stdout


def everything(parent, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ms = {k: [] for k in PLAN}
    peak = {}
    for _ in range(ROUNDS):
        for what, where in PLAN:                                         # fresh processes in turn
            rc, out = child(["one", what, ROOT if where == "this" else parent])
            if rc != 0:
                print(f"step ended with status {rc}: nothing further is started", flush=True)
                return rc
            f = [l for l in out.splitlines() if l.startswith("TIME ")][-1].split()
            ms[(what, where)].append(float(f[2]))
            peak[(what, where)] = int(f[3])
    lines = [f"explain_captions: CaptioningTransformer, V={V}, hidden 512, {N} captions x {L} positions over {T} templates (generate: {N} images, "
             f"beam 5, max_len 32); {ROUNDS} rounds, a fresh process per measurement and round in turn, each the median of {REPEATS} calls "
             f"after 3 warm-ups; ms per call; peak = torch.cuda.max_memory_allocated over the timed calls", ""]
    for k in PLAN:
        a = ms[k]
        lines.append(f"  {k[0]:12s} {k[1]:7s} median {statistics.median(a):9.3f}  rounds {min(a):9.3f} .. {max(a):9.3f}  spread {max(a) - min(a):7.3f}"
                     f"  peak {peak[k] / 2 ** 20:9.1f} MiB")
    med = lambda k: statistics.median(ms[k])                             # noqa: E731
    lines += ["", f"  fp32 fused - logits route: {med(('fp32-fused', 'this')) - med(('fp32-logits', 'this')):+.3f} ms",
              f"  fp32 fused - parent's fp32 score_captions: {med(('fp32-fused', 'this')) - med(('fp32-score', 'parent')):+.3f} ms",
              f"  bf16 return_attention - without: {med(('bf16-attn', 'this')) - med(('bf16', 'this')):+.3f} ms",
              f"  bf16 explain_captions - score_captions: {med(('bf16', 'this')) - med(('score', 'this')):+.3f} ms"]
    for what in ("score", "generate"):
        lines.append(f"  {what}: this tree - parent {med((what, 'this')) - med((what, 'parent')):+.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out_dir, "timing.txt"), "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "all":
        sys.exit(everything(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else "."))
    one(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ROOT)
