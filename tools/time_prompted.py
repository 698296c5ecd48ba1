"""Times a prompted batch on the GPU against what a caller had to do without ``caption_lengths``: the BASELINE C3 model
(CaptioningTransformer, V = 36,541, bf16), 256 images, beam 5, ``max_len=32``, prompt lengths uniform in 0...8.

    python tools/time_prompted.py [report.txt]

Three variants, alternated inside every repeat after a warm-up of every shape, each a host clock around calls that end in a device
synchronise: (a) one prompted call, (b) one dense call with p = 8 for all images (other captions: the cost floor of a dense batch),
(c) the same images cut into one dense call per prompt length that occurs (nine here) -- what a caller does today; its Philox keys
are per call, so (c) is comparable with (a) in shapes and cost, not caption by caption.  Four rows of (a) are checked against their
dense single-image calls; the full contract is in tests/test_prompted_gpu.py.  Information, not a gate."""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import deephumor_amd.models as M                      # noqa: E402
from deephumor_amd.synth import synth_images, synth_state_dict   # noqa: E402

N, P, V, REPEATS = 256, 8, 36541, 10


def main():
    dev = torch.device("cuda", 0)
    model = M.CaptioningTransformer(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).bfloat16()
    g = np.random.Generator(np.random.Philox(key=[2, 19]))
    cap = torch.from_numpy(g.integers(6, V, size=(N, P)).astype(np.int64)).to(dev)
    lengths = torch.from_numpy(g.integers(0, P + 1, size=N).astype(np.int64))
    images = synth_images(N, seed=0).to(dev)
    kw = dict(max_len=32, beam_size=5, top_k=50, seed=7)
    groups = [(n, torch.nonzero(lengths == n).flatten().to(dev)) for n in range(P + 1) if bool((lengths == n).any())]

    def prompted(enc=None):
        return model.generate_batch(images, caption=cap, caption_lengths=lengths, **kw) if enc is None else \
            model.decode(enc, caption=cap, caption_lengths=lengths, **kw)

    def dense(enc=None):
        return model.generate_batch(images, caption=cap, **kw) if enc is None else model.decode(enc, caption=cap, **kw)

    def cut(enc=None):
        toks = torch.zeros((N, kw["max_len"]), dtype=torch.int64, device=dev)
        lens = torch.zeros((N,), dtype=torch.int64, device=dev)
        for n, idx in groups:
            # (a caller's own cut: images of one prompt length gathered into one dense call; the Philox key is per call here, so
            #  only shapes and cost are comparable, not captions)
            c = cap[idx][:, :n] if n else None
            t, l = model.generate_batch(images[idx], caption=c, **kw) if enc is None else \
                model.decode(tuple(e[idx] for e in enc), caption=c, **kw)
            toks[idx], lens[idx] = t, l
        return toks, lens

    times = {}
    with torch.no_grad():
        enc = model.encode(images)
        variants = [("prompted, one call", prompted), ("dense p=8, one call", dense), (f"cut into {len(groups)} dense calls by length", cut)]
        for whole in (True, False):
            for _ in range(3):
                for name, fn in variants:
                    fn(None if whole else enc)
            torch.cuda.synchronize()
            for _ in range(REPEATS):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(None if whole else enc)
                    torch.cuda.synchronize()
                    times.setdefault((whole, name), []).append((time.perf_counter() - t0) * 1e3)
        # the prompted rows are the per-image dense rows (spot check on 4 images; the test suite holds the full contract)
        toks, lens = prompted()
        for i in (0, 1, 100, 255):
            n = int(lengths[i])
            t, l = model.generate_batch(images[i:i + 1], caption=cap[i:i + 1, :n] if n else None, img0=i, **kw)
            assert torch.equal(t[0], toks[i]) and int(l[0]) == int(lens[i]), i
    lines = [f"prompted generate_batch: CaptioningTransformer (C3), V={V}, bf16, {N} images, beam 5, max_len 32, top_k 50",
             f"prompt lengths uniform in 0..{P}: histogram {[int((lengths == n).sum()) for n in range(P + 1)]}",
             f"device: {torch.cuda.get_device_name(0)}; host clock around device-synchronised calls; 3 warm-up rounds of every shape, "
             f"{REPEATS} repeats, variants alternated inside each repeat; ms per {N} images",
             ""]
    for whole in (True, False):
        lines.append("encoder + decode (generate_batch):" if whole else "decode only (model.decode on encoded features):")
        for (w, name), ts in times.items():
            if w == whole:
                lines.append(f"  {name:42s} median {statistics.median(ts):8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
