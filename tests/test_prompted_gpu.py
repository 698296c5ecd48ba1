"""Prompted batches on the GPU: ``generate_batch(..., caption=C, caption_lengths=L)`` gives every image a caption prompt of its own
length.  The contract (extended): row ``i`` equals the reference's result for image ``i`` under prompt ``i`` --
pinned against the reference's recorded captions and the CPU oracle for greedy fp32, and against the dense single-image call
``generate_batch(images[i:i+1], caption=C[i:i+1, :L[i]], img0=i)`` for sampled beams in every number format and execution mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import KINDS, golden, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS = {}


def build(kind, v=None, dtype="fp32"):
    """(model on the GPU, state dict, hp); one instance per (kind, vocabulary, storage type) for the module."""
    key = (kind, v, dtype in ("bf16", "fp16") and dtype)
    if key not in _MODELS:
        import deephumor_amd.models as M
        sd, hp = synthetic_sd(kind, v)
        model = getattr(M, kind)(**hp).eval()
        model.load_state_dict(sd)
        model = model.cuda()
        model = model.bfloat16() if dtype == "bf16" else model.half() if dtype == "fp16" else model
        _MODELS[key] = (model, sd, hp)
    return _MODELS[key]


def scope(dtype):
    from deephumor_amd import hip
    return hip.option_scope(f32_split=1) if dtype == "f32x" else hip.option_scope()


def inputs(n, p, v, seed, lengths=None):
    """images [n], labels [n, 3], prompts [n, p] from ids 6..v-1, lengths [n] (mixed, with 0 and p among them)."""
    g = np.random.Generator(np.random.Philox(key=[seed, 19]))
    cap = torch.from_numpy(g.integers(6, v, size=(n, p)).astype(np.int64))
    labels = torch.from_numpy(g.integers(6, v, size=(n, 3)).astype(np.int64))
    if lengths is None:
        lengths = g.integers(0, p + 1, size=n)
        lengths[0], lengths[1], lengths[n - 1] = 0, p, 0
    return synth_images(n, seed=seed).cuda(), labels.cuda(), cap.cuda(), torch.as_tensor(np.asarray(lengths), dtype=torch.int64)


def margs(kind, images, labels, sl=slice(None)):
    return (images[sl], labels[sl]) if "WithLabels" in kind else (images[sl],)


def singles(model, kind, images, labels, cap, lengths, **kw):
    """The contract's right-hand side: one dense single-image call per row, ``img0=i``."""
    rows, lens = [], []
    for i, n in enumerate(lengths.tolist()):
        t, l = model.generate_batch(*margs(kind, images, labels, slice(i, i + 1)), caption=cap[i:i + 1, :n] if n else None, img0=i, **kw)
        rows.append(t[0].tolist())
        lens.append(int(l[0]))
    return rows, lens


def assert_rows(got, want, what=""):
    toks, lens = got
    rows, wl = want
    for i in range(len(rows)):
        assert toks[i].tolist() == rows[i] and int(lens[i]) == wl[i], (what, i, toks[i].tolist(), rows[i], int(lens[i]), wl[i])


# ---- 1. against the reference, greedy, fp32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_greedy_rows_equal_the_reference(kind):
    """8 images, prompt lengths [0, 1, 3, 3, 7, 12, 5, 0], max_len 32, beam 1 / top-1: every row equals the caption the REAL reference
    returned for that image under that prompt (``g19_prompted.npz``, recorded by ``tools/make_prompted_golden.py``) and what the CPU
    oracle returns here.  Prompt seed 0 -- the first one tried -- has a smallest top-2 logit margin of 0.001243 over all kinds, rows
    and steps, above the project's fp32 logit bar of 1e-3, so no arg-max flip is excusable."""
    from oracle import ref_path as R
    g = golden("g19_prompted.npz")
    assert float(g["min_margin"][0]) >= 1e-3
    model, sd, hp = build(kind)
    images = synth_images(8, seed=0)
    prompts, labels, lengths = torch.from_numpy(g["prompts"]), torch.from_numpy(g["labels"]), torch.from_numpy(g["lengths"])
    assert lengths.tolist() == [0, 1, 3, 3, 7, 12, 5, 0]
    with torch.no_grad():
        toks, lens = model.generate_batch(*margs(kind, images.cuda(), labels.cuda()), caption=prompts.cuda(), caption_lengths=lengths,
                                          max_len=32, beam_size=1, top_k=1)
    toks, lens = toks.cpu(), lens.cpu()
    for i, n in enumerate(lengths.tolist()):
        got = toks[i, :int(lens[i])].tolist()
        assert got == g[f"{kind}_ids_{i}"].tolist(), (kind, i, "recorded reference")
        want = R.model_generate(kind, sd, hp, images[i:i + 1], label=labels[i:i + 1] if "WithLabels" in kind else None,
                                caption=prompts[i:i + 1, :n] if n else None, max_len=32, beam_size=1, top_k=1)
        assert got == want.reshape(-1).tolist(), (kind, i, "oracle")
        assert got[:n] == prompts[i, :n].tolist() and int(toks[i, int(lens[i]):].abs().sum()) == 0


# ---- 2. batch == singles, sampled -------------------------------------------------------------------------------------------------
SAMPLED_KINDS = ("CaptioningLSTM", "CaptioningTransformer", "CaptioningTransformerBase")


@pytest.mark.parametrize("dtype", ("fp32", "f32x", "bf16", "fp16"))
@pytest.mark.parametrize("kind", SAMPLED_KINDS)
def test_sampled_batch_equals_single_image_calls(kind, dtype):
    """Beam 5, top-50, fixed seed, 16 images with mixed prompt lengths (0 and P among them), V = 1000 (the plain row sampler)."""
    model, _, _ = build(kind, dtype=dtype)
    images, labels, cap, lengths = inputs(16, 9, 1000, seed=5)
    kw = dict(max_len=20, beam_size=5, top_k=50, temperature=1.0, seed=1234)
    with torch.no_grad(), scope(dtype):
        got = model.generate_batch(*margs(kind, images, labels), caption=cap, caption_lengths=lengths, **kw)
        want = singles(model, kind, images, labels, cap, lengths, **kw)
    assert_rows(got, want, (kind, dtype))
    assert len({tuple(r) for r in want[0]}) > 8                                # sampled captions, not one degenerate row


def test_sampled_batch_at_the_word_vocabulary_takes_the_group_sampler():
    """V = 36,541, 64 images, bf16: ``top_k <= n_groups`` so the row draw is ``dh_beam_row_sample_groups_prompted``."""
    from deephumor_amd import hip
    kind = "CaptioningTransformer"
    model, _, _ = build(kind, v=36541, dtype="bf16")
    assert 50 <= hip.n_groups(36541)
    images, labels, cap, lengths = inputs(64, 8, 36541, seed=6)
    kw = dict(max_len=16, beam_size=5, top_k=50, temperature=1.0, seed=99)
    with torch.no_grad():
        got = model.generate_batch(images, caption=cap, caption_lengths=lengths.cuda(), **kw)
        want = singles(model, kind, images, labels, cap, lengths, **kw)
    assert_rows(got, want, "V=36541")


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_sampled_batch_exact_sampler(kind):
    model, _, _ = build(kind)
    images, labels, cap, lengths = inputs(6, 5, 1000, seed=7)
    kw = dict(max_len=12, beam_size=5, top_k=50, seed=3, exact=True)
    with torch.no_grad():
        got = model.generate_batch(images, caption=cap, caption_lengths=lengths, **kw)
        assert_rows(got, singles(model, kind, images, labels, cap, lengths, **kw), kind)
        fast = model.generate_batch(images, caption=cap, caption_lengths=lengths, **dict(kw, exact=False))
    assert fast[0].tolist() == got[0].tolist()                                  # same seed, nothing overflows: same captions


# ---- 3. / 4. padding is ignored; dense == prompted for equal lengths ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTMWithLabels", "CaptioningTransformerWithLabels"))
def test_padding_is_ignored_and_equal_lengths_equal_the_dense_call(kind):
    model, _, hp = build(kind)
    images, labels, cap, lengths = inputs(6, 7, 1000, seed=8)
    kw = dict(max_len=14, beam_size=4, top_k=30, seed=11)
    used = torch.arange(7)[None, :] < lengths[:, None]
    with torch.no_grad():
        base = model.generate_batch(images, labels, caption=cap, caption_lengths=lengths, **kw)
        for fill in (torch.randint(6, 1000, (6, 7)), torch.full((6, 7), hp.get("pad_index", 0)), torch.full((6, 7), 3)):
            other = torch.where(used, cap.cpu(), fill).cuda()
            t, l = model.generate_batch(images, labels, caption=other, caption_lengths=lengths.cuda().int(), **kw)
            assert t.tolist() == base[0].tolist() and l.tolist() == base[1].tolist()
        dense = model.generate_batch(images, labels, caption=cap[:, :3], **kw)
        same = model.generate_batch(images, labels, caption=cap, caption_lengths=torch.full((6,), 3), **kw)
        assert same[0].tolist() == dense[0].tolist() and same[1].tolist() == dense[1].tolist()
        none = model.generate_batch(images, labels, **kw)
        zero = model.generate_batch(images, labels, caption=cap, caption_lengths=torch.zeros(6, dtype=torch.int64), **kw)
        assert zero[0].tolist() == none[0].tolist() and zero[1].tolist() == none[1].tolist()


# ---- 5. execution modes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_streams_early_stop_and_graph_replay(kind, dtype):
    model, _, _ = build(kind, dtype=dtype)
    images, labels, cap, lengths = inputs(8, 6, 1000, seed=9)
    kw = dict(max_len=14, beam_size=3, top_k=20, temperature=1.2)
    with torch.no_grad():
        want = model.generate_batch(images, caption=cap, caption_lengths=lengths, seed=21, **kw)
        assert_rows(want, singles(model, kind, images, labels, cap, lengths, seed=21, **kw), (kind, dtype))
        for extra in (dict(streams=2), dict(streams=3), dict(early_stop_every=4), dict(early_stop_every=1, streams=2)):
            t, l = model.generate_batch(images, caption=cap, caption_lengths=lengths, seed=21, **kw, **extra)
            assert t.tolist() == want[0].tolist() and l.tolist() == want[1].tolist(), extra
        # one captured graph, replayed with other lengths (and another seed) of the same shape: what eager returns
        other = torch.tensor([6, 0, 2, 2, 5, 1, 0, 3])
        for seed, lens in ((21, lengths), (22, other), (21, lengths)):
            eager = model.generate_batch(images, caption=cap, caption_lengths=lens, seed=seed, **kw)
            t, l = model.generate_batch_graphed(images, caption=cap, caption_lengths=lens, seed=seed, **kw)
            assert t.tolist() == eager[0].tolist() and l.tolist() == eager[1].tolist(), (seed, lens.tolist())
        assert sum(1 for k in model._graphs if k[-1]) == 1
        with pytest.raises(ValueError):
            model.generate_batch_graphed(images, caption=cap, caption_lengths=torch.full((8,), 7), seed=1, **kw)
    model._graphs.clear()


SHARD_CHILD = r"""
import sys, os, json, socket, datetime
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch, torch.distributed as dist
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
with socket.socket() as _s:
    _s.bind(("127.0.0.1", 0))
    _port = _s.getsockname()[1]
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT") or str(_port))
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=300))
import deephumor_amd.models as M
from deephumor_amd import hip
from deephumor_amd.dist import generate_micro_sharded, shard_range
from deephumor_amd.synth import synth_images, synth_state_dict
hip.set_option("dist_always", 1)
N, SH, P, V = 7, 2, 6, 1000
res = {"backend": dist.get_backend()}
g = np.random.Generator(np.random.Philox(key=[3, 19]))
cap = torch.from_numpy(g.integers(6, V, size=(N, P)).astype(np.int64)).to(dev)
lengths = torch.tensor([0, 6, 2, 5, 0, 3, 1])
images = synth_images(N, seed=4).to(dev)
kw = dict(max_len=14, beam_size=4, top_k=40, seed=17)
for name, cls in (("lstm", M.CaptioningLSTM), ("transformer", M.CaptioningTransformer)):
    model = cls(V).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234))
    model = model.to(dev).bfloat16()
    spans = []
    def fn(lo, hi):
        spans.append((lo, hi))
        return model.generate_batch(images[lo:hi], caption=cap[lo:hi], caption_lengths=lengths[lo:hi], img0=lo, **kw)
    with torch.no_grad():
        toks, lens = generate_micro_sharded(fn, N, SH)
        one, one_l = model.generate_batch(images, caption=cap, caption_lengths=lengths, **kw)
    res[name] = [b - a for a, b in spans] + [bool(torch.equal(toks, one) and torch.equal(lens, one_l))]
print("RESULT " + json.dumps(res))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_uneven_shards_equal_one_batch():
    """``dist.generate_micro_sharded`` on the one-rank group: shards of 4 and 3 images, each with its slice of ``caption`` and
    ``caption_lengths`` and ``img0`` = its first image, give the rows of the single batch of 7."""
    p = subprocess.run([sys.executable, "-c", SHARD_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res == {"backend": "nccl", "lstm": [4, 3, True], "transformer": [4, 3, True]}


# ---- 6. EOS inside the mixed range ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_eos_while_a_neighbour_is_still_forced(kind):
    """The classifier bias forces <eos> (as ``test_forced_eos_shapes`` does): images 0 and 2 end at positions 1-2 and 3-4 while
    images 1 and 3 are still being teacher-forced up to position 6.  Lengths and the LSTM's ``[..., 3, 0]`` / the Transformer's
    EOS-excluded output are the reference's (CPU oracle on the same weights) and the dense single-image call's."""
    import deephumor_amd.models as M
    from oracle import ref_path as R
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()
    model.load_state_dict(sd)
    model = model.cuda()
    sd = dict(sd)
    sd["decoder.classifier.bias"] = sd["decoder.classifier.bias"].clone()
    sd["decoder.classifier.bias"][3] += 100.0
    with torch.no_grad():
        model.decoder.classifier.bias[3] += 100.0
    images, labels, cap, _ = inputs(4, 6, 1000, seed=10)
    lengths = torch.tensor([0, 6, 2, 5])
    for kw in (dict(max_len=12, beam_size=1, top_k=1), dict(max_len=12, beam_size=3, top_k=10, seed=4)):
        with torch.no_grad():
            toks, lens = model.generate_batch(images, caption=cap, caption_lengths=lengths, **kw)
            assert_rows((toks, lens), singles(model, kind, images, labels, cap, lengths, **kw), kind)
        if kw["beam_size"] == 1:
            for i, n in enumerate(lengths.tolist()):
                want = R.model_generate(kind, sd, hp, images[i:i + 1].cpu(), caption=cap[i:i + 1, :n].cpu() if n else None, **kw)
                got = toks[i, :int(lens[i])].tolist()
                assert got == want.reshape(-1).tolist(), (kind, i)
                assert got == cap[i, :n].tolist() + ([3, 0] if "LSTM" in kind else [3])


# ---- 7. kernel level --------------------------------------------------------------------------------------------------------------
def _state(n_img, b, t_ld, s_ld, dev, gen):
    r = n_img * b
    base = (torch.arange(r, dtype=torch.int32) // b) * b
    st = dict(tokens=torch.randint(6, 900, (r, t_ld), generator=gen, dtype=torch.int32),
              vals=-torch.rand(r, generator=gen), ended=torch.zeros(r, dtype=torch.uint8),
              src=base[:, None] + torch.randint(0, b, (r, s_ld), generator=gen, dtype=torch.int32),
              parent=base.clone(), hparent=base.clone(), done=torch.zeros(n_img, dtype=torch.uint8),
              end_step=torch.zeros(n_img, dtype=torch.int32))
    return {k: v.to(dev) for k, v in st.items()}


@pytest.mark.parametrize("sampler,v", (("plain", 1000), ("exact", 1000), ("groups", 4096), ("general", 70000)))
@pytest.mark.parametrize("lstm", (False, True))
def test_prompted_kernels_one_launch_three_phases(sampler, v, lstm):
    """One launch holding a forced image (NaN in all its logits rows), a first image and a normal one: the forced image's tokens,
    scores and flags are untouched, its rows point at its base row, and the error word stays 0; the other two equal the existing
    entry points run on those images alone (same global image index, same step)."""
    from deephumor_amd import hip
    dev, b, top_k, t_ld, step = "cuda", 3, 50, 12, 2
    gen = torch.Generator().manual_seed(77 + v)
    logits = (torch.randn(3 * b, v, generator=gen) * 3).to(dev)
    logits[:b] = float("nan")
    logits[b + 1:2 * b] = float("nan")                      # the first image's other rows are not read either
    gmax = None
    if sampler == "groups":
        ng = hip.n_groups(v)
        pad = torch.full((3 * b, ng * hip.GROUP_COLS), float("-inf"), device=dev)
        pad[:, :v] = logits
        gmax = pad.view(3 * b, ng, hip.GROUP_COLS).max(-1).values.contiguous()
    first_pos = torch.tensor([5, 2, 0], dtype=torch.int32, device=dev)
    st = _state(3, b, t_ld, t_ld + 1, dev, gen)
    if lstm:
        st["src"] = None
    before = {k: (None if x is None else x.clone()) for k, x in st.items()}
    pi = torch.full((3 * b, b), -7, dtype=torch.int32, device=dev)
    pv = torch.full((3 * b, b), -7.0, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    seed, t = 4242, (0 if lstm else step)
    hip.beam_row_sample_prompted(logits, v, 3 * b, b, top_k, 1.0, 1, None, seed, 0, step, first_pos, pi, pv, err,
                                 exact=sampler == "exact", group_max=gmax)
    hip.beam_select_prompted(pi, pv, st["tokens"], st["vals"], st["ended"], st["src"], st["parent"], st["hparent"], st["done"],
                             st["end_step"], 3, b, first_pos, lstm, step, t, step, 1.0, 3, None, seed, 0)
    assert int(err.item()) == 0
    # forced image: nothing drawn, nothing moved
    assert (pi[:b] == -7).all() and (pv[:b] == -7).all() and (pi[b + 1:2 * b] == -7).all()
    for k in ("tokens", "vals", "ended"):
        assert torch.equal(st[k][:b], before[k][:b]), k
    assert int(st["done"][0]) == 0 and int(st["end_step"][0]) == 0
    assert (st["parent"][:b] == 0).all() and (st["hparent"][:b] == 0).all()
    if not lstm:
        assert (st["src"][:b, t] == 0).all() and torch.equal(st["src"][:b, :t], before["src"][:b, :t])
        assert torch.equal(st["src"][:b, t + 1:], before["src"][:b, t + 1:])
    # the other two images alone through the existing entry points
    for img, first in ((1, True), (2, False)):
        lo = img * b
        rows = 1 if first else b
        lg = logits[lo:lo + rows].contiguous()
        api = torch.empty((rows, b), dtype=torch.int32, device=dev)
        apv = torch.empty((rows, b), device=dev)
        aerr = torch.zeros(1, dtype=torch.int32, device=dev)
        if sampler == "groups":
            hip.beam_row_sample_groups(lg, v, gmax[lo:lo + rows].contiguous(), rows, rows, b, top_k, 1.0, 1, None, seed, img, step, api, apv, aerr)
        else:
            hip.beam_row_sample(lg, v, rows, rows, b, top_k, 1.0, 1, None, seed, img, step, api, apv, aerr, exact=sampler == "exact")
        assert int(aerr.item()) == 0
        assert torch.equal(pi[lo:lo + rows], api) and torch.equal(pv[lo:lo + rows], apv), (img, "picks")
        a = {k: (None if x is None else x[(slice(img, img + 1) if k in ("done", "end_step") else slice(lo, lo + b))].clone())
             for k, x in before.items()}
        for k in ("src", "parent", "hparent"):
            if a[k] is not None:
                a[k] -= lo
        hip.beam_select(api, apv, a["tokens"], a["vals"], a["ended"], a["src"], a["parent"], a["hparent"], a["done"], a["end_step"],
                        1, b, first, lstm, step, t, step, 1.0, 3, None, seed, img)
        for k in ("tokens", "vals", "ended"):
            assert torch.equal(st[k][lo:lo + b], a[k]), (img, k)
        for k in ("parent", "hparent") + (() if lstm else ("src",)):
            assert torch.equal(st[k][lo:lo + b], a[k] + lo), (img, k)
        assert torch.equal(st["done"][img:img + 1], a["done"]) and torch.equal(st["end_step"][img:img + 1], a["end_step"])
        assert (st["tokens"][lo:lo + b, step] != before["tokens"][lo:lo + b, step]).any()         # (something was written)
