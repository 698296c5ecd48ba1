"""Nucleus (top-p) filtering on a real MI355X: ``dh_beam_row_sample_nucleus`` on every kernel route against the torch-CPU
restatement (``tests/nucleus_ref.py``) with supplied noise, its prompted phases, its overflow rule, ``generate_batch(..., top_p=p)``
against golden G20 recorded from the reference, and the keyword through every layer that carries it."""
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import KINDS, captions_and_lengths, golden, synthetic_sd, synth_images  # noqa: E402
from nucleus_ref import nucleus_keep, nucleus_row_sample  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20_KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
ROWS, RPI = 6, 3


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


def close(a, b, atol):
    assert float((a.detach().cpu().float() - b.detach().cpu().float()).abs().max()) <= atol


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
def make_rows(v, top_k, beam, temp, seed, scale=2.5):
    """Six rows: random logits; row 0 with <unk> as its arg-max; row 1 with one dominant token (p > 0.999: the ``beam`` floor decides);
    row 2 with one token of p ~ 0.45, FIVE bit-equal logits of p ~ 0.1 each and ~ 0.05 for the rest of the top-k -- at
    ``top_p = 0.8`` the boundary falls between the fourth and the fifth of the equal ones, which only their index tells apart."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(ROWS, v, generator=g) * scale
    if top_k > 6:
        logits[0, 1] = 50.0
        logits[1, 7] = float(logits[1].max()) + 12.0 * temp
        rest = torch.topk(logits[2], top_k - 6).values
        m = temp * float(torch.log(torch.exp(rest.double() / temp).sum() / 0.5))
        logits[2, 5] = m + temp * float(torch.log(torch.tensor(4.5)))
        logits[2, 10:15] = m
    noise = torch.empty(ROWS, v).exponential_(1, generator=g)
    return logits, noise


_inputs = {}


def inputs(v, top_k, beam, temp, top_p, scale=2.5):
    """The first seed (of 64 at most) whose rows keep every nucleus boundary at least 1e-4 away from ``top_p`` in the restatement:
    a condition on the inputs, met on the CPU before the GPU is asked anything.  Reference computed once per case."""
    key = (v, top_k, beam, temp, top_p, scale)
    if key not in _inputs:
        for seed in range(64):
            logits, noise = make_rows(v, top_k, beam, temp, seed, scale)
            picks, vals, margin, keep = nucleus_row_sample(logits, noise, temp, beam, top_k, top_p)
            if margin >= 1e-4:
                break
        _inputs[key] = (logits, noise, picks, vals, margin, keep)
    return _inputs[key]


def group_max(h, x):
    rows, v = x.shape
    ng = h.n_groups(v)
    pad = torch.full((rows, ng * 64), float("-inf"))
    pad[:, :v] = x
    return pad.view(rows, ng, 64).max(-1).values.cuda()


def run_kernel(h, logits, noise, beam, top_k, top_p, temp, route, rpi=RPI, first_pos=None, step=0, seed=0, img0=0, fill=None):
    rows, v = logits.shape
    pi = torch.full((rows, beam), -7 if fill is None else fill, dtype=torch.int32, device="cuda")
    pv = torch.full((rows, beam), -7.0, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    x = logits.cuda()
    h.beam_row_sample_nucleus(x, v, rows, rpi, beam, top_k, top_p, temp, 1, None if noise is None else noise.cuda(), seed, img0, step,
                              pi, pv, err, exact=route == "exact", group_max=group_max(h, logits) if route == "groups" else None,
                              first_pos=first_pos)
    return pi.cpu().long(), pv.cpu(), int(err.item())


# (v, top_k, beam, temperature, spread of the random logits, routes)
CASES = [(71, 50, 7, 1.1, 2.5, ("plain",)),                       # the 512-thread single-pass kernel, n < 64
         (1000, 20, 3, 1.3, 2.5, ("plain",)),
         (36541, 50, 5, 1.0, 2.5, ("plain", "exact", "groups")),  # 1,024 threads (one sorted position each) / 256 threads / groups
         # n > NT: several elements per thread in the sort and the scan.  700 survivors of N(0, 2.5) logits would pass top_p = 0.97 at
         # p ~ 1e-4 per token, where no boundary can lie 1e-4 from anything: the wider spread puts the mass on fewer tokens
         (4000, 700, 5, 1.0, 4.5, ("exact",)),
         # nearly uniform p ~ 0.005: the nucleus is 60 .. 190 tokens long, so the prefix crosses DPP rows, waves (1,024 threads: one
         # position per thread) and the threads' runs (256 threads: four positions each)
         (5000, 200, 3, 1.0, 0.3, ("plain", "exact")),
         (500, 1, 1, 1.0, 2.5, ("plain", "exact"))]               # beam = top_k = 1


@pytest.mark.parametrize("top_p", [0.3, 0.8, 0.97])
@pytest.mark.parametrize("v,top_k,beam,temp,scale,routes", CASES, ids=lambda c: str(c) if not isinstance(c, tuple) else "-".join(c))
def test_kernel_matches_the_restatement(hip, v, top_k, beam, temp, scale, routes, top_p):
    """Picks equal, values within 2e-6 (as test_beam_row_sample), on every route the case names."""
    logits, noise, picks, vals, margin, keep = inputs(v, top_k, beam, temp, top_p, scale)
    from oracle.ref_path import BeamBook
    survivors = torch.isfinite(BeamBook(temp, beam, top_k).keep_top_k(logits.clone())).sum(1).tolist()
    print("margin", margin, "kept per row", keep.sum(1).tolist(), "of survivors", survivors)
    assert margin >= 1e-4
    if top_k > 6:
        assert not keep[0, 1] and int(logits[0].argmax()) == 1                   # <unk> as the arg-max
        assert int(keep[1].sum()) == beam and bool(keep[1, 7])                  # one dominant token: the floor
        if top_p == 0.8 and beam <= 5 and scale > 1:
            assert keep[2, 10:15].tolist() == [True, True, True, True, False]   # five bit-equal logits straddle the boundary
    for route in routes:
        pi, pv, err = run_kernel(hip, logits, noise, beam, top_k, top_p, temp, route)
        print(route, "err", err, "max |value diff|", float((pv - vals).abs().max()))
        assert err == 0, route
        assert pi.tolist() == picks.tolist(), route
        close(pv, vals, atol=2e-6)
    # Philox: every pick inside the nucleus, distinct, deterministic, seed-dependent
    a = run_kernel(hip, logits, None, beam, top_k, top_p, temp, routes[0], seed=11, img0=5, step=2)[0]
    b = run_kernel(hip, logits, None, beam, top_k, top_p, temp, routes[-1], seed=11, img0=5, step=2)[0]
    assert a.tolist() == b.tolist()
    assert bool(keep.gather(1, a).all()) and all(len(set(r)) == beam for r in a.tolist())


def test_kept_noise_does_not_move(hip):
    """The noise is indexed by token id: with ``top_p`` so close to 1 that nothing is cut, the Philox picks are those of
    ``dh_beam_row_sample`` with the same key."""
    logits, _ = make_rows(1000, 20, 3, 1.3, 0)
    from oracle.ref_path import BeamBook
    filt = BeamBook(1.3, 3, 20).keep_top_k(logits.clone())
    keep, _ = nucleus_keep(filt, 1.3, 0.9999999, 3)
    rows = [r for r in range(ROWS) if torch.equal(keep[r], torch.isfinite(filt[r]))]
    assert len(rows) >= 3
    a = run_kernel(hip, logits, None, 3, 20, 0.9999999, 1.3, "plain", seed=9, img0=4, step=6)[0]
    pi = torch.empty(ROWS, 3, dtype=torch.int32, device="cuda")
    pv = torch.empty(ROWS, 3, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.beam_row_sample(logits.cuda(), 1000, ROWS, RPI, 3, 20, 1.3, 1, None, 9, 4, 6, pi, pv, err)
    assert a[rows].tolist() == pi.cpu().long()[rows].tolist()


# ---- 2. prompted route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["plain", "exact", "groups"])
def test_prompted_phases(hip, route):
    """``first_pos = [0, 2]`` at steps 0, 2 and 3: idle rows untouched, an image's first row and its normal rows equal the dense
    calls on that image alone (same global image index, same step)."""
    v, b, top_k, temp, top_p = 36541 if route == "groups" else 1000, 3, 20, 1.0, 0.8
    logits = torch.randn(2 * b, v, generator=torch.Generator().manual_seed(3)) * 2.5
    fp = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    for step in (0, 2, 3):
        pi, pv, err = run_kernel(hip, logits, None, b, top_k, top_p, temp, route, rpi=b, first_pos=fp, step=step, seed=21)
        assert err == 0
        for img, f in enumerate((0, 2)):
            lo = img * b
            if step < f:
                assert bool((pi[lo:lo + b] == -7).all()) and bool((pv[lo:lo + b] == -7.0).all())
                continue
            n = 1 if step == f else b                 # first: the base row alone draws, as the dense first step (row index 0)
            di, dv, derr = run_kernel(hip, logits[lo:lo + n], None, b, top_k, top_p, temp, route, rpi=n, step=step, seed=21, img0=img)
            assert derr == 0 and pi[lo:lo + n].tolist() == di.tolist() and torch.equal(pv[lo:lo + n], dv), (step, img)
            assert bool((pi[lo + n:lo + b] == -7).all())


# ---- 3. overflow ------------------------------------------------------------------------------------------------------------------
def test_flat_row_flags_overflow_on_every_route(hip):
    x = torch.full((2, 5000), 0.25)
    for route in ("plain", "exact", "groups"):
        pi, pv, err = run_kernel(hip, x, None, 3, 50, 0.9, 1.0, route, rpi=1)
        assert err & hip.ERR_OVERFLOW, route
        assert bool((pi >= 0).all()) and bool((pi < 5000).all())


def build(kind, v=None, **hp_over):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind, v)
    hp = dict(hp, **hp_over)
    model = getattr(M, kind)(**hp).eval()
    model.load_state_dict(sd)
    return model.cuda(), sd, hp


@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0)


def model_args(kind, images, lo, hi):
    _, _, labels = captions_and_lengths()
    return (images[lo:hi].cuda(), labels[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_flat_logits_raise_beam_overflow_naming_top_p(kind, images):
    from deephumor_amd.models.beam import BeamOverflow
    model, _, _ = build(kind, 5000)
    with torch.no_grad():
        model.decoder.classifier.weight.zero_()
        model.decoder.classifier.bias.zero_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(BeamOverflow, match="top_p"), torch.no_grad():
            model.generate_batch(*model_args(kind, images, 0, 2), max_len=5, beam_size=3, top_k=20, seed=5, top_p=0.9)
        with torch.no_grad():                                      # without the nucleus the exact retry still answers
            model.generate_batch(*model_args(kind, images, 0, 2), max_len=5, beam_size=3, top_k=20, seed=5)


# ---- 4. model level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_caption_matches_the_reference(kind, images):
    """fp32, ``rng="torch"``: the caption is golden G20's, token for token (the fixture keeps every nucleus boundary >= 1e-3 away
    from ``top_p``, the fp32 logit gate)."""
    g = golden(f"g20_nucleus_{kind}.npz")
    model, _, _ = build(kind)
    kw = dict(G20_KW, max_len=int(g["max_len"]))       # (12; 8 for the two cross-attention models, see the recorder)
    for i in range(2):
        img = int(g[f"image_{i}"])
        assert float(g[f"margin_{i}"]) >= 1e-3
        with torch.no_grad():
            toks, lens = model.generate_batch(*model_args(kind, images, img, img + 1), seed=int(g[f"seed_{i}"]), rng="torch",
                                              top_p=float(g["top_p"]), **kw)
            assert toks[0, :int(lens[0])].cpu().tolist() == g[f"out_{i}"].tolist(), (kind, i)
            torch.manual_seed(int(g[f"seed_{i}"]))
            one = model.generate(*model_args(kind, images, img, img + 1), rng="torch", top_p=0.8, **kw)
            assert one.cpu().tolist() == g[f"out_{i}"].tolist()
            plain, plens = model.generate_batch(*model_args(kind, images, img, img + 1), seed=int(g[f"seed_{i}"]), rng="torch", **kw)
            assert plain[0, :int(plens[0])].cpu().tolist() == g[f"plain_{i}"].tolist()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_sixteen_bit_tokens_lie_inside_the_restated_nucleus(kind, dtype, images):
    """Every drawn token of a 16-bit call was inside the restated nucleus of the logits the call itself produced: a ``logits_hook``
    records each step's fp32 logits and, one step later, the tokens the engine wrote for them.  Rows whose boundary lies within 1e-4
    of ``top_p`` are left out (coin tosses); the call is also deterministic per seed and differs from ``top_p = 1``."""
    from oracle.ref_path import BeamBook
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = (torch.cat([images, images]).cuda(),)
    kw = dict(max_len=8, beam_size=3, top_k=50, temperature=1.0, seed=13)
    rec = []

    def hook(pos, logits, tokens):
        rec.append((pos, logits.detach().float().cpu().clone(), tokens.detach().cpu().clone()))
    hook.with_tokens = True
    with torch.no_grad():
        a = model.generate_batch(*args, top_p=0.8, logits_hook=hook, **kw)
        b = model.generate_batch(*args, top_p=0.8, **kw)
        c = model.generate_batch(*args, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool((a[0] != c[0]).any(1).sum() >= 1)
    checked = 0
    for (pos, logits, _), (_, _, after) in zip(rec[:-1], rec[1:]):
        n_img = after.shape[0] // 3
        rpi = logits.shape[0] // n_img                 # 1: the image's first draw (one source row), 3: its beam rows
        filt = BeamBook(1.0, 3, 50).keep_top_k(logits.clone())
        for img in range(n_img):
            # a new beam's token comes from one of the image's rows (which one, the candidate draw decided): the union of their
            # nuclei; a finished beam carries on with token 0 (beam.py:83-95)
            allowed, ok = ({0} if rpi > 1 else set()), True
            for r in range(img * rpi, (img + 1) * rpi):
                keep, margin = nucleus_keep(filt[r:r + 1], 1.0, 0.8, 3)
                ok = ok and margin >= 1e-4
                allowed |= set(keep[0].nonzero().flatten().tolist())
            if ok:
                assert set(after[img * 3:(img + 1) * 3, pos].tolist()) <= allowed, (kind, pos, img)
                assert len(allowed) < 3 * 50
                checked += 1
    assert checked >= 8


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_top_p_one_is_the_call_without_the_keyword(kind, images):
    from deephumor_amd import hip
    model, _, _ = build(kind)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=8, beam_size=3, top_k=20, seed=1)

    def same_bits(m):
        with torch.no_grad():
            a, b = m.generate_batch(*args, **kw), m.generate_batch(*args, top_p=1.0, **kw)
            c = m.generate_batch(*args, top_p=1, return_beams=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(c.best()[0], a[0])
    same_bits(model)

    def counts(**extra):
        with torch.no_grad(), hip.profile() as prof:
            model.generate_batch(*args, **kw, **extra)
        calls = {}
        for name, rec in prof.summary().items():
            calls[name.split("[")[0]] = calls.get(name.split("[")[0], 0) + rec["calls"]
        return calls
    for streams in (1, 2):
        plain, one, nuc = counts(streams=streams), counts(streams=streams, top_p=1.0), counts(streams=streams, top_p=0.8)
        assert plain == one and "dh_beam_row_sample_nucleus" not in one and plain.get("dh_beam_row_sample", 0) > 0
        assert nuc.get("dh_beam_row_sample_nucleus") == plain["dh_beam_row_sample"] and "dh_beam_row_sample" not in nuc
        rest = lambda c: {k: v for k, v in c.items() if not k.startswith("dh_beam_row_sample")}
        assert rest(nuc) == rest(plain)
    same_bits(model.bfloat16())


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------
KW = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2, top_p=0.8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_beams_prompts_batches_and_streams(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    with torch.no_grad():
        plain = model.generate_batch(*args, seed=31, **KW)
        nothing = model.generate_batch(*args, seed=31, **dict(KW, top_p=1.0))
        assert not torch.equal(plain[0], nothing[0])                         # the nucleus is not a no-op here
        beams = model.generate_batch(*args, seed=31, return_beams=True, **KW)
        assert torch.equal(beams.best()[0], plain[0]) and torch.equal(beams.best()[1], plain[1])
        two = model.generate_batch(*args, seed=31, streams=2, **KW)
        assert torch.equal(two[0], plain[0]) and torch.equal(two[1], plain[1])
        for i in range(4):                                                   # a batch equals its singles
            one = model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, **KW)
            assert torch.equal(one[0], plain[0][i:i + 1]) and torch.equal(one[1], plain[1][i:i + 1]), i
        cap = torch.randint(6, 1000, (4, 3), generator=torch.Generator().manual_seed(2)).cuda()
        lens = torch.tensor([0, 2, 1, 3])
        prompted = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **KW)
        for i, n in enumerate(lens.tolist()):
            one = model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, caption=cap[i:i + 1, :n] if n else None, **KW)
            assert torch.equal(one[0], prompted[0][i:i + 1]) and torch.equal(one[1], prompted[1][i:i + 1]), (i, n)
        ex = model.generate_batch(*args, seed=31, exact=True, **KW)
        assert torch.equal(ex[0], plain[0])


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay_beside_the_top_p_one_graph(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2)
    with torch.no_grad():
        for seed in (3, 4):
            nuc_g = model.generate_batch_graphed(*args, seed=seed, top_p=0.8, **kw)
            one_g = model.generate_batch_graphed(*args, seed=seed, top_p=1.0, **kw)
            nuc_e = model.generate_batch(*args, seed=seed, top_p=0.8, **kw)
            one_e = model.generate_batch(*args, seed=seed, **kw)
            assert torch.equal(nuc_g[0], nuc_e[0]) and torch.equal(nuc_g[1], nuc_e[1]), (kind, seed)
            assert torch.equal(one_g[0], one_e[0]) and torch.equal(one_g[1], one_e[1]), (kind, seed)
    assert len(model._graphs) == 2                               # top_p is in the cache key: two graphs side by side
    assert sorted(dict(k[2]).get("top_p") for k in model._graphs) == [0.8, 1.0]


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_pipeline(kind, images):
    from deephumor_amd.pipeline import CaptionPipeline
    model, _, _ = build(kind)
    model = model.bfloat16()
    batches = [(images[:2],), (images[2:],), (images[1:3],)]
    with torch.no_grad():
        want = [model.generate_batch(b[0].cuda(), seed=40 + i, **KW) for i, b in enumerate(batches)]
    pipe = CaptionPipeline(model, **KW)
    got = [tuple(t.clone() for t in r) for r in pipe.run(batches, seeds=[40, 41, 42])]
    for w, r in zip(want, got):
        assert torch.equal(w[0].cpu(), r[0].cpu()) and torch.equal(w[1].cpu(), r[1].cpu())
    for bad, exc in ((0, ValueError), (True, ValueError), ("0.8", TypeError)):
        with pytest.raises(exc):
            CaptionPipeline(model, top_p=bad)


CHILD = r"""
import datetime, json, os, socket, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
with socket.socket() as _s:
    _s.bind(("127.0.0.1", 0))
    _port = _s.getsockname()[1]
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT") or str(_port))
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=120))
from deephumor_amd.dist import generate_micro_sharded, generate_sharded
from deephumor_amd.models import CaptioningLSTM
from deephumor_amd.synth import load_synthetic, synth_images
model = load_synthetic(CaptioningLSTM(1000), seed=7).to(dev).eval()
images = synth_images(4, seed=0).to(dev)
kw = dict(max_len=10, beam_size=3, top_k=20, seed=11, top_p=0.8)
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, img0=0, **kw)
    plain = model.generate_batch(images, img0=0, **dict(kw, top_p=1.0))
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 2, always=True) for a in (0, 2)]
    got = tuple(torch.cat(ts, 0) for ts in zip(*halves))
    micro = generate_micro_sharded(fn, 4, 2, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want),
                              "differs": not same(plain, want)}))
dist.barrier()
dist.destroy_process_group()
"""


def test_batch_equals_sharded_halves_through_one_rank_rccl():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True, "differs": True}
