"""n-best output on a real MI355X: ``generate_batch(..., return_beams=True)`` returns every beam the search ends with
(``dh_beam_finalize_beams``), against golden G19 recorded from the reference, against the plain call, and through every layer
that carries it (sessions, graph replay, pipeline, sharding, text helpers)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import KINDS, PREFIX, captions_and_lengths, golden, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_beams import check_beams, own_lengths  # noqa: E402

G5_KW = dict(max_len=12, beam_size=3, top_k=20, temperature=1.3)
EOS = 3


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


def g19_cases(kind):
    cases = [("0", 0, None), ("1", 1, None)]
    if kind in ("CaptioningLSTM", "CaptioningTransformer"):
        cases.append(("prefix_0", 0, PREFIX))
    return cases


# ---- 1. reference parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_beam_matches_the_reference(kind, images):
    """fp32, ``rng="torch"``: every image's ``(row[:length], score)`` equals golden G19's in slot order, ``best()`` is the
    reference's own output.  Tokens exact; scores within 2e-3 x the image's draw steps (the fp32 logit gate is 1e-3 and every step
    adds one log_softmax over B gathered logits, whose error is at most twice the logit error)."""
    g = golden(f"g19_beams_{kind}.npz")
    model, _, _ = build(kind)
    for tag, i, cap in g19_cases(kind):
        rows, scores = g[f"rows_{tag}"], g[f"scores_{tag}"]
        first = int(g[f"first_col_{tag}"])
        with torch.no_grad():
            beams = model.generate_batch(*model_args(kind, images, i, i + 1), caption=None if cap is None else cap.cuda(),
                                         seed=int(g[f"seed_{tag}"]), rng="torch", return_beams=True, **G5_KW)
        order = np.argsort(-scores, kind="stable")
        steps = rows.shape[1] - first
        for slot, j in enumerate(order.tolist()):
            hits = np.nonzero(rows[j, first:] == EOS)[0]
            want_len = first + int(hits[0]) + 1 if hits.size else rows.shape[1]
            got_len = int(beams.lengths[0, slot])
            print(kind, tag, "slot", slot, "engine beam", int(beams.beam_index[0, slot]), "length", got_len, want_len,
                  "score", float(beams.scores[0, slot]), float(scores[j]))
            assert got_len == want_len, (kind, tag, slot)
            assert beams.tokens[0, slot, :got_len].cpu().tolist() == rows[j, :want_len].tolist(), (kind, tag, slot)
            assert int(beams.beam_index[0, slot]) == j
            assert abs(float(beams.scores[0, slot]) - float(scores[j])) <= 2e-3 * steps, (kind, tag, slot)
        toks, lens = beams.best()
        assert toks[0, :int(lens[0])].cpu().tolist() == g[f"out_{tag}"].tolist(), (kind, tag)
        assert int(beams.beam_index[0, int(beams.drawn[0])]) == int(g[f"drawn_{tag}"])
        # generate(..., return_beams=True): the one image's BeamCaptions, nothing squeezed
        torch.manual_seed(int(g[f"seed_{tag}"]))
        with torch.no_grad():
            one = model.generate(*model_args(kind, images, i, i + 1), caption=None if cap is None else cap.cuda(), rng="torch",
                                 return_beams=True, **G5_KW)
        assert all(torch.equal(a, b) for a, b in zip(one, beams)) and tuple(one.tokens.shape) == (1, 3, 12)


# ---- 2 + 3. consistency with the plain call, invariants -------------------------------------------------------------------------
def both(model, args, first_cols, pad=0, **kw):
    with torch.no_grad():
        plain = model.generate_batch(*args, **kw)
        beams = model.generate_batch(*args, return_beams=True, **kw)
    check_beams(beams, plain, pad, torch.as_tensor(first_cols).cuda(), tag=kw)
    return beams, plain


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_best_is_the_plain_call_bit_for_bit(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=14, beam_size=5, top_k=20, temperature=1.1, seed=77)
    both(model, args, 0, **kw)
    both(model, args, 0, streams=2, **kw)
    both(model, args, 0, early_stop_every=2, **kw)
    cap = torch.randint(6, 1000, (4, 5), generator=torch.Generator().manual_seed(2)).cuda()
    cap[:, 1] = EOS                       # an <eos> inside the teacher-forced columns is not a beam's end: only the first
    cap[2, 4] = EOS                       # generated column onwards counts (pos / first_pos reach the kernel)
    both(model, args, 5, caption=cap, **kw)
    lens = torch.tensor([0, 5, 2, 3])     # image 0: column 1 is its own; images 1-3: the prompt's <eos> sits below first_pos
    both(model, args, lens, caption=cap, caption_lengths=lens, **kw)
    both(model, args, lens, caption=cap, caption_lengths=lens, streams=2, **kw)


@pytest.mark.parametrize("beam", [1, 5, 24, 64])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_beam_sizes(kind, beam, images):
    model, _, _ = build(kind)
    for m in (model, model.bfloat16()):
        both(m, model_args(kind, images, 0, 2), 0, max_len=9, beam_size=beam, top_k=max(beam, 30), temperature=1.2, seed=5)


@pytest.mark.parametrize("pad", [1, 7])
@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningTransformerBase"))
def test_pad_index_other_than_zero(kind, pad, images):
    model, _, _ = build(kind, pad_index=pad)
    args = model_args(kind, images, 0, 2)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.3, seed=9)
    both(model, args, 0, pad=pad, **kw)
    cap = torch.tensor([[17, EOS, 45], [9, 88, EOS]]).cuda()       # <eos> in the prefix (the reforward session's pos too)
    both(model, args, 3, pad=pad, caption=cap, **kw)
    if pad != 1:
        both(model.bfloat16(), args, 0, pad=pad, **kw)


def test_lstm_no_decode_step(images):
    """The prefix fills ``max_len - 1``: no decode step runs and the reference returns beam 0 -- ``drawn`` then points at it."""
    model, _, _ = build("CaptioningLSTM")
    cap = torch.randint(6, 1000, (2, 7), generator=torch.Generator().manual_seed(4)).cuda()
    cap[0, 3] = EOS
    beams, _ = both(model, model_args("CaptioningLSTM", images, 0, 2), 7, caption=cap, max_len=8, beam_size=4, top_k=20, seed=3)
    assert beams.beam_index.gather(1, beams.drawn[:, None]).flatten().tolist() == [0, 0]


def test_fuzz_one_seed():
    import fuzz_beams
    assert fuzz_beams.run(seed=0, cases=10) == 10


# ---- 4. ordering and dead beams -------------------------------------------------------------------------------------------------
def test_equal_scores_keep_engine_order_and_nan_sorts_last():
    from deephumor_amd import hip
    n, b, t = 3, 6, 70                                   # more than one 64-column round
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(4, 50, (n * b, t), generator=g, dtype=torch.int32).to(dev)
    tokens[1, 66] = EOS                                  # an <eos> in the second round of columns
    tokens[2, 1] = EOS                                   # before the first generated column: not the beam's end
    tokens[2, 9] = EOS
    vals = torch.tensor([[-1.0, -2.0, -1.0, -2.0, -0.5, -1.0],
                         [float("-inf"), -3.0, float("nan"), -3.0, float("-inf"), -0.25],
                         [-4.0, -4.0, -4.0, -4.0, -4.0, -4.0]], device=dev).flatten()
    done = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    end_step = torch.tensor([0, 40, 0], dtype=torch.int32, device=dev)
    out = torch.empty((n, b, t), dtype=torch.int32, device=dev)
    o_len, o_idx = (torch.empty((n, b), dtype=torch.int32, device=dev) for _ in range(2))
    o_score = torch.empty((n, b), device=dev)
    o_drawn, o_row = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
    noise = torch.ones((n, b), device=dev)
    hip.beam_finalize_beams(tokens, vals, done, end_step, out, o_len, o_score, o_idx, o_drawn, o_row, n, b, 1, t, 0, EOS, 3, None,
                            1.0, noise, 0, 0)
    plain, plain_len = torch.empty((n, t), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
    hip.beam_finalize(tokens, vals, done, end_step, plain, plain_len, n, b, 1, t, 0, 1.0, noise, 0, 0)
    assert o_idx.tolist() == [[4, 0, 2, 5, 1, 3], [5, 1, 3, 0, 2, 4], [0, 1, 2, 3, 4, 5]]
    assert o_row.tolist() == [t, 41, t] == plain_len.tolist()
    assert o_score[0].tolist() == [-0.5, -1.0, -1.0, -1.0, -2.0, -2.0]
    for i in range(n):
        assert torch.equal(out[i, int(o_drawn[i])], plain[i])
        for slot in range(b):
            src = tokens[i * b + int(o_idx[i, slot])]
            L = int(o_row[i])
            assert torch.equal(out[i, slot, :L], src[:L]) and bool((out[i, slot, L:] == 0).all())
    want = own_lengths(out.long(), o_row.long(), torch.full((n,), 3, device=dev))
    assert torch.equal(o_len.long(), want)
    assert int(o_len[0, 2]) == 10 and int(o_len[0, 4]) == 67          # engine beams 2 (eos at 9, not 1) and 1 (eos at 66)
    # per-image first columns (prompted batches)
    fp = torch.tensor([10, 0, 0], dtype=torch.int32, device=dev)
    hip.beam_finalize_beams(tokens, vals, done, end_step, out, o_len, o_score, o_idx, o_drawn, o_row, n, b, 1, t, 0, EOS, 3, fp,
                            1.0, noise, 0, 0)
    assert torch.equal(o_len.long(), own_lengths(out.long(), o_row.long(), fp.long()))
    assert int(o_len[0, 2]) == t


def test_dead_beams_sort_last(images):
    """``top_k == beam_size`` with ``<unk>`` forced into the top-k: the first draw has fewer live tokens than beams (ERR_TOO_FEW) and
    fills up with a dead beam at score -inf.  A candidate draw never picks a dead candidate while enough live ones exist, so the
    dead beam is still there at the end only when no further draw runs: the LSTM at ``max_len=1``."""
    kind = "CaptioningLSTM"
    model, _, _ = build(kind)
    with torch.no_grad():
        model.decoder.classifier.bias[1] += 100.0
    beams, _ = both(model, model_args(kind, images, 0, 2), 0, max_len=1, beam_size=4, top_k=4, temperature=1.0, seed=21)
    assert bool(torch.isinf(beams.scores[:, -1]).all()) and bool(torch.isfinite(beams.scores[:, :3]).all())
    assert beams.beam_index[:, -1].tolist() == [3, 3]
    assert beams.beam_index.gather(1, beams.drawn[:, None]).flatten().tolist() == [0, 0]      # no decode step: engine beam 0


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_too_few_live_tokens_keeps_the_invariants(kind, images):
    """The same setting over whole captions: the Transformer always re-draws once more (transformers.py:557), after which no -inf
    score is left, so this run only holds ``best()`` and the invariants; -inf and NaN scores at the kernel are covered above."""
    model, _, _ = build(kind)
    with torch.no_grad():
        model.decoder.classifier.bias[1] += 100.0
    for max_len in (1, 8):
        both(model, model_args(kind, images, 0, 2), 0, max_len=max_len, beam_size=4, top_k=4, temperature=1.0, seed=21)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_overflow_retry_returns_the_same_type(kind, images):
    """Flat logits overflow the pre-filtered samplers (``BeamOverflow``): the repeated batch is a ``BeamCaptions`` too."""
    import warnings
    model, _, _ = build(kind)
    model = model.bfloat16()
    with torch.no_grad():
        model.decoder.classifier.weight.zero_()
        model.decoder.classifier.bias.zero_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        both(model, model_args(kind, images, 0, 2), 0, max_len=6, beam_size=3, top_k=20, seed=5)


# ---- 5. batch invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformerWithLabels"))
def test_batch_equals_singles(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    kw = dict(max_len=11, beam_size=4, top_k=20, temperature=1.2, seed=31, return_beams=True)
    with torch.no_grad():
        whole = model.generate_batch(*model_args(kind, images, 0, 4), **kw)
        for i in range(4):
            one = model.generate_batch(*model_args(kind, images, i, i + 1), img0=i, **kw)
            for name, a, b in zip(whole._fields, whole, one):
                assert torch.equal(a[i:i + 1], b), (kind, i, name)


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
from deephumor_amd.dist import gather_beams, generate_micro_sharded, generate_sharded
from deephumor_amd.models import CaptioningLSTM
from deephumor_amd.synth import load_synthetic, synth_images
model = load_synthetic(CaptioningLSTM(1000), seed=7).to(dev).eval()
images = synth_images(6, seed=0).to(dev)
kw = dict(max_len=10, beam_size=3, top_k=20, seed=11, return_beams=True)
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, img0=0, **kw)
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 3, always=True) for a in (0, 3)]
    got = type(want).cat(halves)
    micro = generate_micro_sharded(fn, 6, 4, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
bits = bool(torch.equal(got.scores.view(torch.int32), want.scores.view(torch.int32)))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want), "bits": bits}))
dist.barrier()
dist.destroy_process_group()
"""


def test_batch_equals_sharded_halves_through_one_rank_rccl():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True, "bits": True}


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay_beside_the_plain_graph(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2)
    with torch.no_grad():
        for seed in (3, 4, 5):
            plain_g = model.generate_batch_graphed(*args, seed=seed, **kw)
            beams_g = model.generate_batch_graphed(*args, seed=seed, return_beams=True, **kw)
            plain_e = model.generate_batch(*args, seed=seed, **kw)
            beams_e = model.generate_batch(*args, seed=seed, return_beams=True, **kw)
            assert all(torch.equal(a, b) for a, b in zip(beams_g, beams_e)), (kind, seed)
            assert torch.equal(plain_g[0], plain_e[0]) and torch.equal(plain_g[1], plain_e[1])
            check_beams(beams_g, plain_g, 0, torch.zeros(3, dtype=torch.int64).cuda())
    assert len(model._graphs) == 2


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_pipeline_yields_beam_captions(kind, images):
    from deephumor_amd.models.beam import BeamCaptions
    from deephumor_amd.pipeline import CaptionPipeline
    model, _, _ = build(kind)
    model = model.bfloat16()
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2)
    batches = [(images[:2],), (images[2:],), (images[1:3],)]
    with torch.no_grad():
        want = [model.generate_batch(b[0].cuda(), seed=40 + i, return_beams=True, **kw) for i, b in enumerate(batches)]
    for to_host in (True, False):
        pipe = CaptionPipeline(model, return_beams=True, **kw)
        got = [r.map(torch.Tensor.clone) for r in pipe.run(batches, seeds=[40, 41, 42], to_host=to_host)]
        for w, r in zip(want, got):
            assert isinstance(r, BeamCaptions) and r.tokens.is_cuda != to_host
            assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(w, r))
    with pytest.raises(TypeError):
        CaptionPipeline(model, return_beams=1)


# ---- 8. rank_beams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_rank_beams(kind, images):
    from deephumor_amd.experiments import rank_beams, score_captions
    model, _, _ = build(kind)
    imgs = images[:2].cuda()
    with torch.no_grad():
        beams = model.generate_batch(imgs, max_len=10, beam_size=4, top_k=20, temperature=1.2, seed=8, return_beams=True)
        order, pp = rank_beams(model, imgs, beams)
        n, b, t = beams.tokens.shape
        lens = beams.lengths.reshape(-1)
        rows = beams.tokens.reshape(n * b, t).clone()
        rows[torch.arange(t, device="cuda")[None, :] >= lens[:, None]] = 0
        by_hand = score_captions(model, imgs, torch.arange(n, device="cuda").repeat_interleave(b), rows, lens).view(n, b)
        assert torch.equal(pp, by_hand)
        assert torch.equal(order, torch.argsort(pp, dim=1, stable=True))
        assert bool((pp.gather(1, order)[:, 1:] >= pp.gather(1, order)[:, :-1]).all())
        # exp(-mean log_softmax) of the teacher-forced forward() logits
        logits = model(imgs.repeat_interleave(b, 0), rows[:, :-1])[:, :t].float()
        logp = logits.log_softmax(-1).gather(-1, rows[:, :, None])[..., 0]
        keep = torch.arange(t, device="cuda")[None, :] < lens[:, None]
        want = torch.exp(-(logp * keep).sum(1) / lens).view(n, b)
    for g, w in zip(pp.flatten().tolist(), want.flatten().tolist()):
        assert abs(g - w) < 2e-3 * w, (g, w)             # the tolerance of tests/test_scoring_gpu.py for this comparison


# ---- 9. default path untouched ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_launch_counts(kind, images):
    from deephumor_amd import hip
    model, _, _ = build(kind)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=8, beam_size=3, top_k=20, seed=1)

    def counts(**extra):
        with torch.no_grad(), hip.profile() as prof:
            model.generate_batch(*args, **kw, **extra)
        calls = {}
        for name, rec in prof.summary().items():
            calls[name.split("[")[0]] = calls.get(name.split("[")[0], 0) + rec["calls"]
        return calls
    for streams in (1, 2):
        plain, beams = counts(streams=streams), counts(streams=streams, return_beams=True)
        assert plain.get("dh_beam_finalize") == streams and "dh_beam_finalize_beams" not in plain
        assert beams.get("dh_beam_finalize_beams") == streams and "dh_beam_finalize" not in beams
        rest = lambda c: {k: v for k, v in c.items() if not k.startswith("dh_beam_finalize")}
        assert rest(plain) == rest(beams)                # nothing else changes
