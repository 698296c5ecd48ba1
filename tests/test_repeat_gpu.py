"""``no_repeat_ngram_size`` / ``repetition_penalty`` on a real MI355X: ``dh_beam_history_logits`` bit for bit against the torch-CPU
restatement (``tests/repeat_ref.py``) -- logits, every group maximum, every word it must not touch --, the repaired group maxima
under the group-guided sampler, ``generate_batch`` against golden G21 recorded from the reference, and the keywords through every
layer that carries them."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import KINDS, captions_and_lengths, golden, synthetic_sd, synth_images  # noqa: E402
from repeat_ref import edit_logits, repeated_ngrams  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21_KW = dict(max_len=12, beam_size=3, top_k=50, temperature=1.3)
POISON_X, POISON_G, INF = 555.0, 777.0, float("inf")
UNK = 1


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
def make_case(v, rows, mult, L, seed):
    """Logits ``[rows, v]`` and a token table ``[rows * mult, max(L, 1) + 2]`` whose used rows (``r * mult``) hold: column 0, column
    ``v - 1`` and ``<unk>``; several tokens of group 1 (columns 64 ..), among them column 69, which every row's logits make the
    holder of that group's maximum; ids ``>= v`` and ``< 0``; and a small alphabet, so that bigrams and trigrams repeat.  With
    ``L >= 64`` row 0's history starts with ALL 64 columns of group 1 (``n = 1`` bans the whole group).  The table's other rows
    hold other tokens (a wrong row stride would show)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(rows, v, generator=g) * 3
    logits[:, 69] = 11.0
    logits[:, 3] = 0.0
    logits[:, 4] = -INF
    alphabet = torch.tensor([0, v - 1, UNK, 64, 65, 69, 70, 3, 4, v + 3, -1, 127 if v > 127 else 66])
    width = max(L, 1) + 2
    table = torch.randint(0, v, (rows * mult, width), generator=g, dtype=torch.int32)
    used = alphabet[torch.randint(0, len(alphabet), (rows, width), generator=g)].to(torch.int32)
    if L >= len(alphabet):                                # every symbol at least once, in every used row
        used[:, :len(alphabet)] = alphabet.to(torch.int32)[torch.randperm(len(alphabet), generator=g)]
    if L >= 64:
        used[0, :64] = torch.arange(64, 128, dtype=torch.int32)
    table[::mult] = used
    return logits, table


def launch(hip, x, v, gm, ng, table, mult, pos, rows, rpi, first_pos, n, penalty):
    hip._launch("dh_beam_history_logits", x.data_ptr(), x.stride(0), v, 0 if gm is None else gm.data_ptr(),
                0 if gm is None else gm.stride(0), ng, 64, table.data_ptr(), table.stride(0), mult, pos, rows, rpi,
                0 if first_pos is None else first_pos.data_ptr(), n, penalty, torch.cuda.current_stream().cuda_stream)


def run_case(hip, logits, table, mult, L, n, penalty, with_groups, rpi=1, first_pos=None, active=None):
    rows, v = logits.shape
    ng = (v + 63) // 64                                   # V = 130: 3 groups, the last of 2 columns
    x = torch.full((rows, v + 5), POISON_X)
    x[:, :v] = logits
    gm0 = torch.full((rows, ng + 1), POISON_G)
    dx, dt = x.cuda(), table.cuda()
    dg = gm0.cuda() if with_groups else None
    launch(hip, dx, v, dg, ng, dt, mult, L, rows, rpi, first_pos, n, penalty)
    want_x, want_g, stored = edit_logits(logits, table[::mult], L, n, penalty, gm0 if with_groups else None, 64, active=active)
    got = dx.cpu()
    assert torch.equal(got[:, :v], want_x), (v, rows, mult, L, n, penalty)
    assert bool((got[:, v:] == POISON_X).all())
    assert torch.equal(dt.cpu(), table)
    if with_groups:
        assert torch.equal(dg.cpu(), want_g), (v, rows, mult, L, n, penalty)
        assert bool((dg.cpu()[:, ng] == POISON_G).all())
    return want_x, want_g, stored


@pytest.mark.parametrize("v", [130, 1000, 4133])
def test_kernel_is_bit_exact(hip, v):
    """Every shape of the issue's list: rows 1 / 7, the dense first-step layout (one logits row per image, its tokens at row img *
    beam) and the normal one, ``L`` in {0, 1, n-1, n, 2n, 37, the bound}, ``n`` in 0 .. 3, penalty 1.0 / 1.3 / 0.8, with and
    without a group table.  Untouched logits, pad columns, untouched group words and the token table keep what they held."""
    bound = hip.MAX_HISTORY
    checked = banned_group = raised = 0
    for rows in (1, 7):
        for mult in (1, 3):
            for n in (0, 1, 2, 3):
                for penalty in (1.0, 1.3, 0.8):
                    if n == 0 and penalty == 1.0:
                        continue
                    for L in sorted({0, 1, max(n - 1, 0), n, 2 * n, 37, bound}):
                        logits, table = make_case(v, rows, mult, L, seed=v + 10 * n + L)
                        for with_groups in (False, True):
                            want_x, want_g, stored = run_case(hip, logits, table, mult, L, n, penalty, with_groups)
                        checked += 1
                        if L == 37:                       # the history holds what the docstring of make_case promises
                            h = set(table[::mult][:, :L].flatten().tolist())
                            assert {0, v - 1, UNK, 69, v + 3, -1} <= h
                            if penalty != 1.0:
                                assert bool(stored[:, [0, v - 1, UNK, 69]].all())
                            if penalty != 1.0 and n == 0:     # column 69 held group 1's maximum (11.0): it fell, or it rose
                                assert bool((want_g[:, 1] < 11.0).all() if penalty > 1 else (want_g[:, 1] > 11.0).all())
                                raised += penalty < 1
                        if L == bound and n == 1:
                            assert bool((want_x[0, 64:128] == -INF).all()) and want_g[0, 1] == -INF
                            banned_group += 1
    assert checked >= 100 and banned_group == 12 and raised >= 4


def test_kernel_prompted_phases(hip):
    """``first_pos`` at position 5: image 0 forced (5 < 7), image 1 at its first draw (its base row alone is active), image 2
    running.  Idle rows keep every word, logits and group maxima."""
    b, v, L = 3, 1000, 5
    logits, table = make_case(v, 3 * b, 1, L, seed=77)
    fp = torch.tensor([7, 5, 2], dtype=torch.int32, device="cuda")
    active = torch.tensor([False] * 3 + [True, False, False] + [True] * 3)
    for n, penalty in ((2, 1.0), (1, 1.3), (0, 0.8), (3, 1.3)):
        _, _, stored = run_case(hip, logits, table, 1, L, n, penalty, True, rpi=b, first_pos=fp, active=active)
        assert not stored[:3].any() and not stored[4:6].any()
        if penalty != 1.0:
            assert stored[3].any() and stored[6:].any(1).all()


def test_binding_uses_the_engine_group_layout(hip):
    """``hip.beam_history_logits`` passes ``hip.n_groups(V)`` groups of 64 columns (V = 130: four words per row, the last without a
    real column, which is never written)."""
    v, rows, L = 130, 4, 20
    logits, table = make_case(v, rows, 1, L, seed=5)
    gm0 = torch.full((rows, hip.n_groups(v)), POISON_G)
    x, gm = logits.cuda(), gm0.cuda()
    hip.beam_history_logits(x, v, table.cuda(), 1, L, rows, 1, 2, 1.3, group_max=gm)
    want_x, want_g, _ = edit_logits(logits, table, L, 2, 1.3, gm0, 64)
    assert torch.equal(x.cpu(), want_x) and torch.equal(gm.cpu(), want_g) and bool((gm.cpu()[:, 3] == POISON_G).all())


# ---- 2. the repaired group maxima under the group-guided sampler ------------------------------------------------------------------
def build(kind, v=None, **hp_over):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind, v)
    hp = dict(hp, **hp_over)
    model = getattr(M, kind)(**hp).eval()
    model.load_state_dict(sd)
    return model.cuda(), sd, hp


def sample(hip, route, x, v, gm, rows, beam, top_k, step):
    pi = torch.full((rows, beam), -7, dtype=torch.int32, device="cuda")
    pv = torch.full((rows, beam), -7.0, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    if route == "groups":
        hip.beam_row_sample_groups(x, v, gm, rows, beam, beam, top_k, 1.0, UNK, None, 9, 0, step, pi, pv, err)
    else:
        hip.beam_row_sample(x, v, rows, beam, beam, top_k, 1.0, UNK, None, 9, 0, step, pi, pv, err, exact=True)
    return pi.cpu(), pv.cpu(), int(err.item())


@pytest.mark.parametrize("kind,planes", [("CaptioningLSTM", False), ("CaptioningTransformer", True)],
                         ids=["bf16-lstm", "f32x-planes-transformer"])
def test_groups_sampler_on_the_edited_maxima_equals_the_exact_sampler(hip, kind, planes):
    """The logits and group maxima of the real classifiers, one small model each (``dh_vocab_logits`` on the bf16 operands of the
    LSTM model's classifier, ``dh_linear_f32xp`` on the split fp32 planes of the Transformer's; V = 1000), edited, then drawn by ``dh_beam_row_sample_groups`` -- which trusts the maxima --
    and by ``dh_beam_row_sample_exact`` -- which reads the whole row -- with the same Philox key: the same picks.  The histories are
    aimed at the bound: the row's top tokens banned (maxima must FALL), runners-up raised by a penalty below 1 (maxima must RISE)."""
    from deephumor_amd import f32xp
    model, _, _ = build(kind)
    w, bias = model.decoder.classifier.weight.detach(), model.decoder.classifier.bias.detach().float()
    v, k = w.shape
    rows, beam, top_k = 6, 3, 10
    assert top_k <= hip.n_groups(v)
    a = torch.randn(rows, k, generator=torch.Generator().manual_seed(4)).cuda()
    raw = torch.empty((rows, v), device="cuda")
    gm_raw = torch.empty((rows, hip.n_groups(v)), device="cuda")
    if planes:
        f32xp.linear(f32xp.split_act(a), hip.split_f32x(w.float().contiguous()), bias, out=raw, group_max=gm_raw)
    else:
        hip.vocab_logits(a.bfloat16(), w.bfloat16().contiguous(), bias, raw, gm_raw)
    order = raw.argsort(1, descending=True).to(torch.int32)
    for name, hist, n, penalty in (("ban the top 8", order[:, :8], 1, 1.0),
                                   ("raise ranks 9 .. 24", order[:, 8:24], 0, 0.5),
                                   ("both, and a bigram", torch.cat([order[:, :2], order[:, 12:20], order[:, :1]], 1), 2, 1.3)):
        L = hist.shape[1]
        x, gm = raw.clone(), gm_raw.clone()
        hip.beam_history_logits(x, v, hist.contiguous(), 1, L, rows, beam, n, penalty, group_max=gm)
        want_x, want_g, stored = edit_logits(raw.cpu(), hist.cpu(), L, n, penalty, gm_raw.cpu(), 64)
        assert torch.equal(x.cpu(), want_x) and torch.equal(gm.cpu(), want_g), name
        moved = (want_g != gm_raw.cpu()).sum().item()
        assert moved >= rows, name                       # the edits hit holders of group maxima: a stale table would be wrong
        gi, gv, gerr = sample(hip, "groups", x, v, gm, rows, beam, top_k, step=L)
        ei, ev, eerr = sample(hip, "exact", x, v, None, rows, beam, top_k, step=L)
        assert gerr == eerr == 0 and gi.tolist() == ei.tolist() and torch.equal(gv, ev), name
        if n == 1:
            for r in range(rows):                         # a ban is the row's own: no row drew a token of its own history
                assert not (set(gi[r].tolist()) & set(hist[r].tolist())), (name, r)


# ---- 3. model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0)


def model_args(kind, images, lo, hi):
    _, _, labels = captions_and_lengths()
    return (images[lo:hi].cuda(), labels[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


@pytest.mark.parametrize("kind", KINDS)
def test_sampled_caption_matches_the_reference(kind, images):
    """fp32, ``rng="torch"``: every G21 slot, token for token (the recorder kept only captions that 8 relative perturbations of 1e-4
    of the reference's logits do not move)."""
    g = golden(f"g21_repeat_{kind}.npz")
    model, _, _ = build(kind)
    kw = dict(G21_KW, max_len=int(g["max_len"]))
    for c in range(int(g["n_configs"])):
        ctl = dict(no_repeat_ngram_size=int(g[f"ngram_{c}"]), repetition_penalty=float(g[f"penalty_{c}"]))
        for i in range(2):
            img, seed = int(g[f"c{c}_image_{i}"]), int(g[f"c{c}_seed_{i}"])
            with torch.no_grad():
                toks, lens = model.generate_batch(*model_args(kind, images, img, img + 1), seed=seed, rng="torch", **ctl, **kw)
                assert toks[0, :int(lens[0])].cpu().tolist() == g[f"c{c}_out_{i}"].tolist(), (kind, c, i)
                torch.manual_seed(seed)
                one = model.generate(*model_args(kind, images, img, img + 1), rng="torch", **ctl, **kw)
                assert one.cpu().tolist() == g[f"c{c}_out_{i}"].tolist()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_no_beam_repeats_a_bigram(kind, dtype, images):
    """16-bit paths (group-guided sampler), ``return_beams=True``, ``no_repeat_ngram_size=2``: no beam holds a bigram twice within
    its own length -- without a prompt and behind a repeat-free prompt of its own length per image."""
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=12, beam_size=3, top_k=10, temperature=0.7, seed=3, return_beams=True)
    cap = torch.tensor([[17, 230, 45], [8, 9, 8], [300, 301, 302], [40, 41, 40]]).cuda()
    lens = torch.tensor([0, 3, 1, 2])
    with torch.no_grad():
        for extra in ({}, dict(caption=cap, caption_lengths=lens)):
            beams = model.generate_batch(*args, no_repeat_ngram_size=2, **extra, **kw)
            plain = model.generate_batch(*args, **extra, **kw)
            toks, blen = beams.tokens.cpu(), beams.lengths.cpu()
            for i in range(4):
                for j in range(3):
                    row = toks[i, j, :int(blen[i, j])].tolist()
                    assert not repeated_ngrams(row, 2), (kind, i, j, row)
            print(kind, dtype, "prompted" if extra else "dense", "beams that differ from the plain call:",
                  int((beams.tokens != plain.tokens).any(-1).sum()))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_default_route_equals_exact(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=12, beam_size=3, top_k=10, temperature=1.2, seed=5, repetition_penalty=1.3, no_repeat_ngram_size=3)
    with torch.no_grad():
        a, b = model.generate_batch(*args, **kw), model.generate_batch(*args, exact=True, **kw)
        c = model.generate_batch(*args, **dict(kw, repetition_penalty=1.0, no_repeat_ngram_size=0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])                              # the controls are not a no-op here


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_defaults_are_the_call_without_the_keywords(kind, images, monkeypatch):
    """Equal outputs and the same launches, counted at ``hip._launch``; with a control on, exactly one more launch per row draw."""
    from deephumor_amd import hip
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=8, beam_size=3, top_k=10, seed=1)
    names = []
    real = hip._launch

    def counting(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", counting)

    def run(**extra):
        del names[:]
        with torch.no_grad():
            out = model.generate_batch(*args, **kw, **extra)
        return out, list(names)
    run()                                                           # (weight plans are built on the first call)
    for streams in (1, 2):
        (p_t, p_l), p_names = run(streams=streams)
        (d_t, d_l), d_names = run(streams=streams, no_repeat_ngram_size=0, repetition_penalty=1.0)
        assert torch.equal(p_t, d_t) and torch.equal(p_l, d_l) and p_names == d_names
        assert "dh_beam_history_logits" not in d_names
        _, on = run(streams=streams, no_repeat_ngram_size=2)
        draws = sum(n.startswith("dh_beam_row_sample") for n in p_names)
        assert draws > 0 and on.count("dh_beam_history_logits") == draws and len(on) == len(p_names) + draws


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------
KW = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2, top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_top_p_prompts_batches_and_streams(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    with torch.no_grad():
        plain = model.generate_batch(*args, seed=31, **KW)
        nothing = model.generate_batch(*args, seed=31, **dict(KW, no_repeat_ngram_size=0, repetition_penalty=1.0))
        assert not torch.equal(plain[0], nothing[0])
        two = model.generate_batch(*args, seed=31, streams=2, **KW)
        assert torch.equal(two[0], plain[0]) and torch.equal(two[1], plain[1])
        for i in range(4):                                                   # a batch equals its singles
            one = model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, **KW)
            assert torch.equal(one[0], plain[0][i:i + 1]) and torch.equal(one[1], plain[1][i:i + 1]), i
        cap = torch.tensor([[17, 230, 45], [8, 9, 8], [300, 301, 302], [40, 41, 40]]).cuda()
        lens = torch.tensor([0, 3, 1, 2])
        prompted = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **KW)
        both = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, streams=2, **KW)
        assert torch.equal(both[0], prompted[0]) and torch.equal(both[1], prompted[1])
        for i, n in enumerate(lens.tolist()):
            one = model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, caption=cap[i:i + 1, :n] if n else None, **KW)
            assert torch.equal(one[0], prompted[0][i:i + 1]) and torch.equal(one[1], prompted[1][i:i + 1]), (i, n)
            assert not repeated_ngrams(prompted[0][i, :int(prompted[1][i])].tolist(), 2)
        ex = model.generate_batch(*args, seed=31, exact=True, **KW)
        assert torch.equal(ex[0], plain[0])


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay_beside_the_plain_graph(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2, top_p=0.8)
    ctl = dict(no_repeat_ngram_size=2, repetition_penalty=1.3)
    cap = torch.tensor([[17, 230, 45], [8, 9, 8], [300, 301, 302]]).cuda()
    lens = torch.tensor([0, 3, 2])
    with torch.no_grad():
        for seed in (3, 4):
            on_g = model.generate_batch_graphed(*args, seed=seed, **ctl, **kw)
            off_g = model.generate_batch_graphed(*args, seed=seed, **kw)
            on_e = model.generate_batch(*args, seed=seed, **ctl, **kw)
            off_e = model.generate_batch(*args, seed=seed, **kw)
            assert torch.equal(on_g[0], on_e[0]) and torch.equal(on_g[1], on_e[1]), (kind, seed)
            assert torch.equal(off_g[0], off_e[0]) and torch.equal(off_g[1], off_e[1]), (kind, seed)
        assert len(model._graphs) == 2                           # the controls are in the cache key: two graphs side by side
        assert sorted(dict(k[2]).get("no_repeat_ngram_size", 0) for k in model._graphs) == [0, 2]
        pr_g = model.generate_batch_graphed(*args, seed=3, caption=cap, caption_lengths=lens, **ctl, **kw)
        pr_e = model.generate_batch(*args, seed=3, caption=cap, caption_lengths=lens, **ctl, **kw)
        assert torch.equal(pr_g[0], pr_e[0]) and torch.equal(pr_g[1], pr_e[1])


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
    for bad, exc in ((dict(no_repeat_ngram_size=-1), ValueError), (dict(no_repeat_ngram_size=True), ValueError),
                     (dict(no_repeat_ngram_size=2.0), TypeError), (dict(repetition_penalty=0), ValueError),
                     (dict(repetition_penalty="1.3"), TypeError), (dict(repetition_penalty=1.3, max_len=5000), ValueError)):
        with pytest.raises(exc):
            CaptionPipeline(model, **bad)


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
kw = dict(max_len=10, beam_size=3, top_k=20, seed=11, top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3)
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, img0=0, **kw)
    plain = model.generate_batch(images, img0=0, **dict(kw, no_repeat_ngram_size=0, repetition_penalty=1.0))
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
