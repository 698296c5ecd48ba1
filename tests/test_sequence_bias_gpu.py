"""``sequence_bias`` on a real MI355X: ``dh_beam_bias_logits`` bit for bit against the torch-CPU restatement (``tests/bias_ref.py``) --
logits, every group maximum, every word it must not touch --, the repaired group maxima under the group-guided sampler and
``dh_beam_row_best``, ``generate_batch`` step by step against the restatements, and the keyword through every layer that carries it."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from beam_search_ref import State, candidate_gaps, row_best, select_best  # noqa: E402
from bias_ref import CASE_VS, NEG_INF, UNK, bias_logits, bits, flatten_sorted, kernel_cases  # noqa: E402
from helpers import KINDS, captions_and_lengths, golden, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_X, POISON_G = 555.0, 777.0
NAME = "dh_beam_bias_logits"


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
def launch(hip, x, v, gm, ng, table, mult, pos, rows, rpi, first_pos, words, offs, bias, runs, n_words, n_runs):
    hip._launch(NAME, x.data_ptr(), x.stride(0), v, 0 if gm is None else gm.data_ptr(), 0 if gm is None else gm.stride(0), ng, 64,
                table.data_ptr(), table.stride(0), mult, pos, rows, rpi, 0 if first_pos is None else first_pos.data_ptr(),
                words.data_ptr(), offs.data_ptr(), bias.data_ptr(), runs.data_ptr(), n_words, n_runs, torch.cuda.current_stream().cuda_stream)


def run_case(hip, c, with_groups, rpi=1, first_pos=None, active=None):
    """One launch on a copy of the case: logits in a wider buffer (pad columns poisoned), group words pre-filled with a sentinel and
    one word more than there are groups.  The logits are compared word for word (int32 views), edited groups equal the exact
    maximum, every other group word is still the sentinel, the token table and the list are untouched."""
    v, rows, mult, pos, pairs = c["v"], c["rows"], c["mult"], c["pos"], c["pairs"]
    ng = (v + 63) // 64                                   # V = 130: 3 groups, the last of 2 real columns
    x = torch.full((rows, v + 5), POISON_X)
    x[:, :v] = c["logits"]
    gm0 = torch.full((rows, ng + 1), POISON_G)
    host = flatten_sorted(pairs)
    dev = [t.cuda() for t in host]
    dx, dt = x.cuda(), c["table"].cuda()
    dg = gm0.cuda() if with_groups else None
    launch(hip, dx, v, dg, ng, dt, mult, pos, rows, rpi, first_pos, *dev, len(pairs), host[3].numel() - 1)
    want_x, want_g, stored = bias_logits(c["logits"], c["table"][::mult], pos, pairs, gm0 if with_groups else None, 64, active=active)
    got = dx.cpu()
    tag = (v, rows, mult, pos, with_groups)
    assert torch.equal(bits(got[:, :v]), bits(want_x)), tag
    assert torch.equal(bits(got[:, :v][~stored]), bits(c["logits"][~stored])), tag          # untouched words: the input's
    assert bool((got[:, v:] == POISON_X).all()), tag
    assert torch.equal(dt.cpu(), c["table"]) and all(torch.equal(d.cpu(), h) for d, h in zip(dev, host))
    if with_groups:
        got_g = dg.cpu()
        assert torch.equal(bits(got_g), bits(want_g)), tag
        touched = torch.zeros((rows, ng + 1), dtype=torch.bool)
        touched[:, :ng] = torch.nn.functional.pad(stored.to(torch.uint8), (0, ng * 64 - v)).view(rows, ng, 64).any(-1)
        assert bool((got_g[~touched] == POISON_G).all()), tag                 # every other word is still the sentinel
        exact = torch.nn.functional.pad(want_x, (0, ng * 64 - v), value=NEG_INF).view(rows, ng, 64).max(-1).values
        assert torch.equal(got_g[:, :ng][touched[:, :ng]], exact[touched[:, :ng]]), tag
    return want_x, want_g, stored


@pytest.mark.parametrize("v", CASE_VS)
def test_kernel_is_bit_exact(hip, v):
    """The cases of ``bias_ref.kernel_cases``: 12 rows at ``pos`` 0 / 1 / 5 / 40 and the dense first step (4 rows, ``tok_row_mult =
    3``), 300 pairs each, with and without a group table."""
    cases = kernel_cases(v)
    assert len(cases) == 5
    for c in cases:
        for with_groups in (False, True):
            want_x, want_g, stored = run_case(hip, c, with_groups)
        assert bool((want_x[:, 69] == 2.0).all()) and bool((want_g[:, 1] == 9.0).all())      # the lowered maximum: the group's second value
        assert bool((want_x[:, 4] == NEG_INF).all()) and bool(stored[:, 4].all())
        assert bool((want_g[:, 0] == want_x[:, :64].max(1).values).all()) and bool((want_g[:, 0] >= c["logits"][:, 8] + 40.0).all())
        assert bool(stored[0, v - 1]) == (c["pos"] >= 1)


def test_kernel_prompted_phases(hip):
    """``first_pos`` at position 5: image 0 forced (5 < 7), image 1 at its first draw (its base row alone is active), image 2
    running, image 3 forced.  Idle rows keep every word, logits and group maxima."""
    c = kernel_cases(1000)[2]
    assert c["pos"] == 5 and c["rows"] == 12
    fp = torch.tensor([7, 5, 2, 6], dtype=torch.int32, device="cuda")
    active = torch.tensor([False] * 3 + [True, False, False] + [True] * 3 + [False] * 3)
    for with_groups in (True, False):
        _, _, stored = run_case(hip, c, with_groups, rpi=3, first_pos=fp, active=active)
        assert not stored[:3].any() and not stored[4:6].any() and not stored[9:].any()
        assert stored[3].any() and stored[6:9].any(1).all()


# ---- 2. the repaired group maxima under the group-guided sampler and dh_beam_row_best -----------------------------------------------
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
    elif route == "exact":
        hip.beam_row_sample(x, v, rows, beam, beam, top_k, 1.0, UNK, None, 9, 0, step, pi, pv, err, exact=True)
    else:
        hip.beam_row_best(x, v, rows, beam, beam, 1.0, UNK, step, pi, pv, err, group_max=gm if route == "best-groups" else None)
    return pi.cpu(), pv.cpu(), int(err.item())


@pytest.mark.parametrize("kind,planes", [("CaptioningLSTM", False), ("CaptioningTransformer", True)],
                         ids=["bf16-lstm", "f32x-planes-transformer"])
def test_samplers_on_the_repaired_maxima_equal_the_exact_ones(hip, kind, planes):
    """The logits and group maxima of the real classifiers, one small model each (``dh_vocab_logits`` on the bf16 operands of the
    LSTM model's classifier, ``dh_linear_f32xp`` on the split fp32 planes of the Transformer's; V = 1000), biased through the public
    binding, then drawn by ``dh_beam_row_sample_groups`` -- which trusts the maxima -- and by the exact sampler -- which reads the
    whole row -- with the same Philox key: the same picks; and ``dh_beam_row_best`` with and without the maxima: the same picks and
    values.  Three lists: every row's OWN top 8 tokens lowered by 30 (row ``r``'s history ends in a marker ``900 + r``), so the maxima
    of the groups that bound the top-k must FALL; every row's own 30th .. 32nd tokens RAISED by 20, from outside the top-k
    into it, so maxima must RISE -- a stale table hides exactly these columns from the groups sampler --; and both at once with
    singles on top."""
    from deephumor_amd import f32xp
    from deephumor_amd.models.beam import compile_sequence_bias
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
    order = raw.argsort(1, descending=True).cpu()
    order = torch.stack([o[o != UNK] for o in order])                       # (<unk> is never drawn: keep it out of the planted ranks)
    pos = 4
    table = torch.randint(0, 800, (rows, pos + 2), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    table[:, pos - 1] = 900 + torch.arange(rows, dtype=torch.int32)
    down = [([900 + r, int(t)], -30.0) for r in range(rows) for t in order[r, :8]]
    up = [([900 + r, int(t)], 20.0) for r in range(rows) for t in order[r, 30:33]]
    singles = [([int(t)], -25.0) for t in order[0, :3]] + [([int(order[1, 500])], 20.0)]
    for name, plist in (("own top 8 lowered", down), ("ranks 30 .. 32 raised", up), ("both, and singles", up + singles + down)):
        sb = compile_sequence_bias(plist, v, "cuda")
        x, gm = raw.clone(), gm_raw.clone()
        hip.beam_bias_logits(x, v, table.cuda(), 1, pos, rows, beam, sb.words, sb.offsets, sb.bias, sb.run_off, len(sb), sb.n_runs, group_max=gm)
        want_x, want_g, stored = bias_logits(raw.cpu(), table, pos, plist, gm_raw.cpu(), 64)
        assert torch.equal(bits(x.cpu()), bits(want_x)) and torch.equal(bits(gm.cpu()), bits(want_g)), name
        if plist is down:
            assert int((want_g < gm_raw.cpu()).sum()) >= rows, name             # maxima FELL: a stale table would be wrong
        if plist is up:
            assert int((want_g > gm_raw.cpu()).sum()) >= rows, name             # maxima ROSE
            top = want_x.argsort(1, descending=True)[:, :top_k]
            for r in range(rows):                                               # from outside the top-k into it
                assert all(int(t) in top[r].tolist() for t in order[r, 30:33]), r
        gi, gv, gerr = sample(hip, "groups", x, v, gm, rows, beam, top_k, step=pos)
        ei, ev, eerr = sample(hip, "exact", x, v, None, rows, beam, top_k, step=pos)
        assert gerr == eerr == 0 and gi.tolist() == ei.tolist() and torch.equal(gv, ev), name
        bi, bv, berr = sample(hip, "best-groups", x, v, gm, rows, beam, top_k, step=pos)
        pi, pv, perr = sample(hip, "best", x, v, None, rows, beam, top_k, step=pos)
        assert berr == perr == 0 and bi.tolist() == pi.tolist() and torch.equal(bits(bv), bits(pv)), name
        picks, _, _ = row_best(want_x, 1.0, beam, UNK)
        assert bi.tolist() == picks.tolist(), name


# ---- 3. model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0)


def model_args(kind, images, lo, hi):
    _, _, labels = captions_and_lengths()
    return (images[lo:hi].cuda(), labels[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


G24_KW = dict(beam_size=3, top_k=50, temperature=1.3)


def g24_pairs(g, slot):
    words, offs, bias = g[f"words_{slot}"].tolist(), g[f"offsets_{slot}"].tolist(), g[f"bias_{slot}"].tolist()
    return [(words[a:b], x) for a, b, x in zip(offs[:-1], offs[1:], bias)]


@pytest.mark.parametrize("kind", KINDS)
def test_sampled_caption_matches_the_reference(kind, images):
    """fp32, ``rng="torch"``: every G24 slot, token for token (the recorder kept only captions that 8 relative perturbations of 1e-4
    of the reference's logits do not move); as a list of pairs and as a mapping."""
    g = golden(f"g24_sequence_bias_{kind}.npz")
    model, _, _ = build(kind)
    kw = dict(G24_KW, max_len=int(g["max_len"]))
    for i in range(int(g["n_slots"])):
        pairs = g24_pairs(g, i)
        img, seed, boost = int(g[f"image_{i}"]), int(g[f"seed_{i}"]), int(g[f"boost_{i}"])
        with torch.no_grad():
            toks, lens = model.generate_batch(*model_args(kind, images, img, img + 1), seed=seed, rng="torch", sequence_bias=pairs, **kw)
            assert toks[0, :int(lens[0])].cpu().tolist() == g[f"out_{i}"].tolist(), (kind, i)
            assert boost in toks[0].tolist()
            torch.manual_seed(seed)
            one = model.generate(*model_args(kind, images, img, img + 1), rng="torch", sequence_bias={tuple(w): b for w, b in pairs}, **kw)
            assert one.cpu().tolist() == g[f"out_{i}"].tolist()
            plain, pl = model.generate_batch(*model_args(kind, images, img, img + 1), seed=seed, rng="torch", **kw)
            assert plain[0, :int(pl[0])].cpu().tolist() == g[f"plain_{i}"].tolist()


def rows_of(toks, lens):
    return [toks[i, :int(lens[i])].tolist() for i in range(toks.shape[0])]


def absent_token(rows, v=1000):
    """A token no row holds, not a special one."""
    held = {t for r in rows for t in r}
    return next(t for t in range(10, v) if t not in held)


def biting_bias(model, args, kw):
    """``(sequence_bias, boosted token, plain result)`` from the call without the keyword: +60 on a token no plain caption holds (far
    above the spread of the synthetic models' logits, some 30 from end to end, so every row draws it), -8 on every plain caption's first token, and +6 on the
    third token of every plain caption behind its second."""
    with torch.no_grad():
        t0, l0 = model.generate_batch(*args, **kw)
    rows = rows_of(t0, l0)
    boost = absent_token(rows)
    bias = [((boost,), 60.0)] + [((r[0],), -8.0) for r in rows] + [(tuple(r[1:3]), 6.0) for r in rows if len(r) >= 3]
    bias = list(dict(bias).items())                         # (a phrase two captions share is listed once: the mapping is the list)
    return bias, boost, (t0, l0)


def snapshots(monkeypatch):
    """Every beam step of the calls made from now on: the raw logits and the engine's own state in front of and behind each."""
    from deephumor_amd.models.beam import BeamSearchHelper
    steps = []
    real_step = BeamSearchHelper._draw_and_select
    c = lambda t: None if t is None else t.detach().cpu().clone()

    def state_of(h):
        return dict(tokens=c(h.tokens), vals=c(h.vals), ended=c(h._ended), done=c(h.done), end_step=c(h.end_step), src=c(h.src))

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        rec = dict(logits=c(logits.float()), first=first, write_pos=write_pos, t=t, step=step_index, before=state_of(self),
                   temperature=self.temperature, unk=self.unk_index, eos=self.eos_index, beam=self.beam_size)
        real_step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted)
        rec["after"] = state_of(self)
        rec["biased"] = c(logits.float())
        rec["pick_idx"], rec["pick_val"], rec["pick_lp"] = c(self.pick_idx), c(self.pick_val), c(self.pick_lp)
        steps.append(rec)
    monkeypatch.setattr(BeamSearchHelper, "_draw_and_select", step)
    return steps


GAP, VAL_TOL = 1e-3, 2e-5        # (tests/test_beam_search_gpu.py: a candidate gap below GAP is a coin toss under the row step's fp32 error)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_beam_search_scores_are_those_of_the_biased_rows(kind, images, monkeypatch):
    """fp32, ``search="beam"``: at every step the logits the engine leaves behind are the restatement of the raw ones bit for bit,
    and tokens, flags and scores are what ``tests/beam_search_ref.py`` computes FROM THE BIASED ROWS (steps whose candidates lie
    closer than ``GAP`` are left out, as there); the boosted token is in every caption."""
    model, _, _ = build(kind)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=8, beam_size=3, top_k=20, search="beam")
    bias, boost, plain = biting_bias(model, args, kw)
    steps = snapshots(monkeypatch)
    with torch.no_grad():
        beams = model.generate_batch(*args, sequence_bias=bias, return_beams=True, **kw)
    assert len(steps) == 8 + (0 if "LSTM" in kind else 1)
    checked = skipped = 0
    for rec in steps:
        b = rec["beam"]
        if rec["write_pos"] >= rec["before"]["tokens"].shape[1]:
            continue
        mult = b if rec["first"] else 1
        want_x, _, stored = bias_logits(rec["logits"], rec["before"]["tokens"][::mult], rec["write_pos"], bias)
        assert torch.equal(bits(rec["biased"]), bits(want_x)), rec["step"]
        assert bool(stored[:, boost].all())
        st = State.of(beam=b, **rec["before"])
        picks, vals, _ = row_best(want_x, rec["temperature"], b, rec["unk"])
        gaps = candidate_gaps(st, picks, vals, rec["first"], None, rec["step"])
        select_best(st, picks, vals.to(torch.float32), rec["first"], rec["write_pos"], rec["t"], rec["step"], rec["eos"])
        for img, gap in enumerate(gaps):
            if gap < GAP:
                skipped += 1
                continue
            checked += 1
            rows = slice(img * b, (img + 1) * b)
            assert torch.equal(rec["after"]["tokens"][rows], st.tokens[rows]), (rec["step"], img)
            assert torch.allclose(rec["after"]["vals"][rows], st.vals[rows], rtol=0, atol=VAL_TOL * (rec["step"] + 1), equal_nan=True)
    print(f"{kind}: {checked} steps checked, {skipped} left out")
    assert checked + skipped == 4 * 8 and skipped <= 0.2 * (checked + skipped)
    rows = rows_of(beams.tokens[:, 0], beams.lengths[:, 0])
    assert all(boost in r for r in rows) and not any(boost in r for r in rows_of(*plain))


@pytest.mark.parametrize("search", ("sample", "beam"))
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_return_logprobs_are_taken_on_the_biased_rows(kind, search, images, monkeypatch):
    """``logprobs[i, slot, c]`` is ``log_softmax(biased row / T)`` at the token (fp64 on the engine's own biased rows, within the
    row sweep's fp32 error), and under ``search="beam"`` the left-to-right fp32 sum over a live beam's columns IS its score."""
    model, _, _ = build(kind)
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=8, beam_size=3, top_k=20, temperature=1.3, seed=2, search=search)
    bias, boost, _ = biting_bias(model, args, kw)
    steps = snapshots(monkeypatch)
    with torch.no_grad():
        beams, lp = model.generate_batch(*args, sequence_bias=bias, return_beams=True, return_logprobs=True, **kw)
    toks, lens, lp, scores = beams.tokens.cpu(), beams.lengths.cpu(), lp.cpu(), beams.scores.cpu()
    assert any(boost in toks[i, j, :int(lens[i, j])].tolist() for i in range(3) for j in range(3))
    # every recorded pick against the biased row it was taken from
    seen = 0
    for rec in steps:
        if rec["write_pos"] >= rec["before"]["tokens"].shape[1]:
            continue
        rows, mult = rec["biased"].shape[0], rec["beam"] if rec["first"] else 1
        want_x, _, _ = bias_logits(rec["logits"], rec["before"]["tokens"][::mult], rec["write_pos"], bias)
        assert torch.equal(bits(rec["biased"]), bits(want_x)), rec["step"]
        ref = torch.log_softmax(want_x.double() / 1.3, 1)
        live = ~rec["before"]["ended"][::mult][:rows].bool()
        idx, got = rec["pick_idx"][:rows].long().clamp(0, want_x.shape[1] - 1), rec["pick_lp"][:rows].double()
        assert bool((got[~live] == 0).all())
        assert torch.allclose(got[live], ref.gather(1, idx)[live], rtol=0, atol=VAL_TOL), rec["step"]
        seen += int(live.sum())
    assert seen > 0
    if search == "beam":
        for i in range(3):
            for j in range(3):
                n = int(lens[i, j])
                if scores[i, j] == NEG_INF or (kind == "CaptioningTransformer" and n < 8):
                    continue                                  # (a dead beam; an all-ended Transformer image drops its last <eos> column)
                acc = torch.zeros((), dtype=torch.float32)
                for c in range(n):
                    acc = acc + lp[i, j, c]
                assert torch.equal(bits(acc.view(1)), bits(scores[i, j].view(1))), (i, j)
    assert bool((lp <= VAL_TOL).all()) and bool((lp < -1.0).any())      # (a boosted token's log-probability is 0 within the sweep's error)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_default_route_equals_exact_and_the_boosted_token_is_there(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=12, beam_size=3, top_k=10, temperature=1.2, seed=5)
    bias, boost, plain = biting_bias(model, args, kw)
    with torch.no_grad():
        a = model.generate_batch(*args, sequence_bias=bias, **kw)
        b = model.generate_batch(*args, sequence_bias=bias, exact=True, **kw)
        d = model.generate_batch(*args, sequence_bias=dict(bias), **kw)           # (the mapping in the list's order)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], d[0])
    assert not torch.equal(a[0], plain[0])
    assert all(boost in r for r in rows_of(*a)) and not any(boost in r for r in rows_of(*plain))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_none_is_the_call_without_the_keyword(kind, images, monkeypatch):
    """Equal outputs and the same launches, counted at ``hip._launch``.  With a list, exactly one more launch per row draw, behind
    the history edits and in front of the bans."""
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
        for off in (None, {}, []):
            (d_t, d_l), d_names = run(streams=streams, sequence_bias=off)
            assert torch.equal(p_t, d_t) and torch.equal(p_l, d_l) and p_names == d_names and NAME not in d_names
        _, on = run(streams=streams, sequence_bias={(17,): 2.0, (230, 45): -1.0})
        draws = sum(n.startswith("dh_beam_row_sample") for n in p_names)
        assert draws > 0 and on.count(NAME) == draws and len(on) == len(p_names) + draws
        _, on = run(streams=streams, sequence_bias={(17,): 2.0}, no_repeat_ngram_size=2, bad_words_ids=[[5]])
        at = [i for i, n in enumerate(on) if n == NAME]
        assert len(at) == draws
        assert all(on[i - 1] == "dh_beam_history_logits" and on[i + 1] == "dh_beam_constrain_logits" and
                   on[i + 2].startswith("dh_beam_row_sample") for i in at)


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------
KW = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2, top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_top_p_repeat_controls_bans_prompts_batches_and_streams(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    bias, boost, nothing = biting_bias(model, args, dict(KW, seed=31))
    kw = dict(KW, sequence_bias=bias)
    with torch.no_grad():
        plain = model.generate_batch(*args, seed=31, **kw)
        assert not torch.equal(plain[0], nothing[0]) and all(boost in r for r in rows_of(*plain))
        for r in rows_of(*plain):                                             # (no_repeat_ngram_size=2 still holds: no bigram twice)
            grams = list(zip(r, r[1:]))
            assert len(grams) == len(set(grams)), r
        two = model.generate_batch(*args, seed=31, streams=2, **kw)
        assert torch.equal(two[0], plain[0]) and torch.equal(two[1], plain[1])
        for lo in (0, 2):                                                    # a batch equals its halves
            half = model.generate_batch(*model_args(kind, images, lo, lo + 2), seed=31, img0=lo, **kw)
            assert torch.equal(half[0], plain[0][lo:lo + 2]) and torch.equal(half[1], plain[1][lo:lo + 2]), lo
        ex = model.generate_batch(*args, seed=31, exact=True, **kw)
        assert torch.equal(ex[0], plain[0])
        # a banned and boosted token stays banned: -inf + b = -inf
        banned = model.generate_batch(*args, seed=31, bad_words_ids=[[boost]], **kw)
        assert not any(boost in r for r in rows_of(*banned))
        # prompts of their own length: each prompt ENDS in a phrase prefix (the history includes the prompt), and the batch equals
        # the dense single-image calls with those prompts
        cap = torch.tensor([[17, 230, 45], [8, 9, 8], [300, 301, 302], [40, 41, 40]]).cuda()
        lens = torch.tensor([0, 3, 1, 2])
        pbias = [((601,), 30.0), ((9, 8, 602), 30.0), ((300, 603), 30.0), ((40, 41, 604), 30.0), ((8, 8, 605), 30.0), ((301, 606), 30.0)]
        kwp = dict(kw, sequence_bias=pbias)
        before = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **dict(kw, sequence_bias=None))
        prompted = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **kwp)
        both = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, streams=2, **kwp)
        assert torch.equal(both[0], prompted[0]) and torch.equal(both[1], prompted[1]) and not torch.equal(prompted[0], before[0])
        for i, n in enumerate(lens.tolist()):
            row = prompted[0][i, :int(prompted[1][i])].tolist()
            assert row[:n] == cap[i, :n].tolist(), (i, row)
            one =model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, caption=cap[i:i + 1, :n] if n else None, **kwp)
            assert torch.equal(one[0], prompted[0][i:i + 1]) and torch.equal(one[1], prompted[1][i:i + 1]), (i, n)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay_beside_the_plain_graph(kind, images):
    from deephumor_amd.models.beam import SequenceBias
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2)
    bias, boost, _ = biting_bias(model, args, dict(kw, seed=3))
    other = [(w, -b) for w, b in bias]                                          # a second list of the same shape
    with torch.no_grad():
        for seed in (3, 4):
            on_g = model.generate_batch_graphed(*args, seed=seed, sequence_bias=bias, **kw)
            off_g = model.generate_batch_graphed(*args, seed=seed, **kw)
            none_g = model.generate_batch_graphed(*args, seed=seed, sequence_bias=None, **kw)
            on_e = model.generate_batch(*args, seed=seed, sequence_bias=bias, **kw)
            off_e = model.generate_batch(*args, seed=seed, **kw)
            assert torch.equal(on_g[0], on_e[0]) and torch.equal(on_g[1], on_e[1]), (kind, seed)
            assert torch.equal(off_g[0], off_e[0]) and torch.equal(off_g[1], off_e[1]) and torch.equal(none_g[0], off_e[0]), (kind, seed)
            assert not torch.equal(on_e[0], off_e[0]) and all(boost in r for r in rows_of(*on_g))
        assert len(model._graphs) == 2                           # the list is in the cache key: two graphs side by side, None the plain one
        keys = [dict(k[2]).get("sequence_bias") for k in model._graphs]
        assert sorted(k is None for k in keys) == [False, True] and all(k is None or isinstance(k, SequenceBias) for k in keys)
        o_g = model.generate_batch_graphed(*args, seed=3, sequence_bias=other, **kw)
        o_e = model.generate_batch(*args, seed=3, sequence_bias=other, **kw)
        assert torch.equal(o_g[0], o_e[0]) and torch.equal(o_g[1], o_e[1])
        assert len(model._graphs) == 3                           # its own graph
        again = model.generate_batch_graphed(*args, seed=3, sequence_bias=bias, **kw)       # the first list's graph is still the first list's
        assert torch.equal(again[0], model.generate_batch(*args, seed=3, sequence_bias=bias, **kw)[0])
        assert len(model._graphs) == 3


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_pipeline(kind, images):
    from deephumor_amd.models.beam import compile_sequence_bias
    from deephumor_amd.pipeline import CaptionPipeline
    model, _, _ = build(kind)
    model = model.bfloat16()
    batches = [(images[:2],), (images[2:],), (images[1:3],)]
    bias, boost, _ = biting_bias(model, (images.cuda(),), dict(KW, seed=40))
    kw = dict(KW, sequence_bias=bias)
    with torch.no_grad():
        want = [model.generate_batch(b[0].cuda(), seed=40 + i, **kw) for i, b in enumerate(batches)]
        off = model.generate_batch(batches[0][0].cuda(), seed=40, **dict(kw, sequence_bias=None))
    assert not torch.equal(want[0][0], off[0]) and all(boost in r for w in want for r in rows_of(*w))
    for given in (kw, dict(kw, sequence_bias=compile_sequence_bias(bias, 1000, "cuda"))):       # the raw list or a SequenceBias
        pipe = CaptionPipeline(model, **given)
        got = [tuple(t.clone() for t in r) for r in pipe.run(batches, seeds=[40, 41, 42])]
        for w, r in zip(want, got):
            assert torch.equal(w[0].cpu(), r[0].cpu()) and torch.equal(w[1].cpu(), r[1].cpu())
    pipe = CaptionPipeline(model, **dict(KW, sequence_bias=None))
    assert "sequence_bias" not in pipe.gen_kw
    for bad, exc in ((dict(sequence_bias={(5,): float("nan")}), ValueError), (dict(sequence_bias={(5,): True}), ValueError),
                     (dict(sequence_bias={(1000,): 1.0}), ValueError), (dict(sequence_bias=[[5]]), ValueError),
                     (dict(sequence_bias="word"), TypeError)):
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
base = dict(max_len=10, beam_size=3, top_k=20, seed=11, top_p=0.8)
with torch.no_grad():
    t0, l0 = model.generate_batch(images, img0=0, **base)
rows = [t0[i, :int(l0[i])].tolist() for i in range(4)]
held = set(t for r in rows for t in r)
boost = next(t for t in range(10, 1000) if t not in held)
kw = dict(base, sequence_bias=[((boost,), 60.0)] + [((r[0],), -8.0) for r in rows] + [(tuple(r[1:3]), 6.0) for r in rows])
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, img0=0, **kw)
    plain = model.generate_batch(images, img0=0, **dict(kw, sequence_bias=None))
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 2, always=True) for a in (0, 2)]
    got = tuple(torch.cat(ts, 0) for ts in zip(*halves))
    micro = generate_micro_sharded(fn, 4, 2, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want),
                              "differs": not same(plain, want),
                              "boosted": all(boost in want[0][i, :int(want[1][i])].tolist() for i in range(4))}))
dist.barrier()
dist.destroy_process_group()
"""


def test_batch_equals_sharded_halves_through_one_rank_rccl():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True, "differs": True, "boosted": True}
