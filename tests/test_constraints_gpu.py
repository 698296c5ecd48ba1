"""``min_len`` / ``bad_words_ids`` on a real MI355X: ``dh_beam_constrain_logits`` bit for bit against the torch-CPU restatement
(``tests/constraints_ref.py``) -- logits, every group maximum, every word it must not touch --, the repaired group maxima under the
group-guided sampler, ``generate_batch`` against golden G22 recorded from the reference, and the keywords through every layer that
carries them."""
import json
import os
import subprocess
import sys
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu

from constraints_ref import CASE_VS, EOS, NEG_INF, UNK, banned_phrase_in, constrain_logits, eos_below, flatten, kernel_cases  # noqa: E402
from helpers import KINDS, captions_and_lengths, golden, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G22_KW = dict(beam_size=3, top_k=50, temperature=1.3)
POISON_X, POISON_G = 555.0, 777.0
NAME = "dh_beam_constrain_logits"


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
def launch(hip, x, v, gm, ng, table, mult, pos, rows, rpi, first_pos, eos, min_len, words, offs, n_words):
    hip._launch(NAME, x.data_ptr(), x.stride(0), v, 0 if gm is None else gm.data_ptr(), 0 if gm is None else gm.stride(0), ng, 64,
                table.data_ptr(), table.stride(0), mult, pos, rows, rpi, 0 if first_pos is None else first_pos.data_ptr(), eos, min_len,
                0 if words is None else words.data_ptr(), 0 if offs is None else offs.data_ptr(), n_words,
                torch.cuda.current_stream().cuda_stream)


def run_case(hip, c, min_len, with_groups, phrases=None, rpi=1, first_pos=None, active=None):
    """One launch on a copy of the case: logits in a wider buffer (pad columns poisoned), group words pre-filled with a sentinel and
    one word more than there are groups.  Everything is compared with ``torch.equal``: the logits bit for bit, edited groups equal
    to the exact maximum, every other group word still the sentinel, the token table and the list untouched."""
    v, rows, mult, pos = c["v"], c["rows"], c["mult"], c["pos"]
    phrases = c["phrases"] if phrases is None else phrases
    ng = (v + 63) // 64                                   # V = 130: 3 groups, the last of 2 real columns
    x = torch.full((rows, v + 5), POISON_X)
    x[:, :v] = c["logits"]
    gm0 = torch.full((rows, ng + 1), POISON_G)
    words, offs = flatten(phrases) if phrases else (None, None)
    dx, dt = x.cuda(), c["table"].cuda()
    dw, do = (words.cuda(), offs.cuda()) if phrases else (None, None)
    dg = gm0.cuda() if with_groups else None
    launch(hip, dx, v, dg, ng, dt, mult, pos, rows, rpi, first_pos, c["eos"], min_len, dw, do, len(phrases))
    want_x, want_g, stored = constrain_logits(c["logits"], c["table"][::mult], pos, phrases, min_len, c["eos"],
                                              gm0 if with_groups else None, 64, active=active)
    got = dx.cpu()
    tag = (v, rows, mult, pos, min_len, with_groups)
    assert torch.equal(got[:, :v], want_x), tag
    assert bool((got[:, v:] == POISON_X).all()), tag
    assert torch.equal(dt.cpu(), c["table"])
    if phrases:
        assert torch.equal(dw.cpu(), words) and torch.equal(do.cpu(), offs)
    if with_groups:
        got_g = dg.cpu()
        assert torch.equal(got_g, want_g), tag
        touched = torch.zeros((rows, ng + 1), dtype=torch.bool)
        touched[:, :ng] = torch.nn.functional.pad(stored.to(torch.uint8), (0, ng * 64 - v)).view(rows, ng, 64).any(-1)
        assert bool((got_g[~touched] == POISON_G).all()), tag                 # every other word is still the sentinel
        exact = torch.nn.functional.pad(want_x, (0, ng * 64 - v), value=NEG_INF).view(rows, ng, 64).max(-1).values
        assert torch.equal(got_g[:, :ng][touched[:, :ng]], exact[touched[:, :ng]]), tag
    return want_x, want_g, stored


@pytest.mark.parametrize("v", CASE_VS)
def test_kernel_is_bit_exact(hip, v):
    """The cases of ``constraints_ref.kernel_cases``: 12 rows at ``pos`` 0 / 1 / 5 / 40 and the dense first step (4 rows,
    ``tok_row_mult = 3``), 300 phrases each, ``min_len`` above ``pos`` and at-or-below it, with and without a group table -- and the
    same rows with an empty list (the ``<eos>`` ban alone)."""
    cases = kernel_cases(v)
    assert len(cases) == 5
    for c in cases:
        for min_len in c["min_lens"]:
            for with_groups in (False, True):
                want_x, want_g, stored = run_case(hip, c, min_len, with_groups)
            assert bool((want_x[:, c["eos"]] == NEG_INF).all()) == (c["pos"] < min_len)      # (no phrase of the cases ends in <eos>)
            assert bool((want_g[:, 1] == NEG_INF).all())                                      # group 1: every column banned
        _, want_g, stored = run_case(hip, c, c["pos"] + 1, True, phrases=[])
        assert stored.sum(1).tolist() == [1] * c["rows"] and bool((want_g[:, 0] < POISON_G).all())


def test_kernel_prompted_phases(hip):
    """``first_pos`` at position 5: image 0 forced (5 < 7), image 1 at its first draw (its base row alone is active), image 2
    running, image 3 forced.  Idle rows keep every word, logits and group maxima."""
    c = kernel_cases(1000)[2]
    assert c["pos"] == 5 and c["rows"] == 12
    fp = torch.tensor([7, 5, 2, 6], dtype=torch.int32, device="cuda")
    active = torch.tensor([False] * 3 + [True, False, False] + [True] * 3 + [False] * 3)
    for min_len in (7, 0):
        _, _, stored = run_case(hip, c, min_len, True, rpi=3, first_pos=fp, active=active)
        assert not stored[:3].any() and not stored[4:6].any() and not stored[9:].any()
        assert stored[3].any() and stored[6:9].any(1).all()


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
def test_groups_sampler_on_the_repaired_maxima_equals_the_exact_sampler(hip, kind, planes):
    """The logits and group maxima of the real classifiers, one small model each (``dh_vocab_logits`` on the bf16 operands of the
    LSTM model's classifier, ``dh_linear_f32xp`` on the split fp32 planes of the Transformer's; V = 1000), banned through the public
    binding, then drawn by ``dh_beam_row_sample_groups`` -- which trusts the maxima -- and by the exact sampler -- which reads the
    whole row -- with the same Philox key: the same picks.  Every row's OWN top 8 tokens are banned (row ``r``'s history ends in a
    marker ``900 + r``, the phrases are ``[900 + r, token]``), so the maxima of the groups that bound the top-k must FALL; a stale
    table would let the groups sampler stop at groups whose maximum is gone."""
    from deephumor_amd import f32xp
    from deephumor_amd.models.beam import compile_bad_words
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
    pos = 4
    table = torch.randint(0, 800, (rows, pos + 2), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    table[:, pos - 1] = 900 + torch.arange(rows, dtype=torch.int32)
    phrases = [[900 + r, int(t)] for r in range(rows) for t in order[r, :8]]
    for name, plist, min_len in (("the rows' own top 8", phrases, 0), ("and <eos> below min_len", phrases, pos + 1),
                                 ("the top 3 of row 0, everywhere", [[int(t)] for t in order[0, :3]], 0)):
        bw = compile_bad_words(plist, v, "cuda")
        x, gm = raw.clone(), gm_raw.clone()
        hip.beam_constrain_logits(x, v, table.cuda(), 1, pos, rows, beam, EOS, min_len, bw.words, bw.offsets, len(bw), group_max=gm)
        want_x, want_g, stored = constrain_logits(raw.cpu(), table, pos, plist, min_len, EOS, gm_raw.cpu(), 64)
        assert torch.equal(x.cpu(), want_x) and torch.equal(gm.cpu(), want_g), name
        if plist is phrases:
            assert stored.sum(1).min() >= 8 and bool(stored[torch.arange(rows)[:, None], order[:, :8]].all())
            assert not bool(stored[0, order[1, :8]].all())                      # the bans are the row's own
            assert int((want_g < gm_raw.cpu()).sum()) >= rows, name           # maxima FELL: a stale table would be wrong
        gi, gv, gerr = sample(hip, "groups", x, v, gm, rows, beam, top_k, step=pos)
        ei, ev, eerr = sample(hip, "exact", x, v, None, rows, beam, top_k, step=pos)
        assert gerr == eerr == 0 and gi.tolist() == ei.tolist() and torch.equal(gv, ev), name
        for r in range(rows):                                                   # and no row drew a token banned for it
            assert not bool(stored[r, gi[r].long()].any()), (name, r)


# ---- 3. model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0)


def model_args(kind, images, lo, hi):
    _, _, labels = captions_and_lengths()
    return (images[lo:hi].cuda(), labels[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


def g22_phrases(g, slot):
    words, offs = g[f"words_{slot}"].tolist(), g[f"offsets_{slot}"].tolist()
    return [words[a:b] for a, b in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize("kind", KINDS)
def test_sampled_caption_matches_the_reference(kind, images):
    """fp32, ``rng="torch"``: every G22 slot, token for token (the recorder kept only captions that 8 relative perturbations of 1e-4
    of the reference's logits do not move).  Slots 2 and 3 use an ``eos_index`` the model draws, so that ``min_len`` bites."""
    g = golden(f"g22_constraints_{kind}.npz")
    model, _, _ = build(kind)
    kw = dict(G22_KW, max_len=int(g["max_len"]))
    for i in range(int(g["n_slots"])):
        ctl = dict(min_len=int(g[f"min_len_{i}"]), bad_words_ids=g22_phrases(g, i), eos_index=int(g[f"eos_{i}"]))
        img, seed = int(g[f"image_{i}"]), int(g[f"seed_{i}"])
        with torch.no_grad():
            toks, lens = model.generate_batch(*model_args(kind, images, img, img + 1), seed=seed, rng="torch", **ctl, **kw)
            assert toks[0, :int(lens[0])].cpu().tolist() == g[f"out_{i}"].tolist(), (kind, i)
            torch.manual_seed(seed)
            one = model.generate(*model_args(kind, images, img, img + 1), rng="torch", **ctl, **kw)
            assert one.cpu().tolist() == g[f"out_{i}"].tolist()


def frequent_token(rows, lo, hi):
    """The most frequent token at columns ``lo .. hi - 1`` of the beam rows (a list of lists): made ``eos_index``, it ends captions
    early, which the synthetic models' ``<eos>`` (one token of 1,000, hardly ever among the top-k) does not."""
    return Counter(t for r in rows for t in r[lo:hi]).most_common(1)[0][0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_no_beam_holds_a_banned_phrase_or_an_early_eos(kind, dtype, images):
    """``return_beams=True``, every row scanned on the host at its own length.  The controls are taken from the call without
    them, so that they bite: ``eos_index`` is a token that call draws often in columns 1 .. 4 (it ends beams below ``min_len`` =
    8), the list holds every image's first drawn token as a single and a bigram and a trigram of every image's drawn beam."""
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=12, beam_size=3, top_k=10, temperature=0.7, seed=3, return_beams=True)
    with torch.no_grad():
        first = model.generate_batch(*args, **kw)
        eos = frequent_token([first.tokens[i, j].tolist() for i in range(4) for j in range(3)], 1, 5)
        kw["eos_index"], min_len = eos, 8
        plain = model.generate_batch(*args, **kw)
        rows = [[plain.tokens[i, j, :int(plain.lengths[i, j])].tolist() for j in range(3)] for i in range(4)]
        assert any(eos_below(r, min_len, eos) for im in rows for r in im)                       # the plain call does end early
        drawn = [rows[i][int(plain.drawn[i])] for i in range(4)]
        phrases = [[r[0]] for r in drawn] + [r[1:3] for r in drawn if len(r) >= 3] + [r[2:5] for r in drawn if len(r) >= 5]
        assert any(len(w) == 2 for w in phrases) and all(banned_phrase_in(r, phrases) for r in drawn)
        beams = model.generate_batch(*args, min_len=min_len, bad_words_ids=phrases, **kw)
    toks, blen = beams.tokens.cpu(), beams.lengths.cpu()
    for i in range(4):
        for j in range(3):
            row = toks[i, j, :int(blen[i, j])].tolist()
            assert banned_phrase_in(row, phrases) is None, (kind, i, j, row)
            assert not eos_below(row, min_len, eos), (kind, i, j, row)
            assert int(blen[i, j]) > min_len or eos not in row
    assert not torch.equal(beams.tokens, plain.tokens)


def biting_controls(model, args, kw):
    """``(controls, plain result)``: ``eos_index`` = a token the plain call draws early, ``min_len`` 6, the first token and a bigram of
    every plain caption banned."""
    with torch.no_grad():
        t0, l0 = model.generate_batch(*args, **kw)
        eos = frequent_token([t0[i, :int(l0[i])].tolist() for i in range(t0.shape[0])], 1, 5)
        rows = [t0[i, :int(l0[i])].tolist() for i in range(t0.shape[0])]
    phrases = [[r[0]] for r in rows] + [r[1:3] for r in rows if len(r) >= 3]
    return dict(eos_index=eos, min_len=6, bad_words_ids=phrases), (t0, l0)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_default_route_equals_exact(kind, images):
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 4)
    kw = dict(max_len=12, beam_size=3, top_k=10, temperature=1.2, seed=5)
    ctl, plain = biting_controls(model, args, kw)
    with torch.no_grad():
        a, b = model.generate_batch(*args, **ctl, **kw), model.generate_batch(*args, exact=True, **ctl, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], plain[0])                           # the controls are not a no-op here


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_defaults_are_the_call_without_the_keywords(kind, images, monkeypatch):
    """Equal outputs and the same launches, counted at ``hip._launch``.  With a list, exactly one more launch per row draw; with
    ``min_len = 3`` alone, one more per row draw at positions 0, 1, 2 and none after."""
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
        (d_t, d_l), d_names = run(streams=streams, min_len=0, bad_words_ids=None)
        assert torch.equal(p_t, d_t) and torch.equal(p_l, d_l) and p_names == d_names
        (e_t, e_l), e_names = run(streams=streams, bad_words_ids=[])
        assert torch.equal(p_t, e_t) and e_names == p_names and NAME not in d_names
        _, on = run(streams=streams, bad_words_ids=[[17], [230, 45]])
        draws = sum(n.startswith("dh_beam_row_sample") for n in p_names)
        assert draws > 0 and on.count(NAME) == draws and len(on) == len(p_names) + draws
        _, on = run(streams=streams, min_len=3)
        assert on.count(NAME) == 3 * streams and len(on) == len(p_names) + 3 * streams
        _, on = run(streams=streams, min_len=3, no_repeat_ngram_size=2)           # behind the history edits, in front of the draw
        at = [i for i, n in enumerate(on) if n == NAME]
        assert len(at) == 3 * streams
        assert all(on[i - 1] == "dh_beam_history_logits" and on[i + 1].startswith("dh_beam_row_sample") for i in at)


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------
KW = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2, top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_top_p_repeat_controls_prompts_batches_and_streams(kind, dtype, images):
    model, _, _ = build(kind)
    model = model.to(dtype)
    args = model_args(kind, images, 0, 4)
    ctl, nothing = biting_controls(model, args, dict(KW, seed=31))
    kw = dict(KW, **ctl)
    with torch.no_grad():
        plain = model.generate_batch(*args, seed=31, **kw)
        assert not torch.equal(plain[0], nothing[0])
        for i in range(4):
            row = plain[0][i, :int(plain[1][i])].tolist()
            assert banned_phrase_in(row, ctl["bad_words_ids"]) is None and not eos_below(row, 6, ctl["eos_index"])
        two = model.generate_batch(*args, seed=31, streams=2, **kw)
        assert torch.equal(two[0], plain[0]) and torch.equal(two[1], plain[1])
        for lo in (0, 2):                                                    # a batch equals its halves
            half = model.generate_batch(*model_args(kind, images, lo, lo + 2), seed=31, img0=lo, **kw)
            assert torch.equal(half[0], plain[0][lo:lo + 2]) and torch.equal(half[1], plain[1][lo:lo + 2]), lo
        ex = model.generate_batch(*args, seed=31, exact=True, **kw)
        assert torch.equal(ex[0], plain[0])
        # prompts of their own length; the phrases are taken from the prompted call without a list, so that each prompt ENDS in a
        # phrase prefix and the first generated token is the one that is banned
        cap = torch.tensor([[17, 230, 45], [8, 9, 8], [300, 301, 302], [40, 41, 40]]).cuda()
        lens = torch.tensor([0, 3, 1, 2])
        kw0 = dict(kw, bad_words_ids=None)
        before = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **kw0)
        firsts = [int(before[0][i, n]) for i, n in enumerate(lens.tolist())]
        phrases = [[firsts[0]], [9, 8, firsts[1]], [300, firsts[2]], [40, 41, firsts[3]], [8, 8, (firsts[1] + 1) % 1000]]
        kwp = dict(kw, bad_words_ids=phrases)
        prompted = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, **kwp)
        both = model.generate_batch(*args, seed=31, caption=cap, caption_lengths=lens, streams=2, **kwp)
        assert torch.equal(both[0], prompted[0]) and torch.equal(both[1], prompted[1])
        for i, n in enumerate(lens.tolist()):
            row = prompted[0][i, :int(prompted[1][i])].tolist()
            assert row[:n] == cap[i, :n].tolist() and row[n] != firsts[i], (i, row)
            assert banned_phrase_in(row, phrases, start=n) is None and not eos_below(row, 6, ctl["eos_index"], start=n)
            one = model.generate_batch(*model_args(kind, images, i, i + 1), seed=31, img0=i, caption=cap[i:i + 1, :n] if n else None, **kwp)
            assert torch.equal(one[0], prompted[0][i:i + 1]) and torch.equal(one[1], prompted[1][i:i + 1]), (i, n)


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay_beside_the_plain_graph(kind, images):
    from deephumor_amd.models.beam import BadWords
    model, _, _ = build(kind)
    model = model.bfloat16()
    args = model_args(kind, images, 0, 3)
    kw = dict(max_len=10, beam_size=3, top_k=20, temperature=1.2)
    ctl, _ = biting_controls(model, args, dict(kw, seed=3))
    other = dict(ctl, bad_words_ids=[[t + 1 for t in w] for w in ctl["bad_words_ids"]])      # a second list of the same shape
    with torch.no_grad():
        for seed in (3, 4):
            on_g = model.generate_batch_graphed(*args, seed=seed, **ctl, **kw)
            off_g = model.generate_batch_graphed(*args, seed=seed, eos_index=ctl["eos_index"], **kw)
            on_e = model.generate_batch(*args, seed=seed, **ctl, **kw)
            off_e = model.generate_batch(*args, seed=seed, eos_index=ctl["eos_index"], **kw)
            assert torch.equal(on_g[0], on_e[0]) and torch.equal(on_g[1], on_e[1]), (kind, seed)
            assert torch.equal(off_g[0], off_e[0]) and torch.equal(off_g[1], off_e[1]), (kind, seed)
            assert not torch.equal(on_e[0], off_e[0])
        assert len(model._graphs) == 2                           # the list is in the cache key: two graphs side by side
        keys = [dict(k[2]).get("bad_words_ids") for k in model._graphs]
        assert sorted(k is None for k in keys) == [False, True] and all(k is None or isinstance(k, BadWords) for k in keys)
        o_g = model.generate_batch_graphed(*args, seed=3, **other, **kw)
        o_e = model.generate_batch(*args, seed=3, **other, **kw)
        assert torch.equal(o_g[0], o_e[0]) and torch.equal(o_g[1], o_e[1])
        assert len(model._graphs) == 3                           # its own graph
        again = model.generate_batch_graphed(*args, seed=3, **ctl, **kw)           # the first list's graph is still the first list's
        want = model.generate_batch(*args, seed=3, **ctl, **kw)
        assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1]) and len(model._graphs) == 3


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_pipeline(kind, images):
    from deephumor_amd.models.beam import compile_bad_words
    from deephumor_amd.pipeline import CaptionPipeline
    model, _, _ = build(kind)
    model = model.bfloat16()
    batches = [(images[:2],), (images[2:],), (images[1:3],)]
    ctl, _ = biting_controls(model, (images.cuda(),), dict(KW, seed=40))
    kw = dict(KW, **ctl)
    with torch.no_grad():
        want = [model.generate_batch(b[0].cuda(), seed=40 + i, **kw) for i, b in enumerate(batches)]
        off = model.generate_batch(batches[0][0].cuda(), seed=40, **dict(kw, min_len=0, bad_words_ids=None))
    assert not torch.equal(want[0][0], off[0])
    for given in (kw, dict(kw, bad_words_ids=compile_bad_words(ctl["bad_words_ids"], 1000, "cuda"))):       # raw nesting or BadWords
        pipe = CaptionPipeline(model, **given)
        got = [tuple(t.clone() for t in r) for r in pipe.run(batches, seeds=[40, 41, 42])]
        for w, r in zip(want, got):
            assert torch.equal(w[0].cpu(), r[0].cpu()) and torch.equal(w[1].cpu(), r[1].cpu())
    for bad, exc in ((dict(min_len=-1), ValueError), (dict(min_len=True), ValueError), (dict(min_len=2.0), TypeError),
                     (dict(min_len=10, max_len=10), ValueError), (dict(min_len=25), ValueError), (dict(bad_words_ids=[[]]), ValueError),
                     (dict(bad_words_ids=[[1000]]), ValueError), (dict(bad_words_ids="word"), TypeError)):
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
eos = max(set(t for r in rows for t in r[1:5]), key=[t for r in rows for t in r[1:5]].count)
kw = dict(base, eos_index=eos, min_len=6, bad_words_ids=[[r[0]] for r in rows] + [r[1:3] for r in rows])
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, img0=0, **kw)
    plain = model.generate_batch(images, img0=0, **dict(kw, min_len=0, bad_words_ids=None))
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
