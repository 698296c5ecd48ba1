"""``generate_batch(..., return_logprobs=True)`` on a real MI355X.

Kernel level: ``dh_beam_pick_logprobs`` against fp64 (``logprobs_ref.pick_logprobs``) within ``VAL_TOL`` -- the project's bound for
``dh_beam_row_best``'s sweep, whose arithmetic it restates --, bit-identical runs, the ``from_vals`` copy and the prompted phases;
``dh_beam_record_logprobs`` / ``dh_beam_gather_logprobs`` bit for bit against ``logprobs_ref.record`` / ``gather`` on random tables.

Model level, every kind: the returned ``[N, B, T]`` against ``logprobs_ref.track`` on the engine's own snapshots (the fp32 logits
the row step saw are the input in every storage type, so ``VAL_TOL`` holds for all three); under ``search="beam"`` the sequential
fp32 sum of a beam's own columns IS its score, bit for bit; the values against the teacher-forced ``forward``; bitwise
self-consistency of everything the keyword composes with; graph replay; the default's launch sequence; the refusals.

``FORWARD_GATE``: measured on an MI355X, not set in advance -- 1.25 x the worst difference ``test_values_are_the_teacher_forced_forward``
prints over the five kinds (fp32, no edits, temperature 1), see DESIGN.md section 5.  The contract's fp32 logit parity between the
incremental decode and ``forward`` is 1e-3; twice that (a token's logit and the row's normaliser) is the ceiling it must stay below."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import logprobs_ref as R  # noqa: E402
from helpers import KINDS, captions_and_lengths, synthetic_sd, synth_images  # noqa: E402

VAL_TOL = 2e-5              # tests/test_beam_search_gpu.py's bound for the same sweep: fp32 expf + a tree sum over 36 k terms + ulp(32)
FORWARD_WORST = 8.125e-07   # CaptioningLSTM; the other kinds 5.7e-07 .. 7.3e-07 (what the test below prints)
FORWARD_GATE = None if FORWARD_WORST is None else 1.25 * FORWARD_WORST
NINF, NAN, INF = float("-inf"), float("nan"), float("inf")
N_IMG, BEAM, MAX_LEN = 4, 3, 8
KW = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20, temperature=1.1, seed=5)
CROSS = ("CaptioningTransformer", "CaptioningTransformerWithLabels")


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


# ---- 1. dh_beam_pick_logprobs ------------------------------------------------------------------------------------------------------
ROWS = 8
ENDED_ROW = 5


def make_rows(v, beam):
    """Eight rows, |x| <= 30: random; half the columns ``-inf``; a constant row; one nearly one-hot; row 5 is the ended one; and random
    picks, ``-inf`` columns among them."""
    g = torch.Generator().manual_seed(1000 * v + beam)
    x = (torch.randn(ROWS, v, generator=g) * 2.5).clamp_(-30.0, 30.0)
    x[2, torch.rand(v, generator=g) < 0.5] = NINF
    x[2, 0] = 1.0
    x[4] = 0.75
    x[6] = -30.0
    x[6, v - 1] = 30.0
    x[7] = (x[7] * 8).clamp(-30.0, 30.0)
    picks = torch.stack([torch.randperm(v, generator=g)[:beam] for _ in range(ROWS)]).int()
    gone = (x[2] == NINF).nonzero().flatten()
    if len(gone):
        picks[2, 0] = int(gone[0])                                    # a pick that the edits have banned: -inf, not NaN
    return x, picks


def run_pick(h, x, picks, beam, temp, rpi, pad=0, first_pos=None, step=0, vals=None):
    rows, v = x.shape
    buf = torch.full((rows, v + pad), 1e30)
    if pad:
        buf[:, v::2], buf[:, v + 1::2] = NAN, INF
    buf[:, :v] = x
    dev = buf.cuda()[:, :v]
    ended = torch.zeros(rows * (beam if rpi == 1 else 1), dtype=torch.uint8)
    ended[ENDED_ROW * (beam if rpi == 1 else 1)] = 1
    out = torch.full((rows * beam + 64,), NAN, device="cuda")
    h.beam_pick_logprobs(None if vals is not None else dev, v, rows, rpi, beam, temp, step, ended.cuda(), picks.cuda(),
                         None if vals is None else vals.cuda(), out, from_vals=vals is not None, first_pos=first_pos)
    torch.cuda.synchronize()
    assert bool(out[rows * beam:].isnan().all())
    return out[:rows * beam].view(rows, beam).cpu()


def worst_diff(got, want):
    """``-inf`` exactly where the restatement has it; the largest difference elsewhere."""
    dead = want == NINF
    assert torch.equal(got == NINF, dead) and not bool(got.isnan().any())
    diff = (got.double() - want)[~dead].abs()
    return float(diff.max()) if diff.numel() else 0.0


PICK_CASES = [(v, b) for v in (2, 71, 1000, 36541) for b in (1, 3, 5, 64) if b <= v - 1]


@pytest.mark.parametrize("temp", (1.0, 1.3))
@pytest.mark.parametrize("v,beam", PICK_CASES)
def test_pick_logprobs_against_fp64(hip, v, beam, temp):
    x, picks = make_rows(v, beam)
    assert float((x[torch.isfinite(x)] / temp).abs().max()) <= 32.0
    ended = torch.zeros(ROWS, dtype=torch.bool)
    ended[ENDED_ROW] = True
    want = R.pick_logprobs(x, picks, ended, temp)
    dead = want == NINF
    assert bool((want[ENDED_ROW] == 0).all()) and not bool(want.isnan().any()) and (v < 71 or bool(dead[2, 0]))
    worst = 0.0
    for pad in (0, 3):                                                # 16-byte aligned rows (V + pad a multiple of 4 or not) and rows that are not
        runs = []
        for rpi in (1, beam, 1):
            got = run_pick(hip, x, picks, beam, temp, rpi, pad=pad)
            assert bool((got[ENDED_ROW] == 0).all())
            worst = max(worst, worst_diff(got, want))
            runs.append(got)
        for got in runs[1:]:                                          # a second run, and the other row mapping: the same bits
            assert torch.equal(got.view(torch.int32), runs[0].view(torch.int32)), pad
    print(f"V={v} beam={beam} T={temp}: max |pick_lp - fp64| = {worst:.3e}")
    assert worst <= VAL_TOL
    if v >= 71:                                                       # the constant row: -log(V), exactly the same value for every pick
        assert float((runs[0][4].double() + np.log(v)).abs().max()) <= VAL_TOL and len(set(runs[0][4].tolist())) == 1


@pytest.mark.parametrize("v,beam", [(71, 3), (36541, 64)])
def test_pick_logprobs_from_vals_is_a_masked_bit_copy(hip, v, beam):
    x, picks = make_rows(v, beam)
    g = torch.Generator().manual_seed(v)
    vals = torch.randn(ROWS, beam, generator=g) * 7
    vals[0, 0], vals[1, beam - 1] = NINF, -0.0
    for rpi in (1, beam):
        got = run_pick(hip, x, picks, beam, 1.3, rpi, vals=vals)
        want = vals.clone()
        want[ENDED_ROW] = 0.0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rpi


def test_pick_logprobs_prompted_phases_and_bad_rows(hip):
    """``first_pos``: a forced image's rows and all but the base row of an image at its first step are not written; a row with NaN or
    ``+inf``, a row of ``-inf`` only and a pick outside ``[0, V)`` give zeros, never NaN."""
    v, beam = 71, 4
    x, picks = make_rows(v, beam)                                     # 8 rows = 2 images x 4 beams
    ended = torch.zeros(ROWS, dtype=torch.bool)
    ended[ENDED_ROW] = True
    want = R.pick_logprobs(x, picks, ended, 1.0)
    for step, written in ((1, [4]), (2, [0, 4, 5, 6, 7]), (3, list(range(8))), (0, [])):
        got = run_pick(hip, x, picks, beam, 1.0, beam, first_pos=torch.tensor([2, 1], dtype=torch.int32).cuda(), step=step)
        rows = ~got.isnan().any(1)
        assert rows.nonzero().flatten().tolist() == written and bool(got[~rows].isnan().all()), step
        assert worst_diff(got[rows], want[rows]) <= VAL_TOL
    x[0, 5], x[1, 6], x[3] = NAN, INF, NINF
    picks[7, 0], picks[7, 1] = -1, v
    got = run_pick(hip, x, picks, beam, 1.0, beam)
    assert not bool(got.isnan().any()) and bool((got[[0, 1, 3]] == 0).all()) and got[7, :2].tolist() == [0.0, 0.0]
    assert float((got[7, 2:].double() - want[7, 2:]).abs().max()) <= VAL_TOL


# ---- 2. dh_beam_record_logprobs / dh_beam_gather_logprobs --------------------------------------------------------------------------
@pytest.mark.parametrize("prompted", (False, True), ids=("dense", "prompted"))
@pytest.mark.parametrize("width", (1, 7))
@pytest.mark.parametrize("beam", (1, 5, 64))
@pytest.mark.parametrize("n", (1, 3))
def test_record_and_gather_are_bit_exact(hip, n, beam, width, prompted):
    """Random tables, one step per slab and a last one that writes no column: the slab tables after every launch and the gathered
    ``[n, beam, width]`` equal the restatement's bit for bit; images that are done, forced or at their first step included."""
    g = torch.Generator().manual_seed(7 * n + beam + 100 * width + prompted)
    rows, n_pos = n * beam, width + 1
    first_pos = torch.randint(0, width + 1, (n,), generator=g).int() if prompted else None
    if prompted:
        first_pos[-1] = width                                         # an image forced to the end of the table ...
        first_pos[0] = 0 if n > 1 else min(2, width)                  # ... and one that draws from column 0
    lp_w, par_w = R.new_tables(n_pos, rows, torch.float32)
    d_lp, d_par = lp_w.cuda(), par_w.cuda()
    for s in range(n_pos):
        wp = s
        tokens = torch.randint(0, 2 * beam + 1, (rows, width), generator=g).int()
        base = (torch.arange(rows) // beam) * beam
        parent = (base + torch.randint(0, beam, (rows,), generator=g)).int()
        done = (torch.rand(n, generator=g) < 0.4).to(torch.uint8)
        end_step = torch.randint(max(s - 1, 0), s + 2, (n,), generator=g).int()
        pick_idx = torch.randint(0, 2 * beam + 1, (rows, beam), generator=g).int()
        pick_lp = -torch.rand(rows, beam, generator=g) * 9
        first = s == 0 and not prompted
        R.record(lp_w, par_w, s, tokens, parent, done, end_step, pick_idx, pick_lp, beam, first, wp, first_pos)
        hip.beam_record_logprobs(tokens.cuda(), parent.cuda(), done.cuda(), end_step.cuda(), pick_idx.cuda(), pick_lp.cuda(), n, beam, first,
                                 wp, s, d_lp, d_par, first_pos=None if first_pos is None else first_pos.cuda())
        assert torch.equal(d_par.cpu(), par_w) and torch.equal(d_lp.cpu().view(torch.int32), lp_w.view(torch.int32)), s
    assert bool((lp_w[width] == 0).all())                             # the step behind the table wrote parents only
    index = torch.stack([torch.randperm(beam, generator=g) for _ in range(n)]).int()
    lengths = torch.randint(0, width + 1, (n, beam), generator=g).int()
    lengths[0, 0] = width
    pos = 0 if prompted else int(torch.randint(0, width, (), generator=g))
    out = torch.full((rows * width + 64,), NAN, device="cuda")
    view = out[:rows * width].view(n, beam, width)
    hip.beam_gather_logprobs(d_lp, d_par, index.cuda(), lengths.cuda(), view, pos=pos, first_pos=None if first_pos is None else first_pos.cuda())
    want = R.gather(lp_w, par_w, index, lengths, width, pos, first_pos)
    assert torch.equal(view.cpu().view(torch.int32), want.view(torch.int32)) and bool(out[rows * width:].isnan().all())
    assert n == 1 or width == 1 or beam == 1 or bool((want != 0).any())


# ---- 3. models ---------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def build(kind, dt=torch.float32, **hp_over):
    key = (kind, dt, tuple(sorted(hp_over.items())))
    if key not in _MODELS:
        import deephumor_amd.models as M
        sd, hp = synthetic_sd(kind)
        model = getattr(M, kind)(**dict(hp, **hp_over)).eval()
        model.load_state_dict(sd)
        _MODELS[key] = model.to(dt).cuda()
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def drop_models():
    yield
    _MODELS.clear()


@pytest.fixture(scope="module")
def images():
    return synth_images(N_IMG, seed=0).cuda()


def labels():
    return captions_and_lengths()[2]


def model_args(kind, images, lo=0, hi=N_IMG):
    return (images[lo:hi], labels()[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi],)


def gen(model, args, **kw):
    with torch.no_grad():
        return model.generate_batch(*args, **kw)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def snapshots(monkeypatch):
    """Every beam step and the final step of the calls made from now on, as ``tests/test_beam_search_gpu.py`` takes them -- with the
    parents, and with the logits as they stand BEHIND the step's in-place edits and bans (the samplers write nothing into them)."""
    from deephumor_amd.models.beam import BeamSearchHelper
    steps, finals = [], []
    real_step, real_final = BeamSearchHelper._draw_and_select, BeamSearchHelper.finalize
    c = lambda t: None if t is None else t.detach().cpu().clone()

    def state_of(h):
        return dict(tokens=c(h.tokens), ended=c(h._ended), done=c(h.done), end_step=c(h.end_step), parent=c(h.parent))

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        rec = dict(first=first, write_pos=write_pos, step=step_index, before=state_of(self), temperature=self.temperature, beam=self.beam_size,
                   first_pos=None if self.first_pos is None or not prompted else self.first_pos.cpu().tolist(),
                   skipped=self.search == "beam" and write_pos >= self.tokens.shape[1])
        real_step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted)
        rec["logits"], rec["after"] = c(logits.float()), state_of(self)
        steps.append(rec)

    def final(self, len_bias_done, full_len, pad_index=0, **kw):
        finals.append(dict(pos=kw.get("pos", 0), first_pos=None if self.first_pos is None else self.first_pos.cpu().tolist(), width=self.max_len))
        return real_final(self, len_bias_done, full_len, pad_index, **kw)
    monkeypatch.setattr(BeamSearchHelper, "_draw_and_select", step)
    monkeypatch.setattr(BeamSearchHelper, "finalize", final)
    return steps, finals


PREFIX = torch.tensor([[17, 230, 45]])
PROMPT_LENS = [0, 2, 5, 3]
VARIANTS = {
    "dense with a prefix": lambda: dict(caption=PREFIX.repeat(N_IMG, 1).cuda()),
    "prompted": lambda: dict(caption=captions_and_lengths()[0][:N_IMG, :5].cuda(), caption_lengths=torch.tensor(PROMPT_LENS)),
    "edits and bans": lambda: dict(no_repeat_ngram_size=2, bad_words_ids=[[17], [230, 45], [8]]),
    "nucleus": lambda: dict(top_p=0.9),
}


def tracked(model, kind, images, monkeypatch, **extra):
    """One call with both keywords on the snapshot harness -> (beams, logprobs on the CPU, ``track``'s fp64 statement, first columns)."""
    steps, finals = snapshots(monkeypatch)
    beams, lp = gen(model, model_args(kind, images), return_beams=True, return_logprobs=True, **extra)
    monkeypatch.undo()
    assert len(finals) == 1 and steps
    final = dict(finals[0], beam_index=beams.beam_index.cpu(), lengths=beams.lengths.cpu())
    first = final["first_pos"] if final["first_pos"] is not None else [final["pos"]] * N_IMG
    return beams, lp.cpu(), R.track(steps, final), torch.tensor(first)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_on_the_engines_own_snapshots(hip, kind, dtype, images, monkeypatch):
    model = build(kind, dtype)
    for name, extra in VARIANTS.items():
        beams, lp, want, first = tracked(model, kind, images, monkeypatch, **KW, **extra())
        assert lp.shape == (N_IMG, BEAM, MAX_LEN) and lp.dtype == torch.float32 and want.shape == lp.shape
        assert bool(torch.isfinite(beams.scores).all()), name          # no beam of these inputs is dead: nothing is left out
        cols = torch.arange(MAX_LEN)[None, None, :]
        own = (cols >= first[:, None, None]) & (cols < beams.lengths.cpu()[:, :, None])
        assert bool((lp[~own] == 0).all()) and bool(own.any(-1).all()), name
        assert bool(torch.isfinite(lp).all()) and bool((lp[own] < 0).all()), name
        worst = float((lp.double() - want).abs().max())
        print(f"[logprobs snapshots] {kind} {dtype} {name}: worst {worst:.3e}")
        assert worst <= VAL_TOL, name
        if name == "prompted":
            assert first.tolist() == PROMPT_LENS
        if name == "dense with a prefix":
            assert first.tolist() == [3] * N_IMG


@pytest.mark.parametrize("kind", KINDS)
def test_search_beam_values_sum_to_the_scores_bit_for_bit(hip, kind, images, monkeypatch):
    """The values are the bits ``dh_beam_row_best`` left in ``pick_val``: a numpy float32 loop over a live beam's own columns, left to
    right, gives ``BeamCaptions.scores`` exactly -- dense, behind a prefix and prompted."""
    model = build(kind)
    kw = dict(KW, search="beam")
    for name in ("plain", "dense with a prefix", "prompted"):
        extra = VARIANTS[name]() if name != "plain" else {}
        beams, lp, want, first = tracked(model, kind, images, monkeypatch, **kw, **extra)
        scores, lens, vals = beams.scores.cpu().numpy(), beams.lengths.cpu(), lp.numpy()
        live = 0
        for i in range(N_IMG):
            for j in range(BEAM):
                if not np.isfinite(scores[i, j]):
                    continue
                acc = np.float32(0.0)
                for c in range(int(first[i]), int(lens[i, j])):
                    acc = np.float32(acc + vals[i, j, c])
                assert acc.tobytes() == scores[i, j].tobytes(), (name, i, j, float(acc), float(scores[i, j]))
                live += 1
        assert live == N_IMG * BEAM
        assert float((lp.double() - want).abs().max()) <= VAL_TOL       # and they are the logits' log_softmax at the tokens
        assert same(gen(model, model_args(kind, images), return_beams=True, **kw, **extra), beams)


def forward_logprobs(model, kind, images, tokens):
    """fp64 ``log_softmax`` of the teacher-forced ``forward`` at the rows' own tokens (``tests/test_beam_search_gpu.py``'s recipe)."""
    rows, n = tokens.shape
    rep = rows // images.shape[0]
    lens = torch.full((rows,), n, dtype=torch.int64)
    with torch.no_grad():
        if "WithLabels" in kind:
            logits = model(images.repeat_interleave(rep, 0), tokens.cuda(), lens, labels().cuda().repeat_interleave(rep, 0))
        else:
            logits = model(images.repeat_interleave(rep, 0), tokens.cuda(), lens)
    lp = torch.log_softmax(logits[:, :n].double().cpu(), -1)
    return lp.gather(-1, tokens.cpu().long().unsqueeze(-1)).squeeze(-1)


_forward_worst = {}


@pytest.mark.parametrize("kind", KINDS)
def test_values_are_the_teacher_forced_forward(hip, kind, images):
    """fp32, no edits, temperature 1, ``search="sample"``: every value against the model's own ``forward`` on the beam's own tokens."""
    model = build(kind)
    beams, lp = gen(model, model_args(kind, images), return_beams=True, return_logprobs=True, **dict(KW, temperature=1.0))
    want = forward_logprobs(model, kind, images, beams.tokens.reshape(N_IMG * BEAM, MAX_LEN)).view(N_IMG, BEAM, MAX_LEN)
    own = torch.arange(MAX_LEN)[None, None, :] < beams.lengths.cpu()[:, :, None]
    worst = float((lp.cpu().double() - want)[own].abs().max())
    _forward_worst[kind] = worst
    print(f"[logprobs forward] {kind}: worst {worst:.3e}; over the kinds so far {max(_forward_worst.values()):.3e} "
          f"(gate {FORWARD_GATE if FORWARD_GATE is None else format(FORWARD_GATE, '.3e')})")
    assert FORWARD_GATE is not None and FORWARD_GATE < 2e-3
    assert worst <= FORWARD_GATE


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_bitwise_self_consistency(hip, kind, dtype, images):
    model = build(kind, dtype)
    args = model_args(kind, images)
    toks, lens, lp = gen(model, args, return_logprobs=True, **KW)
    assert same((toks, lens), gen(model, args, **KW)) and lp.shape == (N_IMG, MAX_LEN) and lp.dtype == torch.float32 and lp.is_cuda
    beams, lp4 = gen(model, args, return_beams=True, return_logprobs=True, **KW)
    assert same(beams, gen(model, args, return_beams=True, **KW)) and lp4.shape == (N_IMG, BEAM, MAX_LEN)
    assert torch.equal(lp, lp4[torch.arange(N_IMG), beams.drawn])                            # the plain call = the drawn slot
    again = gen(model, args, return_beams=True, return_logprobs=True, **KW)                  # two calls, one seed
    assert same(again[0], beams) and torch.equal(again[1], lp4)
    assert not torch.equal(gen(model, args, return_logprobs=True, **dict(KW, seed=6))[2], lp)
    for extra in (dict(streams=2), dict(early_stop_every=2), dict(streams=2, early_stop_every=2)):
        b2, l2 = gen(model, args, return_beams=True, return_logprobs=True, **KW, **extra)
        assert same(b2, beams) and torch.equal(l2, lp4), extra
        assert same(gen(model, args, return_logprobs=True, **KW, **extra), (toks, lens, lp)), extra
    # generate = row 0
    with torch.no_grad():
        cap, l1 = model.generate(*model_args(kind, images, 0, 1), return_logprobs=True, **KW)
        b1, lb1 = model.generate(*model_args(kind, images, 0, 1), return_logprobs=True, return_beams=True, **KW)
    n0 = int(lens[0])
    assert torch.equal(cap, toks[0, :n0]) and l1.shape == (n0,) and torch.equal(l1, lp[0, :n0])
    assert torch.equal(lb1, lp4[:1]) and same(b1, beams.map(lambda t: t[:1]))
    # a prompted batch = the four dense single-image calls
    cap = captions_and_lengths()[0][:N_IMG, :5].cuda()
    pt, pl, pp = gen(model, args, caption=cap, caption_lengths=torch.tensor(PROMPT_LENS), return_logprobs=True, **KW)
    assert same((pt, pl), gen(model, args, caption=cap, caption_lengths=torch.tensor(PROMPT_LENS), **KW))
    for i, n in enumerate(PROMPT_LENS):
        st, sl, sp = gen(model, model_args(kind, images, i, i + 1), caption=cap[i:i + 1, :n] if n else None, img0=i, return_logprobs=True, **KW)
        assert torch.equal(st[0], pt[i]) and torch.equal(sl[0], pl[i]) and torch.equal(sp[0], pp[i]), (i, n)
        assert bool((pp[i, :n] == 0).all()) and bool((pp[i, n:int(pl[i])] < 0).all())
    # the other generators and the general sampler carry it too, and change no token
    for extra in (dict(rng="torch"), dict(exact=True), dict(top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.2, min_len=3)):
        t3 = gen(model, args, return_logprobs=True, **KW, **extra)
        assert same(t3[:2], gen(model, args, **KW, **extra)) and t3[2].shape == (N_IMG, MAX_LEN), extra
    if kind in CROSS:                                                 # both keywords: each tensor is its single-keyword call's
        both = gen(model, args, return_attention=True, return_logprobs=True, **KW)
        att = gen(model, args, return_attention=True, **KW)
        assert len(both) == 4 and same(both[:3], att) and torch.equal(both[3], lp)
        bb = gen(model, args, return_beams=True, return_attention=True, return_logprobs=True, **KW)
        assert len(bb) == 3 and same(bb[0], beams) and torch.equal(bb[2], lp4)
        assert torch.equal(bb[1], gen(model, args, return_beams=True, return_attention=True, **KW)[1])
    from deephumor_amd.experiments import beam_logprob_scores
    total = beam_logprob_scores(beams, lp4)
    assert total.shape == (N_IMG, BEAM) and torch.allclose(total, lp4.sum(-1)) and bool((total < 0).all())


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graph_replay(hip, kind, images):
    model = build(kind, torch.bfloat16)
    args = model_args(kind, images)
    kw = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20)
    first = None
    for seed in (3, 4):
        with torch.no_grad():
            got = model.generate_batch_graphed(*args, seed=seed, return_logprobs=True, **kw)
            plain = model.generate_batch_graphed(*args, seed=seed, **kw)
            beams, blp = model.generate_batch_graphed(*args, seed=seed, return_logprobs=True, return_beams=True, **kw)
        want = gen(model, args, seed=seed, return_logprobs=True, **kw)
        assert len(got) == 3 and same(got, want) and len(plain) == 2 and same(plain, want[:2])
        assert torch.equal(blp[torch.arange(N_IMG), beams.drawn], want[2])
        if first is None:
            first = (got, tuple(t.clone() for t in got))
    assert same(*first) and not torch.equal(first[0][2], got[2])      # the second replay left the first result alone
    n_graphs = len(model._graphs)
    with torch.no_grad():                     # return_logprobs=False is the plain call: the plain graph, not one more
        off = model.generate_batch_graphed(*args, seed=4, return_logprobs=False, **kw)
        best = model.generate_batch_graphed(*args, return_logprobs=True, search="beam", **kw)
    assert same(off, plain) and len(model._graphs) == n_graphs + 1
    assert same(best, gen(model, args, return_logprobs=True, search="beam", **kw))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_default_is_the_call_without_the_keyword(hip, images, kind, monkeypatch):
    """Equal outputs and the same launches, counted at ``hip._launch``; on, one pick launch behind every row draw, one record launch
    behind every select, the n-best final draw and one gather -- nothing else."""
    model = build(kind, torch.bfloat16)
    args = model_args(kind, images)
    kw = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=10, seed=1)
    names = []
    real = hip._launch

    def counting(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", counting)

    def run(**extra):
        del names[:]
        return gen(model, args, **kw, **extra), list(names)
    run()
    new = {"dh_beam_pick_logprobs", "dh_beam_record_logprobs", "dh_beam_gather_logprobs"}
    for streams in (1, 2):
        plain, p_names = run(streams=streams)
        off, off_names = run(streams=streams, return_logprobs=False)
        assert same(plain, off) and off_names == p_names and not new & set(p_names)
        on, on_names = run(streams=streams, return_logprobs=True)
        assert same(on[:2], plain)
        want = []
        for n in p_names:
            want.append("dh_beam_finalize_beams" if n == "dh_beam_finalize" else n)
            if n.startswith("dh_beam_row_sample"):
                want.append("dh_beam_pick_logprobs")
            elif n in ("dh_beam_select", "dh_beam_select_prompted"):
                want.append("dh_beam_record_logprobs")
            elif n == "dh_beam_finalize":
                want.append("dh_beam_gather_logprobs")
        assert on_names == want and on_names.count("dh_beam_gather_logprobs") == streams
        steps = MAX_LEN if "LSTM" in kind else MAX_LEN + 1
        assert on_names.count("dh_beam_pick_logprobs") == on_names.count("dh_beam_record_logprobs") == steps * streams
    best, b_names = run(search="beam")
    best_on, bo_names = run(search="beam", return_logprobs=True)
    assert same(best_on[:2], best) and [n for n in bo_names if n not in new] == b_names
    assert bo_names.count("dh_beam_pick_logprobs") == bo_names.count("dh_beam_record_logprobs") == MAX_LEN


def test_refusals(hip, images):
    from deephumor_amd import dist
    from deephumor_amd.pipeline import CaptionPipeline
    kind = "CaptioningTransformer"
    model = build(kind)
    args = model_args(kind, images)
    one = build(kind, pad_index=1)
    small = dict(max_len=6, beam_size=2, top_k=5)
    for call in (one.generate_batch, one.generate, one.generate_batch_graphed):
        with pytest.raises(NotImplementedError, match="return_logprobs with pad_index == 1"):
            call(*model_args(kind, images, 0, 1), return_logprobs=True, **small)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="pad_index == 1"):
            one.decode(one.encode(*args), return_logprobs=True, **small)
        for m in (model, build("CaptioningLSTM")):
            with pytest.raises(TypeError, match="return_logprobs must be a bool"):
                m.decode(m.encode(images), return_logprobs=1, **small)
            with pytest.raises(TypeError, match="return_logprobs must be a bool"):
                m.generate_batch(images, return_logprobs="yes", **small)
    with pytest.raises(NotImplementedError, match="^return_logprobs: "):
        CaptionPipeline(model, return_logprobs=True, **small)
    with pytest.raises(TypeError, match="must be a bool"):
        CaptionPipeline(model, return_logprobs=1, **small)
    assert "return_logprobs" not in CaptionPipeline(model, return_logprobs=False, **small).gen_kw
    with pytest.raises(NotImplementedError, match="return_logprobs"):
        dist.generate_sharded(lambda lo, hi: gen(model, model_args(kind, images, lo, hi), seed=1, img0=lo, return_logprobs=True, **small), N_IMG)
