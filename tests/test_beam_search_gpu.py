"""``search="beam"`` on a real MI355X: ``dh_beam_row_best`` and ``dh_beam_select_best`` against the torch-CPU restatement
(``tests/beam_search_ref.py``), and ``generate_batch(..., search="beam")`` end to end -- step by step on the engine's own snapshots,
scores against the teacher-forced ``forward``, greedy, determinism, every layer that carries the keyword -- plus the unchanged default."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from beam_search_ref import State, beam_search, candidate_gaps, finalize_best, row_best, select_best  # noqa: E402
from helpers import KINDS, captions_and_lengths, shapes_to_sd, synth_images, synth_state_dict  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF, NAN, INF = float("-inf"), float("nan"), float("inf")
UNK, EOS = 1, 3
VAL_TOL = 2e-5          # fp32 expf + a ~16-level tree sum over 36 k terms (~1.2e-6 on log(sum)) + ulp(32) ~ 1.9e-6 on x/T - m and x/T - lse


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


# ---- 1. dh_beam_row_best against the restatement ----------------------------------------------------------------------------------
ROWS = 8


def make_rows(v, beam, seed=0):
    """Eight rows, |x| <= 32: random; <unk> as the arg-max; bit-equal logits straddling the ``beam``-th place; half the columns
    ``-inf``; ``beam - 1`` finite eligible logits beside a finite <unk>; a constant row; signed zeros on top; and the largest logits
    gathered in the columns that fewer than ``beam - 1`` threads of a 256-thread, 16-byte sweep own (``BIG``), which at ``V = 36,541``,
    ``beam = 64`` puts ~8,800 columns above the sweep's bound: the flat-row fall-back."""
    g = torch.Generator().manual_seed(1000 * v + beam + seed)
    x = (torch.randn(ROWS, v, generator=g) * 2.5).clamp_(-30.0, 30.0)
    x[0, UNK] = float(x[0].max()) + 1.5
    if v >= beam + 3:
        cols = torch.randperm(v, generator=g)[:beam + 2]
        cols = cols[cols != UNK][:beam + 1]
        top = torch.sort(x[1], descending=True).values
        x[1, cols] = float(top[max(beam - 2, 0)])       # beam + 1 equal logits from about the (beam - 1)-th place on: index decides
    x[2, torch.rand(v, generator=g) < 0.5] = NINF
    keep = torch.tensor([c for c in torch.randperm(v, generator=g).tolist() if c != UNK][:beam - 1], dtype=torch.int64)
    row3 = torch.full((v,), NINF)
    row3[keep] = x[3, keep]
    row3[UNK] = 4.0
    x[3] = row3
    x[4] = 0.75
    x[5] = (x[5].abs() * -1.0)
    z = torch.randperm(v, generator=g)[:min(v, beam + 2)]
    x[5, z[::2]], x[5, z[1::2]] = 0.0, -0.0
    x[6] = torch.where(BIG(v, beam), x[6].abs() + 8.0, -x[6].abs() - 8.0)
    return x


def BIG(v, beam):
    c = torch.arange(v) % 1024
    return (c >= 4) & (c < 4 * (beam - 2))


def group_max(h, x):
    rows, v = x.shape
    ng = h.n_groups(v)
    pad = torch.full((rows, ng * 64), NINF)
    pad[:, :v] = x
    return pad.view(rows, ng, 64).max(-1).values.cuda()


def run_row_best(h, x, beam, temp, rpi=1, gmax=False, first_pos=None, step=0, pad=0, fill=-7):
    """``x`` on the device with ``pad`` columns of garbage behind every row (``ldl = V + pad``)."""
    rows, v = x.shape
    buf = torch.full((rows, v + pad), 1e30)
    if pad:
        buf[:, v::2], buf[:, v + 1::2] = NAN, INF
    buf[:, :v] = x
    dev = buf.cuda()[:, :v]
    pi = torch.full((rows, beam), fill, dtype=torch.int32, device="cuda")
    pv = torch.full((rows, beam), -7.0, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    h.beam_row_best(dev, v, rows, rpi, beam, temp, UNK, step, pi, pv, err, group_max=group_max(h, x) if gmax else None, first_pos=first_pos)
    torch.cuda.synchronize()
    return pi.cpu().long(), pv.cpu(), int(err.item())


def same_vals(got, want, tol):
    """``-inf`` where the restatement has ``-inf``, within ``tol`` elsewhere; returns the largest difference."""
    dead = want == NINF
    assert torch.equal(got == NINF, dead)
    diff = (got.double() - want)[~dead].abs()
    worst = float(diff.max()) if diff.numel() else 0.0
    assert worst <= tol, worst
    return worst


_ref = {}


def reference(v, beam, temp):
    key = (v, beam, temp)
    if key not in _ref:
        x = make_rows(v, beam)
        _ref[key] = (x,) + row_best(x, temp, beam, UNK)
    return _ref[key]


ROW_CASES = [(v, b) for v in (2, 71, 1000, 36541) for b in (1, 3, 5, 64) if b <= v - 1]


@pytest.mark.parametrize("temp", (1.0, 1.3))
@pytest.mark.parametrize("v,beam", ROW_CASES)
def test_row_best_matches_the_restatement(hip, v, beam, temp):
    """Picks exact, values within 2e-5 of fp64, the error word the OR of the rows' bits -- with and without group maxima, at
    ``rows_per_img`` 1 and ``beam``, on 16-byte aligned rows and on rows that are not (``ldl = V + 3`` with NaN / +inf in the pad) --
    and two runs bit-identical."""
    x, picks, vals, errs = reference(v, beam, temp)
    assert float((x[torch.isfinite(x)] / temp).abs().max()) <= 32.0
    want_err = 0
    for e in errs:
        want_err |= e
    assert errs[3] == (4 if beam > 1 else 1) and errs[0] == errs[4] == errs[6] == errs[7] == 0
    worst = 0.0
    for pad in (0, 3, 4 - v % 4):                                     # (the row's alignment decides which thread sums which columns)
        runs = []
        for gmax in (False, True, False):
            for rpi in (1, beam):
                pi, pv, err = run_row_best(hip, x, beam, temp, rpi=rpi, gmax=gmax, pad=pad)
                assert torch.equal(pi, picks), (gmax, rpi, pad)
                worst = max(worst, same_vals(pv, vals, VAL_TOL))
                assert err == want_err
                runs.append(pv)
        for pv in runs[1:]:                                           # a second run, and the other route: the same bits
            assert torch.equal(pv.view(torch.int32), runs[0].view(torch.int32)), pad
    print(f"V={v} beam={beam} T={temp}: max |pick_val - fp64| = {worst:.3e}")
    assert int(picks[0, 0]) != UNK and bool((picks != UNK).all())
    assert picks[4].tolist() == [c for c in range(v) if c != UNK][:beam]                 # a constant row: the lowest eligible indices


def test_row_best_flat_row_premise_and_answer(hip):
    """The premise of row 6 at ``V = 36,541``, ``beam = 64``: far more than 1,024 columns reach the bound a 256-thread sweep can find
    (the 64-th largest of 256 per-thread bests), whichever way the threads split the row."""
    x, picks, _, _ = reference(36541, 64, 1.0)
    big = BIG(36541, 64)
    assert int(big.sum()) > 8 * 1024 and bool((x[6][big] > 0).all()) and bool((x[6][~big] < 0).all())
    cols = big.nonzero().flatten()
    for head in range(4):               # columns in front of the row's first 16-byte boundary; thread t owns loads t, t + 256, ...
        owners = set((((cols - head) % 1024) // 4).tolist())
        assert len(owners) <= 62        # fewer than beam - 1 threads hold every large logit: the 64-th thread best is a small one
    assert sorted(picks[6].tolist()) == sorted(torch.topk(x[6], 64).indices.tolist())


def test_row_best_nonfinite_and_all_filtered(hip):
    v, beam = 1000, 3
    x = make_rows(v, beam)[:4].clone()
    for bad, bit in ((NAN, 8), (INF, 8)):
        y = x.clone()
        y[2, 777] = bad
        picks, vals, errs = row_best(y, 1.0, beam, UNK)
        assert errs[2] == bit
        for gmax in (False, True):
            pi, pv, err = run_row_best(hip, y, beam, 1.0, gmax=gmax, pad=1)
            assert err == bit | 4 and torch.equal(pi, picks) and pi[2].tolist() == [0] * beam and pv[2].tolist() == [0.0] * beam
            same_vals(pv, vals, VAL_TOL)
    y = x.clone()
    y[0] = NINF
    y[0, UNK] = 2.0                                                    # only <unk> is finite
    y[1] = NINF                                                        # nothing is
    picks, vals, errs = row_best(y, 1.3, beam, UNK)
    assert errs[:2] == [1, 1]
    pi, pv, err = run_row_best(hip, y, beam, 1.3)
    assert err == 1 | 4 and torch.equal(pi, picks) and pv[:2].tolist() == [[0.0] * beam] * 2
    same_vals(pv, vals, VAL_TOL)
    flat = torch.full((2, 5000), 0.25)                                 # what overflows the samplers has an answer here
    pi, pv, err = run_row_best(hip, flat, 5, 1.0)
    assert err == 0 and pi.tolist() == [[0, 2, 3, 4, 5]] * 2


@pytest.mark.parametrize("v,gmax", [(71, False), (1000, True)])
def test_row_best_prompted_phases(hip, v, gmax):
    """Three images of ``beam = 3`` at position 2: forced (prompt of 4: its rows keep the sentinel and may hold NaN), first (prompt of
    2: its base row only) and normal (no prompt)."""
    beam, step = 3, 2
    g = torch.Generator().manual_seed(v)
    x = (torch.randn(9, v, generator=g) * 2.5).clamp_(-30, 30)
    x[0:3] = NAN
    x[4] = INF                                                         # a non-base row of the image at its first step: not read
    first_pos = torch.tensor([4, 2, 0], dtype=torch.int32, device="cuda")
    ok = x.clone()
    ok[0:3], ok[4] = 0.0, 0.0
    picks, vals, _ = row_best(ok, 1.3, beam, UNK)
    pi, pv, err = run_row_best(hip, x, beam, 1.3, rpi=beam, gmax=gmax, first_pos=first_pos, step=step)
    assert err == 0
    live = [3, 6, 7, 8]
    idle = [0, 1, 2, 4, 5]
    assert torch.equal(pi[live], picks[live]) and bool((pi[idle] == -7).all()) and bool((pv[idle] == -7.0).all())
    same_vals(pv[live], vals[live], VAL_TOL)


# ---- 2. dh_beam_select_best against the fp32 restatement, bitwise ------------------------------------------------------------------
def random_state(n_img, beam, tok_ld, with_src, seed):
    g = torch.Generator().manual_seed(seed)
    r = n_img * beam
    st = State(n_img, beam, tok_ld, src_len=tok_ld + 1 if with_src else 0)
    st.tokens = torch.randint(4, 50, (r, tok_ld), generator=g, dtype=torch.int32)
    st.vals = (torch.randint(-12, 0, (r,), generator=g).float() * 0.25)          # quarters: many equal candidate scores
    st.ended = (torch.rand(r, generator=g) < 0.3).to(torch.uint8)
    st.vals[torch.rand(r, generator=g) < 0.15] = NINF                             # dead beams
    if with_src:
        st.src = (torch.randint(0, beam, (r, tok_ld + 1), generator=g, dtype=torch.int32)
                  + (torch.arange(r, dtype=torch.int32) // beam * beam)[:, None])
    st.parent = torch.full((r,), -5, dtype=torch.int32)
    st.hparent = torch.full((r,), -5, dtype=torch.int32)
    if n_img > 2:
        st.done[2], st.end_step[2] = 1, 1                                         # a finished image: frozen
    if n_img > 1:
        st.ended[beam:2 * beam] = 1                                               # every beam ended: the image finishes in this step
    pick_idx = torch.randint(0, 50, (r, beam), generator=g, dtype=torch.int32)
    pick_idx[torch.rand(r, beam, generator=g) < 0.2] = EOS
    pick_val = torch.sort(torch.randint(-8, 0, (r, beam), generator=g).float() * 0.25, dim=1, descending=True).values
    pick_val[torch.rand(r, beam, generator=g) < 0.1] = NINF
    return st, pick_idx, pick_val


def run_select(h, st, pick_idx, pick_val, first, write_pos, t, step, first_pos=None):
    dev = {k: None if v is None else v.clone().cuda() for k, v in st.fields().items()}
    fp = None if first_pos is None else torch.tensor(first_pos, dtype=torch.int32, device="cuda")
    h.beam_select_best(pick_idx.cuda(), pick_val.cuda(), dev["tokens"], dev["vals"], dev["ended"], dev["src"], dev["parent"], dev["hparent"],
                       dev["done"], dev["end_step"], st.n_img, st.beam, first, True, write_pos, t, step, EOS, first_pos=fp)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in dev.items()}


def same_state(got, st):
    for k, want in st.fields().items():
        if want is None:
            continue
        if k == "vals":
            assert torch.equal(got[k].view(torch.int32), want.view(torch.int32)), k          # bitwise
        else:
            assert torch.equal(got[k], want), k


@pytest.mark.parametrize("with_src", (False, True), ids=("lstm", "src"))
@pytest.mark.parametrize("beam", (1, 3, 5, 64))
def test_select_best_is_the_restatement_bit_for_bit(hip, beam, with_src):
    """Dense first and later steps, the prompted phases, and the step at ``write_pos == tok_ld`` that writes no token: tokens, vals,
    ended, src, parent, hparent, done and end_step -- with ended beams, a finished image, equal candidate scores and ``-inf``."""
    tok_ld, t = 6, 3
    for case, (first, write_pos, first_pos) in enumerate([(True, 0, None), (False, 3, None), (False, tok_ld, None), (False, 3, [5, 3, 1]),
                                                          (False, 3, [3, 0, 4])]):
        st, pick_idx, pick_val = random_state(3, beam, tok_ld, with_src, 17 * beam + case)
        if first:
            st.vals.zero_()
            st.ended.zero_()
            st.done.zero_()
        got = run_select(hip, st, pick_idx, pick_val, first, write_pos, t, 3, first_pos)
        before = st.vals.clone()
        select_best(st, pick_idx, pick_val, first, write_pos, t, 3, EOS, first_pos=first_pos)
        same_state(got, st)
        if not first and first_pos is None:
            assert st.done[1] == 1 and st.end_step[1] == 3 and not torch.equal(before, st.vals)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
N_IMG, BEAM, MAX_LEN = 4, 3, 8
KW = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20, search="beam")
GAP = 1e-3


@pytest.fixture(scope="module")
def images():
    return synth_images(N_IMG, seed=0)


def labels():
    return captions_and_lengths()[2]


_models = {}


def cpu_search(kind, sd, hp, images, gaps):
    """The whole search restated on the CPU over the torch-CPU model (``oracle.ref_path``): which (image, position) steps are coin
    tosses is a property of the weights, known before the GPU is asked anything."""
    from oracle import ref_path
    with torch.no_grad():
        start, enc = ref_path._encode(kind, sd, images, labels() if "WithLabels" in kind else None)
        lstm = "LSTM" in kind

        def logits_fn(tokens, pos, rpi):
            rep = lambda t: None if t is None else t.repeat_interleave(rpi, 0)
            toks = tokens.long()
            if lstm:
                return ref_path.lstm_decoder_forward(sd, "decoder", rep(start), toks[:, :pos])[:, pos]
            return ref_path.transformer_forward(sd, "decoder", toks, rep(enc), rep(start), hp["pad_index"], hp["n_heads"])[:, pos]
        return beam_search(logits_fn, images.shape[0], BEAM, MAX_LEN, 1.0, UNK, EOS, hp.get("pad_index", 0), 1 if lstm else 0, gaps)


def left_out(gaps):
    flat = [g for _, per_img in gaps for g in per_img]
    return sum(g < GAP for g in flat) / len(flat)


def build(kind, images):
    """A fresh fp32 model on the first weight seed (of 64 at most) whose restated search leaves out at most 5 % of its steps; with it
    that share.  The seed is found once per kind."""
    import deephumor_amd.models as M
    if kind not in _models:
        shapes, hp = shapes_to_sd(kind)
        for seed in range(64):
            sd = synth_state_dict(shapes, seed=1234 + seed)
            gaps = []
            cpu_search(kind, sd, hp, images, gaps)
            if left_out(gaps) <= 0.05:
                break
        _models[kind] = (sd, hp, left_out(gaps))
    sd, hp, share = _models[kind]
    model = getattr(M, kind)(**hp).eval()
    model.load_state_dict(sd)
    return model.cuda(), share


def model_args(kind, images, lo=0, hi=N_IMG):
    return (images[lo:hi].cuda(), labels()[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


def snapshots(monkeypatch):
    """Every beam step and the final step of the calls made from now on: the engine's own state in front of and behind each."""
    from deephumor_amd.models.beam import BeamSearchHelper
    steps, finals = [], []
    real_step, real_final = BeamSearchHelper._draw_and_select, BeamSearchHelper.finalize
    c = lambda t: None if t is None else t.detach().cpu().clone()

    def state_of(h):
        return dict(tokens=c(h.tokens), vals=c(h.vals), ended=c(h._ended), done=c(h.done), end_step=c(h.end_step), src=c(h.src))

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        rec = dict(logits=c(logits.float()), first=first, write_pos=write_pos, t=t, step=step_index, prompted=prompted,
                   first_pos=None if self.first_pos is None or not prompted else self.first_pos.cpu().tolist(), before=state_of(self),
                   temperature=self.temperature, unk=self.unk_index, eos=self.eos_index, beam=self.beam_size)
        real_step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted)
        rec["after"] = state_of(self)
        steps.append(rec)

    def final(self, len_bias_done, full_len, pad_index=0, **kw):
        finals.append(dict(state=state_of(self), len_bias_done=len_bias_done, full_len=full_len, pad_index=pad_index, pos=kw.get("pos", 0),
                           first_pos=None if self.first_pos is None else self.first_pos.cpu().tolist(), beam=self.beam_size, eos=self.eos_index))
        return real_final(self, len_bias_done, full_len, pad_index, **kw)
    monkeypatch.setattr(BeamSearchHelper, "_draw_and_select", step)
    monkeypatch.setattr(BeamSearchHelper, "finalize", final)
    return steps, finals


def check_steps(steps):
    """The restatement applied to every snapshot gives the next one's tokens and ended flags; returns (checked, left out)."""
    checked = skipped = 0
    for rec in steps:
        b = rec["beam"]
        if rec["write_pos"] >= rec["before"]["tokens"].shape[1]:      # the Transformer decoders' last step writes no token: skipped
            for k in ("tokens", "vals", "ended", "done"):
                assert torch.equal(rec["after"][k], rec["before"][k]), k
            continue
        st = State.of(beam=b, **rec["before"])
        picks, vals, errs = row_best(rec["logits"], rec["temperature"], b, rec["unk"])
        gaps = candidate_gaps(st, picks, vals, rec["first"], rec["first_pos"], rec["step"])
        select_best(st, picks, vals.to(torch.float32), rec["first"], rec["write_pos"], rec["t"], rec["step"], rec["eos"], first_pos=rec["first_pos"])
        for img, gap in enumerate(gaps):
            if gap < GAP:
                skipped += 1
                continue
            checked += 1
            rows = slice(img * b, (img + 1) * b)
            assert torch.equal(rec["after"]["tokens"][rows], st.tokens[rows]), (rec["step"], img)
            assert torch.equal(rec["after"]["ended"][rows], st.ended[rows]), (rec["step"], img)
            assert torch.allclose(rec["after"]["vals"][rows], st.vals[rows], rtol=0, atol=VAL_TOL * (rec["step"] + 1), equal_nan=True)
    return checked, skipped


def same_captions(beams, fin):
    want = finalize_best(State.of(beam=fin["beam"], **fin["state"]), fin["len_bias_done"], fin["full_len"], fin["pad_index"], fin["eos"],
                         fin["pos"], fin["first_pos"])
    for k in ("tokens", "lengths", "beam_index", "drawn", "row_lengths"):
        assert torch.equal(getattr(beams, k).cpu(), want[k]), k
    assert torch.equal(beams.scores.cpu().view(torch.int32), want["scores"].view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_by_step_on_the_engines_own_snapshots(kind, dtype, images, monkeypatch):
    model, cpu_out = build(kind, images)
    assert cpu_out <= 0.05
    model = model.to(dtype)
    steps, finals = snapshots(monkeypatch)
    with torch.no_grad():
        beams = model.generate_batch(*model_args(kind, images), return_beams=True, **KW)
    assert len(steps) == MAX_LEN + (0 if "LSTM" in kind else 1) and len(finals) == 1
    checked, skipped = check_steps(steps)
    print(f"{kind} {dtype}: {checked} steps checked, {skipped} left out (restatement alone: {cpu_out:.3f})")
    assert checked + skipped == N_IMG * MAX_LEN and skipped <= 0.05 * (checked + skipped)
    same_captions(beams, finals[0])
    assert beams.drawn.tolist() == [0] * N_IMG and bool((beams.scores[:, :-1] >= beams.scores[:, 1:]).all())


def forward_logprobs(model, kind, images, tokens, n):
    """fp64 ``log_softmax`` of the teacher-forced ``forward`` at the rows' own tokens: ``[rows, n]``."""
    rows = tokens.shape[0]
    imgs = images.cuda().repeat_interleave(rows // images.shape[0], 0)
    cap = tokens[:, :n].cuda()
    lens = torch.full((rows,), n, dtype=torch.int64)
    with torch.no_grad():
        if "WithLabels" in kind:
            logits = model(imgs, cap, lens, labels().cuda().repeat_interleave(rows // images.shape[0], 0))
        else:
            logits = model(imgs, cap, lens)
    lp = torch.log_softmax(logits[:, :n].double().cpu(), -1)
    return lp, lp.gather(-1, tokens[:, :n].cpu().long().unsqueeze(-1)).squeeze(-1)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_are_the_teacher_forced_log_probabilities(kind, images):
    """fp32, no edits, ``temperature = 1``: ``scores[i, j]`` is the sum of ``log_softmax(forward)`` at the beam's own tokens, from its
    first generated column through its own length, within ``length x 2e-5``."""
    model, _ = build(kind, images)
    with torch.no_grad():
        beams = model.generate_batch(*model_args(kind, images), return_beams=True, **KW)
    toks = beams.tokens.reshape(N_IMG * BEAM, -1)
    _, lp = forward_logprobs(model, kind, images, toks, toks.shape[1])
    lens = beams.lengths.reshape(-1).cpu()
    worst = 0.0
    for r in range(N_IMG * BEAM):
        n = int(lens[r])
        got, want = float(beams.scores.reshape(-1)[r]), float(lp[r, :n].sum())
        worst = max(worst, abs(got - want) / n)
        assert abs(got - want) <= n * VAL_TOL, (r, n, got, want)
    print(f"{kind}: max |score - forward| / length = {worst:.3e}")


@pytest.mark.parametrize("kind", KINDS)
def test_beam_size_one_is_greedy(kind, images):
    model, _ = build(kind, images)
    with torch.no_grad():
        toks, lens = model.generate_batch(*model_args(kind, images), **dict(KW, beam_size=1))
    full, _ = forward_logprobs(model, kind, images, toks, toks.shape[1])
    checked = 0
    for i in range(N_IMG):
        for pos in range(int(lens[i])):
            row = full[i, pos].clone()
            row[UNK] = NINF
            top = torch.topk(row, 2)
            if float(top.values[0] - top.values[1]) > GAP:
                assert int(toks[i, pos]) == int(top.indices[0]), (i, pos)
                checked += 1
    assert checked >= 0.9 * int(lens.sum())


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_deterministic_whatever_the_seed_and_the_generator(kind, images):
    model, _ = build(kind, images)
    args = model_args(kind, images)
    state = torch.get_rng_state()
    with torch.no_grad():
        a = model.generate_batch(*args, return_beams=True, **KW)
        assert torch.equal(torch.get_rng_state(), state)               # seed=None draws no key: the default generator is not read
        outs = [model.generate_batch(*args, return_beams=True, seed=s, **KW) for s in (1, 2)]
        outs.append(model.generate_batch(*args, return_beams=True, seed=5, rng="torch", **KW))
        outs.append(model.generate_batch(*args, return_beams=True, seed=5, rng="philox", **KW))
        outs.append(model.generate_batch(*args, return_beams=True, noise_source=lambda *a: (_ for _ in ()).throw(AssertionError("noise asked")), **KW))
        outs.append(model.generate_batch(*args, return_beams=True, streams=2, exact=True, **KW))
        plain = model.generate_batch(*args, **KW)
        sampled = model.generate_batch(*args, seed=1, **dict(KW, search="sample"))
    for o in outs:
        for x, y in zip(a, o):
            assert torch.equal(x, y)
    assert torch.equal(a.best()[0], plain[0]) and torch.equal(a.best()[1], plain[1]) and torch.equal(a.tokens[:, 0], plain[0])
    assert not torch.equal(sampled[0], plain[0])
    for i in range(N_IMG):                                            # a batch equals its singles
        with torch.no_grad():
            one = model.generate_batch(*model_args(kind, images, i, i + 1), img0=i, **KW)
        assert torch.equal(one[0], plain[0][i:i + 1]) and torch.equal(one[1], plain[1][i:i + 1])
    single = model.generate(*model_args(kind, images, 0, 1), **KW)
    assert single.tolist() == plain[0][0, :int(plain[1][0])].tolist()


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graphed_pipeline_and_prompted(kind, images):
    from deephumor_amd.pipeline import CaptionPipeline
    model, _ = build(kind, images)
    model = model.bfloat16()
    args = model_args(kind, images)
    with torch.no_grad():
        eager = model.generate_batch(*args, **KW)
        eager_b = model.generate_batch(*args, return_beams=True, **KW)
        for _ in range(2):                                            # capture, then replay
            g = model.generate_batch_graphed(*args, **KW)
            assert torch.equal(g[0], eager[0]) and torch.equal(g[1], eager[1])
        gb = model.generate_batch_graphed(*args, return_beams=True, seed=9, **KW)
        for x, y in zip(gb, eager_b):
            assert torch.equal(x, y)
        s = model.generate_batch_graphed(*args, seed=3, **dict(KW, search="sample"))
        e = model.generate_batch(*args, seed=3, **dict(KW, search="sample"))
        assert torch.equal(s[0], e[0])
    assert sorted(dict(k[2]).get("search", "sample") for k in model._graphs) == ["beam", "beam", "sample"]
    batches = [(images[:2],), (images[2:],)]
    got = [tuple(t.clone() for t in r) for r in CaptionPipeline(model, **KW).run(batches)]
    assert torch.equal(torch.cat([g[0] for g in got]).cpu(), eager[0].cpu()) and torch.equal(torch.cat([g[1] for g in got]).cpu(), eager[1].cpu())
    cap = torch.randint(6, 1000, (N_IMG, 3), generator=torch.Generator().manual_seed(2)).cuda()
    lens = torch.tensor([0, 2, 1, 3])
    with torch.no_grad():
        prompted = model.generate_batch(*args, caption=cap, caption_lengths=lens, rng="torch", return_beams=True, **KW)
        for i, n in enumerate(lens.tolist()):
            one = model.generate_batch(*model_args(kind, images, i, i + 1), caption=cap[i:i + 1, :n] if n else None, **KW)
            assert torch.equal(one[0], prompted.best()[0][i:i + 1]) and torch.equal(one[1], prompted.best()[1][i:i + 1]), (i, n)
            assert prompted.tokens[i, :, :n].tolist() == [cap[i, :n].tolist()] * BEAM
    assert prompted.drawn.tolist() == [0] * N_IMG


def violates(row, n, ngram, min_len, bad_words, first):
    """Does ``row[:n]`` repeat an n-gram, end before ``min_len``, or hold a banned phrase that ends in a generated column?"""
    toks = row[:n]
    grams = [tuple(toks[i:i + ngram]) for i in range(n - ngram + 1)]
    if any(grams.index(gr) != i and i + ngram > first for i, gr in enumerate(grams)):
        return "ngram"
    if EOS in toks[first:min_len]:
        return "min_len"
    for w in bad_words:
        for i in range(max(first - len(w) + 1, 0), n - len(w) + 1):
            if toks[i:i + len(w)] == list(w) and i + len(w) > first:
                return "bad word"
    return None


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_the_edits_and_the_bans(kind, images):
    model, _ = build(kind, images)
    args = model_args(kind, images)
    with torch.no_grad():
        free = model.generate_batch(*args, return_beams=True, **KW)
        bad = [[int(free.tokens[0, 0, 0])], [int(t) for t in free.tokens[1, 0, :2]], [int(free.tokens[2, 0, 1])]]
        got = model.generate_batch(*args, return_beams=True, no_repeat_ngram_size=2, min_len=4, bad_words_ids=bad, **KW)
        again = model.generate_batch_graphed(*args, return_beams=True, no_repeat_ngram_size=2, min_len=4, bad_words_ids=bad, **KW)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    assert not torch.equal(got.tokens, free.tokens)
    alive = torch.isfinite(got.scores)
    for i in range(N_IMG):
        for j in range(BEAM):
            if alive[i, j]:
                assert violates(got.tokens[i, j].tolist(), int(got.lengths[i, j]), 2, 4, bad, 0) is None, (i, j)
    assert bool(alive[:, 0].all()) and got.drawn.tolist() == [0] * N_IMG


@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningTransformerWithLabels"))
def test_return_attention(kind, images):
    model, _ = build(kind, images)
    args = model_args(kind, images)
    with torch.no_grad():
        beams, att = model.generate_batch(*args, return_beams=True, return_attention=True, **KW)
        toks, lens, att1 = model.generate_batch(*args, return_attention=True, **KW)
        plain = model.generate_batch(*args, **KW)
    assert torch.equal(toks, plain[0]) and torch.equal(lens, plain[1]) and torch.equal(att1, att[:, 0])
    sums = att.sum(-1).cpu()
    for i in range(N_IMG):
        for j in range(BEAM):
            n = int(beams.lengths[i, j])
            assert torch.allclose(sums[i, j, :n], torch.ones(n), atol=1e-5) and bool((att[i, j, n:] == 0).all())


# ---- 4. the default is unchanged ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_sample_is_the_call_without_the_keyword(kind, images, monkeypatch):
    from deephumor_amd import hip
    model, _ = build(kind, images)
    args = model_args(kind, images)
    kw = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20, seed=1)
    names = []
    real = hip._launch

    def launch(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", launch)
    runs = {}
    for tag, extra in (("plain", {}), ("sample", dict(search="sample")), ("beam", dict(search="beam"))):
        del names[:]
        with torch.no_grad():
            out = model.generate_batch(*args, return_beams=True, **kw, **extra)
        runs[tag] = (out, list(names))
    for x, y in zip(runs["plain"][0], runs["sample"][0]):
        assert torch.equal(x, y)                                       # bit for bit, the scores included
    assert runs["plain"][1] == runs["sample"][1]
    new = {"dh_beam_row_best", "dh_beam_select_best"}
    assert not new & set(runs["plain"][1]) and new <= set(runs["beam"][1])
    assert not {n for n in runs["beam"][1] if n.startswith("dh_beam_row_sample") or n in ("dh_beam_select", "dh_beam_select_prompted", "dh_beam_finalize")}
    rest = lambda ns: [n for n in ns if not n.startswith("dh_beam_")]
    assert rest(runs["beam"][1]) == rest(runs["plain"][1])            # the model's own launches are the same chain


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
kw = dict(max_len=8, beam_size=3, top_k=20, search="beam")
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, **kw)
    sampled = model.generate_batch(images, seed=11, **dict(kw, search="sample"))
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 2, always=True) for a in (0, 2)]
    got = tuple(torch.cat(ts, 0) for ts in zip(*halves))
    micro = generate_micro_sharded(fn, 4, 2, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want),
                              "differs": not same(sampled, want)}))
dist.barrier()
dist.destroy_process_group()
"""


def test_sharded_through_the_one_rank_group_equals_the_plain_call():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True, "differs": True}
