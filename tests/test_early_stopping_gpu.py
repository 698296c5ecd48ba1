"""``search="beam"`` with ``early_stopping`` on a real MI355X: ``dh_beam_select_pool`` / ``dh_beam_finalize_pool`` against the torch-CPU
restatement (``tests/early_stopping_ref.py``) bit for bit on every state and pool tensor, ``generate_batch`` end to end -- every select
and the finalize replayed on the engine's own snapshots, bit for bit --, the identity with today's search where no beam meets
``<eos>``, the unchanged default, every carrier of the keyword, and the host loop that now ends early.

The models are the synthetic ones of ``helpers.synthetic_sd`` with the classifier's ``<eos>`` bias raised the way
``test_length_penalty_gpu.py``'s ``build`` raises it: until ``<eos>`` stands ``EOS_MARGIN`` logits below a row's best token at the
position where it comes closest (measured once per kind on a search with the plain weights).  Nothing here is compared within a
tolerance: the select's inputs are the engine's own ``pick_idx`` / ``pick_val``, and one fp32 add and one fp32 multiply have one
answer."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_search_ref as R  # noqa: E402
import early_stopping_ref as ES  # noqa: E402
import length_penalty_ref as LP  # noqa: E402
from helpers import KINDS, captions_and_lengths, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")
UNK, EOS = 1, 3
FIELDS = ("tokens", "vals", "keys", "ended", "src", "parent", "hparent", "done", "end_step") + ES.POOL_FIELDS
OUT = ("tokens", "lengths", "scores", "beam_index", "drawn", "row_lengths")
# <eos> this far BELOW the rows' best token where it comes closest (negative: above).  test_length_penalty_gpu.py uses 0.5, which ends
# beams at different lengths; a pool of `beam_size` entries needs <eos> among an image's best `beam_size` candidates several times
EOS_MARGIN = -1.0
# ... except where that makes <eos> every row's best token at one position, so that every pool fills there at once with one length
# (measured: CaptioningTransformerWithLabels at -0.5 and below; at 0.0 its pools hold lengths 7 and 9 and two images are done at 6 and 8)
EOS_MARGINS = {"CaptioningTransformerWithLabels": 0.0}
EARLY_MARGIN = -3.0                                     # the early_stop_every test: every image must fill its pool


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_state(got, st, where=""):
    for k in FIELDS:
        want = getattr(st, k)
        if want is not None:
            assert torch.equal(bits(got[k]), bits(want)), (k, where)


# ---- 1. the two kernels against the restatement, bit for bit ------------------------------------------------------------------------
N_SEL, TOK_LD, V_SEL = 6, 12, 40


def random_state(beam, with_src, seed, len_w, write_pos, first_cols, first):
    """A mid-search state of 6 images under the pool's invariants: live beams with quarter-valued scores (many equal keys) and the key
    of their length, dead slots (``ended``) at ``-inf``; image 1 all dead, image 2 already done; pools that are empty (image 0),
    part-filled (1, 5), full with equal keys (3) and full with falling keys (2, 4)."""
    g = torch.Generator().manual_seed(seed)
    r = N_SEL * beam
    st = ES.new_state(N_SEL, beam, TOK_LD, src_len=TOK_LD + 1 if with_src else 0)
    st.tokens = torch.randint(4, V_SEL, (r, TOK_LD), generator=g, dtype=torch.int32)
    st.vals = torch.randint(-12, 0, (r,), generator=g).float() * 0.25
    st.ended = (torch.rand(r, generator=g) < 0.25).to(torch.uint8)
    if with_src:
        st.src = (torch.randint(0, beam, (r, TOK_LD + 1), generator=g, dtype=torch.int32)
                  + (torch.arange(r, dtype=torch.int32) // beam * beam)[:, None])
    st.parent = torch.full((r,), -5, dtype=torch.int32)
    st.hparent = torch.full((r,), -5, dtype=torch.int32)
    st.done[2], st.end_step[2] = 1, 1
    st.ended[beam:2 * beam] = 1
    if first:
        st.vals.zero_()
        st.ended.zero_()
    st.vals[st.ended.bool()] = NINF
    for row in range(r):
        cur = max(write_pos - first_cols[row // beam], 1)
        st.keys[row] = 0.0 if first else float(LP.key_of(st.vals[row].item(), len_w[cur]))
    st.pool_tokens = torch.randint(4, V_SEL, (N_SEL, beam, TOK_LD), generator=g, dtype=torch.int32)
    for img, n in enumerate((0, (beam + 1) // 2, beam, beam, beam, int(torch.randint(0, beam + 1, (), generator=g)))):
        keys = torch.sort(torch.randint(-10, -2, (beam,), generator=g).float() * 0.25, descending=True).values
        if img == 3:
            keys[:] = -1.5
        st.pool_keys[img, :n] = keys[:n]
        st.pool_vals[img, :n] = keys[:n] - 1.0
        st.pool_len[img, :n] = torch.randint(1, TOK_LD + 1, (n,), generator=g, dtype=torch.int32)
        st.pool_n[img] = n
    pick_idx = torch.randint(0, V_SEL, (r, beam), generator=g, dtype=torch.int32)
    pick_idx[torch.rand(r, beam, generator=g) < 0.2] = EOS
    pick_val = torch.sort(torch.randint(-8, 0, (r, beam), generator=g).float() * 0.25, dim=1, descending=True).values
    pick_val[torch.rand(r, beam, generator=g) < 0.1] = NINF                  # what a TOO_FEW row leaves, and <eos> under min_len
    return st, pick_idx, pick_val


def to_device(st):
    return {k: None if getattr(st, k) is None else getattr(st, k).clone().cuda() for k in FIELDS}


def run_select(h, st, pick_idx, pick_val, first, write_pos, t, step, len_w, mode, first_col, first_pos):
    dev = to_device(st)
    fp = None if first_pos is None else torch.tensor(first_pos, dtype=torch.int32, device="cuda")
    h.beam_select_pool(pick_idx.cuda(), pick_val.cuda(), dev["tokens"], dev["vals"], dev["keys"], dev["ended"], dev["src"], dev["parent"],
                       dev["hparent"], dev["done"], dev["end_step"], dev["pool_tokens"], dev["pool_keys"], dev["pool_vals"], dev["pool_len"],
                       dev["pool_n"], st.n_img, st.beam, first, mode, write_pos, t, step, EOS, len_w.cuda(), first_col=first_col, first_pos=fp)
    torch.cuda.synchronize()
    return dev


def run_finalize(h, dev, n, b, full_len, pad_index, out_ld=TOK_LD):
    out = torch.full((n, b, out_ld), -7, dtype=torch.int32, device="cuda")
    ints = torch.full((2 * n * b + 2 * n,), -7, dtype=torch.int32, device="cuda")
    o_len, o_idx, o_drawn, o_row = ints[:n * b].view(n, b), ints[n * b:2 * n * b].view(n, b), ints[2 * n * b:2 * n * b + n], ints[2 * n * b + n:]
    o_score = torch.zeros((n, b), dtype=torch.float32, device="cuda")
    h.beam_finalize_pool(dev["tokens"], dev["keys"], dev["ended"], dev["done"], dev["pool_tokens"], dev["pool_keys"], dev["pool_len"],
                         dev["pool_n"], out, o_len, o_score, o_idx, o_drawn, o_row, n, b, full_len, pad_index)
    torch.cuda.synchronize()
    return dict(tokens=out.long().cpu(), lengths=o_len.long().cpu(), scores=o_score.cpu(), beam_index=o_idx.long().cpu(),
                drawn=o_drawn.long().cpu(), row_lengths=o_row.long().cpu())


def same_out(got, want, where=""):
    for k in OUT:
        assert torch.equal(bits(got[k]), bits(want[k])), (k, where)


#         first  write_pos  first_col  first_pos (prompted: one image still forced, one at its first step, the rest at their own L)
CASES = [(True, 0, 0, None), (True, 3, 3, None), (False, 3, 0, None), (False, 6, 3, None), (False, TOK_LD - 1, 0, None),
         (False, 4, 0, [6, 4, 0, 2, 3, 1]), (False, 9, 0, [10, 9, 0, 6, 8, 2])]


@pytest.mark.parametrize("with_src", (False, True), ids=("lstm", "src"))
@pytest.mark.parametrize("beam", (1, 2, 5, 16, 17, 64))
def test_select_pool_and_finalize_pool_are_the_restatement_bit_for_bit(hip, beam, with_src):
    t = 3
    offered = entered = died = finished = 0
    for lp in (-1.0, 0.0, 1.0):
        len_w = LP.weights(lp, TOK_LD)
        for case, (first, write_pos, first_col, first_pos) in enumerate(CASES):
            cols = first_pos if first_pos is not None else [first_col] * N_SEL
            for mode in (True, False):
                st, pick_idx, pick_val = random_state(beam, with_src, 1000 * beam + 10 * case + int(lp * 4) + mode, len_w, write_pos, cols, first)
                before = {k: None if getattr(st, k) is None else getattr(st, k).clone() for k in FIELDS}
                dev = run_select(hip, st, pick_idx, pick_val, first, write_pos, t, write_pos, len_w, mode, first_col, first_pos)
                ES.select_pool(st, pick_idx, pick_val, first, write_pos, t, write_pos, EOS, len_w, mode, first_col=first_col, first_pos=first_pos)
                same_state({k: None if v is None else v.cpu() for k, v in dev.items()}, st, (lp, case, mode))
                for frozen in ([2] + ([0] if first_pos is not None else [])):             # the done image and the forced one
                    for k in ("tokens", "vals", "keys", "ended") + ES.POOL_FIELDS:
                        lo, hi = (frozen, frozen + 1) if k.startswith("pool") else (frozen * beam, (frozen + 1) * beam)
                        assert torch.equal(bits(getattr(st, k))[lo:hi], bits(before[k])[lo:hi]), (k, frozen)
                entered += int((st.pool_keys != before["pool_keys"]).any(1).sum())
                died += int((st.ended.bool() & ~before["ended"].bool()).sum())
                finished += int(st.done.sum()) - 1
                same_out(run_finalize(hip, dev, N_SEL, beam, TOK_LD, 9), ES.finalize_pool(st, TOK_LD, 9), (lp, case, mode))
                same_out(run_finalize(hip, dev, N_SEL, beam, 7, 0, out_ld=10), ES.finalize_pool(st, 7, 0, out_ld=10), (lp, case, mode, "narrow"))
    # the inputs exercise the rules: pools moved, images finished, slots died (counted on the restatement: at least 19 / 50 / 30 here)
    assert entered >= 10 and finished >= 10 and died > 0


def test_the_hand_worked_two_beam_search_on_the_device(hip):
    """``test_early_stopping_cpu.py``'s two-beam search: ``True`` is done at step 2, ``False`` at step 3 with the later hypothesis in
    front of the one it pushed out."""
    steps = [([[5, 6], [0, 0]], [[-0.5, -1.0], [0.0, 0.0]]), ([[EOS, 7], [EOS, 8]], [[-0.25, -2.0], [-0.5, -0.25]]),
             ([[9, EOS], [10, 11]], [[-0.125, -0.25], [-0.5, -1.0]]), ([[EOS, 12], [13, 14]], [[-0.0625, -3.0], [-0.125, -0.25]])]
    w = LP.weights(0.0, 8)
    for mode, end, keys, rows in ((True, 2, [-0.75, -1.5], [[5, EOS, 0, 0], [6, 8, EOS, 0]]), (False, 3, [-0.75, -1.4375], [[5, EOS, 0, 0], [6, 8, 9, EOS]])):
        st = ES.new_state(1, 2, 8)
        for pos, (pi, pv) in enumerate(steps):
            dev = run_select(hip, st, torch.tensor(pi, dtype=torch.int32), torch.tensor(pv), pos == 0, pos, 0, pos, w, mode, 0, None)
            for k in FIELDS:
                if dev[k] is not None:
                    setattr(st, k, dev[k].cpu())
        assert st.done.tolist() == [1] and st.end_step.tolist() == [end] and st.pool_keys[0].tolist() == keys
        out = run_finalize(hip, dev, 1, 2, 8, 0, out_ld=8)
        assert out["tokens"][0, :, :4].tolist() == rows and out["beam_index"][0].tolist() == [-1, -1] and out["scores"][0].tolist() == keys


# ---- 2. end to end on the engine's own snapshots ------------------------------------------------------------------------------------
N_IMG, BEAM, MAX_LEN = 4, 3, 10
KW = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20, search="beam")
_sds = {}


@pytest.fixture(scope="module")
def images():
    return synth_images(N_IMG, seed=0)


def labels():
    return captions_and_lengths()[2]


def model_args(kind, images, lo=0, hi=N_IMG):
    return (images[lo:hi].cuda(), labels()[lo:hi].cuda()) if "WithLabels" in kind else (images[lo:hi].cuda(),)


def load(kind, sd, hp, dtype=torch.float32):
    import deephumor_amd.models as M
    model = getattr(M, kind)(**hp).eval()
    model.load_state_dict(sd)
    return model.cuda().to(dtype)


def build(kind, images, dtype=torch.float32, boosted=True, margin=None):
    """The synthetic model of ``kind``; ``boosted``: with ``<eos>`` ``margin`` logits below the rows' best token at the position where
    the median distance between the two is smallest (``test_length_penalty_gpu.py``'s ``build``, the margin a parameter; ``None``:
    the kind's own, ``EOS_MARGINS`` / ``EOS_MARGIN``)."""
    margin = EOS_MARGINS.get(kind, EOS_MARGIN) if margin is None else margin
    if kind not in _sds:
        sd, hp = synthetic_sd(kind)
        seen = []
        with torch.no_grad():
            load(kind, sd, hp).generate_batch(*model_args(kind, images), logits_hook=lambda pos, lg: seen.append(lg.float().cpu().clone()), **KW)
        gap = min(float((x.max(1).values - x[:, EOS]).median()) for x in seen)
        bias = [k for k in sd if "classifier" in k and k.endswith("bias") and sd[k].shape[0] == hp["num_tokens"]]
        assert len(bias) == 1
        _sds[kind] = (sd, hp, bias[0], gap)
    sd, hp, bias, gap = _sds[kind]
    if boosted:
        sd = {k: v.clone() for k, v in sd.items()}
        sd[bias][EOS] += gap - margin
    return load(kind, sd, hp, dtype)


def snapshots(monkeypatch):
    """Every beam step and the final step of the calls made from now on: the engine's state and pool in front of and behind each, and
    the picks the row step left (the select does not write them)."""
    from deephumor_amd.models.beam import BeamSearchHelper
    steps, finals = [], []
    real_step, real_final = BeamSearchHelper._draw_and_select, BeamSearchHelper.finalize
    c = lambda t: None if t is None else t.detach().cpu().clone()

    def state_of(h):
        d = dict(tokens=c(h.tokens), vals=c(h.vals), keys=c(h.keys), ended=c(h._ended), done=c(h.done), end_step=c(h.end_step), src=c(h.src),
                 parent=c(h.parent), hparent=c(h.hparent))
        d.update({k: c(getattr(h, k)) for k in ES.POOL_FIELDS})
        return d

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        rec = dict(first=first, write_pos=write_pos, t=t, step=step_index, before=state_of(self), beam=self.beam_size, eos=self.eos_index,
                   first_pos=None if self.first_pos is None else self.first_pos.cpu().tolist())
        real_step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted)
        rec.update(after=state_of(self), pick_idx=c(self.pick_idx), pick_val=c(self.pick_val), first_col=self.first_col, len_w=c(self.len_w))
        steps.append(rec)

    def final(self, len_bias_done, full_len, pad_index=0, **kw):
        finals.append(dict(state=state_of(self), full_len=full_len, pad_index=pad_index, beam=self.beam_size))
        return real_final(self, len_bias_done, full_len, pad_index, **kw)
    monkeypatch.setattr(BeamSearchHelper, "_draw_and_select", step)
    monkeypatch.setattr(BeamSearchHelper, "finalize", final)
    return steps, finals


def state_from(snap, beam):
    st = R.State.of(snap["tokens"], snap["vals"], snap["ended"], snap["done"], snap["end_step"], beam, snap["src"], snap["parent"], snap["hparent"])
    st.keys = snap["keys"].clone()
    for k in ES.POOL_FIELDS:
        setattr(st, k, snap[k].clone())
    return st


def check_steps(steps, length_penalty, mode, max_len):
    """The restatement applied to every snapshot, with the engine's own picks, gives the next snapshot bit for bit."""
    moved = 0
    for rec in steps:
        assert torch.equal(rec["len_w"], LP.weights(length_penalty, max_len))
        st = state_from(rec["before"], rec["beam"])
        if rec["write_pos"] < rec["before"]["tokens"].shape[1]:              # (the Transformer decoders' last step writes no token: skipped)
            ES.select_pool(st, rec["pick_idx"], rec["pick_val"], rec["first"], rec["write_pos"], rec["t"], rec["step"], rec["eos"], rec["len_w"],
                           mode, first_col=rec["first_col"], first_pos=rec["first_pos"])
            moved += 1
        same_state(rec["after"], st, rec["step"])
    return moved


def same_captions(beams, fin):
    want = ES.finalize_pool(state_from(fin["state"], fin["beam"]), fin["full_len"], fin["pad_index"])
    for k in OUT:
        assert torch.equal(bits(getattr(beams, k).cpu()), bits(want[k])), k


def same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    flat = lambda xs: [t for x in xs for t in (x if isinstance(x, tuple) else (x,))]
    return len(flat(a)) == len(flat(b)) and all(torch.equal(bits(x), bits(y)) for x, y in zip(flat(a), flat(b)))


def pool_facts(fin):
    """(images done, the step each was done at, the sets of lengths in the pools) of a final snapshot."""
    s = fin["state"]
    lens = [sorted(set(s["pool_len"][i, :int(s["pool_n"][i])].tolist())) for i in range(s["pool_n"].shape[0])]
    return s["done"].tolist(), s["end_step"].tolist(), lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_by_step_on_the_engines_own_snapshots(kind, dtype, images, monkeypatch):
    model = build(kind, images, dtype)
    args = model_args(kind, images)
    steps, finals = snapshots(monkeypatch)
    early = mixed = 0
    for lp, mode in ((0.0, True), (0.0, False), (1.0, True), (1.0, False)):
        del steps[:], finals[:]
        with torch.no_grad():
            beams = model.generate_batch(*args, return_beams=True, length_penalty=lp, early_stopping=mode, **KW)
        assert len(steps) == MAX_LEN + (0 if "LSTM" in kind else 1) and len(finals) == 1
        assert check_steps(steps, lp, mode, MAX_LEN) == MAX_LEN
        same_captions(beams, finals[0])
        s = beams.scores.cpu()
        assert beams.drawn.tolist() == [0] * N_IMG and bool((s[:, :-1] >= s[:, 1:]).all()) and torch.equal(beams.row_lengths, beams.lengths[:, 0])
        done, end, lens = pool_facts(finals[0])
        print(f"{kind} {dtype} penalty {lp} early_stopping={mode}: done {done} at {end}, pool lengths {lens}, lengths {beams.lengths.cpu().tolist()}")
        early += any(d and e < MAX_LEN - 1 for d, e in zip(done, end))
        mixed += any(len(x) >= 2 for x in lens)
        for i in range(N_IMG):                                               # a pooled hypothesis ends in its own <eos>
            for j in range(BEAM):
                if int(beams.beam_index[i, j]) < 0:
                    ln = int(beams.lengths[i, j])
                    assert int(beams.tokens[i, j, ln - 1]) == EOS and bool((beams.tokens[i, j, ln:] == finals[0]["pad_index"]).all())
    assert early == 4, "no image was done before the last position"         # conditions, not tolerances: see EOS_MARGIN
    assert mixed == 4, "no pool held two different lengths"
    with torch.no_grad():                                                    # no noise anywhere: another seed, generator, streams -- the same bits
        again = model.generate_batch(*args, return_beams=True, length_penalty=1.0, early_stopping=False, seed=7, rng="torch", **KW)
        third = model.generate_batch(*args, return_beams=True, length_penalty=1.0, early_stopping=False, seed=11, rng="philox", streams=2, **KW)
        pair = model.generate_batch(*args, length_penalty=1.0, early_stopping=False, **KW)
    assert same(beams, again) and same(beams, third)
    assert torch.equal(pair[0], beams.tokens[:, 0]) and torch.equal(pair[1], beams.lengths[:, 0])


# ---- 3. where no beam meets <eos> it is today's search ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_without_eos_both_modes_return_the_plain_search(kind, images):
    model = build(kind, images, boosted=False)
    args = model_args(kind, images)
    for lp in (0.0, 1.0):
        with torch.no_grad():
            want = model.generate_batch(*args, return_beams=True, length_penalty=lp, **KW)
            want_pair = model.generate_batch(*args, length_penalty=lp, **KW)
        assert not bool((want.tokens == EOS).any())
        for mode in (True, False):
            with torch.no_grad():
                got = model.generate_batch(*args, return_beams=True, length_penalty=lp, early_stopping=mode, **KW)
                pair = model.generate_batch(*args, length_penalty=lp, early_stopping=mode, **KW)
            assert same(got, want), (lp, mode)                                # tokens, lengths, scores, beam_index, drawn, row_lengths
            assert same(pair, want_pair), (lp, mode)


# ---- 4. None is the call without the keyword ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_none_is_the_call_without_the_keyword(kind, images, monkeypatch):
    from deephumor_amd import hip
    model = build(kind, images)
    args = model_args(kind, images)
    names = []
    real = hip._launch

    def launch(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", launch)
    runs = {}
    for tag, extra in (("beam", dict(search="beam")), ("beam none", dict(search="beam", early_stopping=None)),
                       ("norm", dict(search="beam", length_penalty=1.0)), ("norm none", dict(search="beam", length_penalty=1.0, early_stopping=None)),
                       ("pool", dict(search="beam", early_stopping=True)), ("sample", {}), ("sample none", dict(early_stopping=None))):
        del names[:]
        with torch.no_grad():
            out = model.generate_batch(*args, return_beams=True, max_len=MAX_LEN, beam_size=BEAM, top_k=20, seed=1, **extra)
        runs[tag] = (out, list(names))
    for a, b in (("beam", "beam none"), ("norm", "norm none"), ("sample", "sample none")):
        assert same(runs[a][0], runs[b][0]) and runs[a][1] == runs[b][1]
        assert "dh_beam_select_pool" not in runs[a][1] and "dh_beam_finalize_pool" not in runs[a][1]
    swap = {"dh_beam_select_best": "dh_beam_select_pool", "dh_beam_finalize_beams": "dh_beam_finalize_pool"}
    assert runs["pool"][1] == [swap.get(n, n) for n in runs["beam"][1]]
    assert runs["pool"][1].count("dh_beam_select_pool") == MAX_LEN and runs["pool"][1].count("dh_beam_finalize_pool") == 1


# ---- 5. the carriers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graphed_and_pipeline(kind, images):
    from deephumor_amd.pipeline import CaptionPipeline
    from deephumor_amd.models import beam as B
    model = build(kind, images, torch.bfloat16)
    args = model_args(kind, images)
    combos = ((0.0, True), (1.0, False))
    with torch.no_grad():
        eager = {c: model.generate_batch(*args, return_beams=True, length_penalty=c[0], early_stopping=c[1], **KW) for c in combos}
        pair = model.generate_batch(*args, early_stopping=True, **KW)
        for _ in range(2):                                                   # capture, then replay
            for c in combos:
                g = model.generate_batch_graphed(*args, return_beams=True, length_penalty=c[0], early_stopping=c[1], seed=3, **KW)
                assert same(g, eager[c]), c
        plain = model.generate_batch_graphed(*args, return_beams=True, early_stopping=None, **KW)
        assert same(plain, model.generate_batch(*args, return_beams=True, **KW))
    keys = sorted(str(dict(k[2]).get("early_stopping")) for k in model._graphs)
    assert keys == ["False", "None", "True"]                                 # None is the graph of the call without the keyword
    ones = B._LEN_W_CACHE[(str(args[0].device), 0.0, MAX_LEN)]
    state = [v for k, v in model._graphs.items() if dict(k[2]).get("early_stopping") is True][0]
    assert any(t is ones for t in state[8])                                  # the graph's state holds the table of ones its nodes read
    assert torch.equal(pair[0], eager[combos[0]].tokens[:, 0]) and torch.equal(pair[1], eager[combos[0]].row_lengths)
    batches = [(images[:2],), (images[2:],)]
    got = [tuple(t.clone() for t in r) for r in CaptionPipeline(model, early_stopping=True, **KW).run(batches)]
    assert torch.equal(torch.cat([g[0] for g in got]).cpu(), pair[0].cpu()) and torch.equal(torch.cat([g[1] for g in got]).cpu(), pair[1].cpu())


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
with torch.no_grad():
    model.decoder.classifier.bias[3] += 8.0
images = synth_images(4, seed=0).to(dev)
kw = dict(max_len=10, beam_size=3, top_k=20, search="beam", length_penalty=1.0, early_stopping=False)
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, **kw)
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 2, always=True) for a in (0, 2)]
    got = tuple(torch.cat(ts, 0) for ts in zip(*halves))
    micro = generate_micro_sharded(fn, 4, 2, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want),
                              "eos": bool((want[0] == 3).any())}))
dist.barrier()
dist.destroy_process_group()
"""


def test_sharded_through_the_one_rank_group_equals_the_plain_call():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True, "eos": True}


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformerWithLabels"))
def test_composes_with_prompts_bans_and_edits(kind, images, monkeypatch):
    """Prompts of unequal lengths, ``min_len`` and ``no_repeat_ngram_size`` with the pool: every select and the finalize are the
    restatement's, an image counts its length from its own first column, no pooled hypothesis is shorter than ``min_len`` allows."""
    model = build(kind, images, margin=-1.0)
    args = model_args(kind, images)
    cap = torch.randint(6, 1000, (N_IMG, 3), generator=torch.Generator().manual_seed(2)).cuda()
    lens = [0, 2, 1, 3]
    extra = dict(caption=cap, caption_lengths=torch.tensor(lens), min_len=5, no_repeat_ngram_size=2, length_penalty=1.0, early_stopping=False)
    steps, finals = snapshots(monkeypatch)
    with torch.no_grad():
        beams = model.generate_batch(*args, return_beams=True, **KW, **extra)
    assert check_steps(steps, 1.0, False, MAX_LEN) == MAX_LEN and all(rec["first_pos"] == lens for rec in steps)
    same_captions(beams, finals[0])
    done, end, pooled = pool_facts(finals[0])
    print(f"{kind}: done {done} at {end}, pool lengths {pooled}")
    for i, n in enumerate(lens):
        assert beams.tokens[i, :, :n].tolist() == [cap[i, :n].tolist()] * BEAM
        for j in range(BEAM):
            if torch.isfinite(beams.scores[i, j]):
                row, ln = beams.tokens[i, j].tolist(), int(beams.lengths[i, j])
                assert EOS not in row[n:5] and ln >= 5 + 1                    # min_len held
                grams = [tuple(row[c:c + 2]) for c in range(ln - 1)]
                assert all(grams.index(gr) == c or c + 2 <= n for c, gr in enumerate(grams))               # no generated bigram repeats
    del steps[:], finals[:]
    with torch.no_grad():
        plain = model.generate_batch(*args, **KW, **extra)
    assert torch.equal(plain[0], beams.tokens[:, 0]) and torch.equal(plain[1], beams.row_lengths)


# ---- 6. the host loop ends early ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_early_stop_every_ends_the_host_loop_and_changes_nothing(kind, images, monkeypatch):
    model = build(kind, images, margin=EARLY_MARGIN)
    args = model_args(kind, images)
    steps, finals = snapshots(monkeypatch)
    with torch.no_grad():
        want = model.generate_batch(*args, return_beams=True, early_stopping=True, **KW)
    full, fin = len(steps), finals[0]
    done, end, _ = pool_facts(fin)
    del steps[:], finals[:]
    with torch.no_grad():
        got = model.generate_batch(*args, return_beams=True, early_stopping=True, early_stop_every=1, **KW)
    print(f"{kind}: done {done} at {end}; {full} steps without the poll, {len(steps)} with it")
    assert all(done) and full >= MAX_LEN
    # the loop ended behind the step that finished the last image (the poll runs from the second position on)
    assert len(steps) == max(max(end), 1) + 1 < MAX_LEN
    assert same(got, want)
