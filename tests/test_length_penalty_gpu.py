"""``search="beam"`` with ``length_penalty`` on a real MI355X: ``dh_beam_select_best_norm`` against the torch-CPU restatement
(``tests/length_penalty_ref.py``) bit for bit on every output tensor, ``generate_batch`` end to end -- every select and the final order
replayed on the engine's own snapshots, bit for bit --, the log-prob identity, the unchanged default, and every carrier of the keyword.

The models are the synthetic ones of ``helpers.synthetic_sd`` with the classifier's ``<eos>`` bias raised until ``<eos>`` stands half a
logit below a row's best token at the position where it comes closest (measured once per kind on the logits of a search with the
plain weights): beams then end at different lengths, which is where a length penalty has something to decide.  Nothing here is compared within a tolerance: the select's inputs are the engine's own
``pick_idx`` / ``pick_val``, and one fp32 add and one fp32 multiply have one answer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_search_ref as R  # noqa: E402
import length_penalty_ref as LP  # noqa: E402
from helpers import KINDS, captions_and_lengths, synthetic_sd, synth_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")
UNK, EOS = 1, 3
FIELDS = ("tokens", "vals", "keys", "ended", "src", "parent", "hparent", "done", "end_step")


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


# ---- 1. dh_beam_select_best_norm against the restatement, bit for bit --------------------------------------------------------------
N_SEL, TOK_LD, V_SEL = 6, 12, 40


def random_state(beam, with_src, seed, len_w, write_pos, first_cols, first, tie_img):
    """A mid-search state of 6 images: live beams and beams that ended at different lengths -- each carrying ``score * w[L_end]`` for
    its OWN ``L_end``, so a recomputation at the step's ``L`` would give another key --, dead beams at ``-inf``, quarter-valued scores
    (many equal candidates), image 1 with every beam ended (it finishes in this step), image 2 already done."""
    g = torch.Generator().manual_seed(seed)
    r = N_SEL * beam
    st = LP.new_state(N_SEL, beam, TOK_LD, src_len=TOK_LD + 1 if with_src else 0)
    st.tokens = torch.randint(4, V_SEL, (r, TOK_LD), generator=g, dtype=torch.int32)
    st.vals = torch.randint(-12, 0, (r,), generator=g).float() * 0.25
    st.ended = (torch.rand(r, generator=g) < 0.3).to(torch.uint8)
    st.vals[torch.rand(r, generator=g) < 0.15] = NINF
    if with_src:
        st.src = (torch.randint(0, beam, (r, TOK_LD + 1), generator=g, dtype=torch.int32)
                  + (torch.arange(r, dtype=torch.int32) // beam * beam)[:, None])
    st.parent = torch.full((r,), -5, dtype=torch.int32)
    st.hparent = torch.full((r,), -5, dtype=torch.int32)
    st.done[2], st.end_step[2] = 1, 1
    st.ended[beam:2 * beam] = 1
    for row in range(r):                                                     # the keys the beams were kept with
        cur = max(write_pos - first_cols[row // beam], 1)                    # columns written before this step (at least the first)
        ln = int(torch.randint(1, cur + 1, (), generator=g)) if st.ended[row] else cur
        st.keys[row] = float(LP.key_of(st.vals[row].item(), len_w[ln]))
    pick_idx = torch.randint(0, V_SEL, (r, beam), generator=g, dtype=torch.int32)
    pick_idx[torch.rand(r, beam, generator=g) < 0.2] = EOS
    pick_val = torch.sort(torch.randint(-8, 0, (r, beam), generator=g).float() * 0.25, dim=1, descending=True).values
    pick_val[torch.rand(r, beam, generator=g) < 0.1] = NINF                  # what a TOO_FEW row leaves: token 0 at -inf
    if first:
        st.vals.zero_()
        st.keys.zero_()
        st.ended.zero_()
        st.done.zero_()
    elif tie_img is not None and beam >= 2:
        # an image at L = 4 under penalty 1 (w = 0.25): beam 0 ended at L = 1 with score -1 (key -1), beam 1 live at -3 with a pick at -1
        # (score -4, key -1): different scores, the same key -- the lower candidate index must win
        r0 = tie_img * beam
        st.ended[r0], st.vals[r0], st.keys[r0] = 1, -1.0, -1.0
        st.ended[r0 + 1], st.vals[r0 + 1] = 0, -3.0
        pick_val[r0 + 1, 0] = -1.0
    return st, pick_idx, pick_val


def run_select(h, st, pick_idx, pick_val, first, write_pos, t, step, len_w, first_col, first_pos):
    dev = {k: None if getattr(st, k) is None else getattr(st, k).clone().cuda() for k in FIELDS}
    fp = None if first_pos is None else torch.tensor(first_pos, dtype=torch.int32, device="cuda")
    guard = torch.full((64,), 77.0, device="cuda")                           # behind the table: the clamp keeps the kernel inside it
    table = torch.cat([len_w.cuda(), guard])[:len_w.numel()]
    h.beam_select_best_norm(pick_idx.cuda(), pick_val.cuda(), dev["tokens"], dev["vals"], dev["keys"], dev["ended"], dev["src"], dev["parent"],
                            dev["hparent"], dev["done"], dev["end_step"], st.n_img, st.beam, first, True, write_pos, t, step, EOS, table,
                            first_col=first_col, first_pos=fp)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in dev.items()}


#         first  write_pos  first_col  first_pos (prompted: one image still forced, one at its first step, the rest at their own L)
CASES = [(True, 0, 0, None), (True, 3, 3, None), (False, 3, 0, None), (False, 6, 3, None), (False, TOK_LD - 1, 0, None),
         (False, 4, 0, [6, 4, 0, 2, 3, 1]), (False, 9, 0, [10, 9, 0, 6, 8, 2])]


@pytest.mark.parametrize("with_src", (False, True), ids=("lstm", "src"))
@pytest.mark.parametrize("beam", (1, 2, 5, 16, 17, 64))
def test_select_best_norm_is_the_restatement_bit_for_bit(hip, beam, with_src):
    t = 3
    ties = 0
    for lp in (-1.0, 0.5, 1.0, 2.0):
        len_w = LP.weights(lp, TOK_LD)
        for case, (first, write_pos, first_col, first_pos) in enumerate(CASES):
            cols = first_pos if first_pos is not None else [first_col] * N_SEL
            at_four = [i for i in range(N_SEL) if i not in (1, 2) and write_pos + 1 - cols[i] == 4]
            tie_img = at_four[0] if lp == 1.0 and not first and at_four else None
            st, pick_idx, pick_val = random_state(beam, with_src, 1000 * beam + 10 * case + int(lp * 4), len_w, write_pos, cols, first, tie_img)
            before = {k: None if getattr(st, k) is None else getattr(st, k).clone() for k in FIELDS}
            got = run_select(hip, st, pick_idx, pick_val, first, write_pos, t, write_pos, len_w, first_col, first_pos)
            LP.select_best_norm(st, pick_idx, pick_val, first, write_pos, t, write_pos, EOS, len_w, first_col=first_col, first_pos=first_pos)
            same_state(got, st, (lp, case))
            if first_pos is not None:                                        # the forced image kept its scores and its keys
                assert torch.equal(st.keys[:beam], before["keys"][:beam]) and torch.equal(st.vals[:beam], before["vals"][:beam])
            if not first:                                                    # the done image is frozen; image 1 has finished
                assert all(torch.equal(bits(getattr(st, k))[2 * beam:3 * beam], bits(before[k])[2 * beam:3 * beam]) for k in ("tokens", "vals", "keys"))
                assert first_pos is not None or (st.done[1] == 1 and st.end_step[1] == write_pos)
            if tie_img is not None and beam == 2:                            # two beams: the tied pair is what stays, the ended beam in front
                r0 = tie_img * beam
                assert st.keys[r0:r0 + 2].tolist() == [-1.0, -1.0] and st.vals[r0:r0 + 2].tolist() == [-1.0, -4.0] and st.ended[r0] == 1
            ties += tie_img is not None
    assert ties == 4                                                         # two dense and two prompted steps carried the planted tie


def test_equal_keys_go_to_the_lower_candidate_index(hip):
    """The hand-worked tie of tests/test_length_penalty_cpu.py on the device: penalty 1, L = 2 -- [5, 6] at score -2 and the beam that
    ended at L = 1 at score -1 both have key -1; whichever stands first in the candidate list stays in front."""
    w = LP.weights(1.0, 3)
    for ended_first in (False, True):
        st = LP.new_state(1, 2, 3)
        first = ([EOS, 5], [-1.0, -1.5]) if ended_first else ([5, EOS], [-1.5, -1.0])
        pi, pv = torch.tensor([first[0], [0, 0]], dtype=torch.int32), torch.tensor([first[1], [0.0, 0.0]])
        got = run_select(hip, st, pi, pv, True, 0, 0, 0, w, 0, None)
        for k in FIELDS:
            if got[k] is not None:
                setattr(st, k, got[k])
        got = run_select(hip, st, torch.tensor([[6, 7], [6, 7]], dtype=torch.int32), torch.tensor([[-0.5, -1.0], [-0.5, -1.0]]), False, 1, 0, 1,
                         w, 0, None)
        assert got["keys"].tolist() == [-1.0, -1.0] and got["parent"].tolist() == [0, 1]
        assert got["tokens"][:, :2].tolist() == ([[EOS, 0], [5, 6]] if ended_first else [[5, 6], [EOS, 0]])
        assert got["vals"].tolist() == ([-1.0, -2.0] if ended_first else [-2.0, -1.0])


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


def build(kind, images, dtype=torch.float32, boosted=True):
    """The synthetic model of ``kind``; ``boosted``: with ``<eos>`` half a logit below the rows' best token at the position where the
    median distance between the two is smallest."""
    if kind not in _sds:
        sd, hp = synthetic_sd(kind)
        seen = []
        with torch.no_grad():
            load(kind, sd, hp).generate_batch(*model_args(kind, images), logits_hook=lambda pos, lg: seen.append(lg.float().cpu().clone()), **KW)
        gap = min(float((x.max(1).values - x[:, EOS]).median()) for x in seen)
        bias = [k for k in sd if "classifier" in k and k.endswith("bias") and sd[k].shape[0] == hp["num_tokens"]]
        assert len(bias) == 1
        up = {k: v.clone() for k, v in sd.items()}
        up[bias[0]][EOS] += gap - 0.5
        _sds[kind] = (sd, up, hp)
    sd, up, hp = _sds[kind]
    return load(kind, up if boosted else sd, hp, dtype)


def snapshots(monkeypatch):
    """Every beam step and the final step of the calls made from now on: the engine's state in front of and behind each, and the
    picks the row step left (the select does not write them)."""
    from deephumor_amd.models.beam import BeamSearchHelper
    steps, finals = [], []
    real_step, real_final = BeamSearchHelper._draw_and_select, BeamSearchHelper.finalize
    c = lambda t: None if t is None else t.detach().cpu().clone()

    def state_of(h):
        return dict(tokens=c(h.tokens), vals=c(h.vals), keys=c(h.keys), ended=c(h._ended), done=c(h.done), end_step=c(h.end_step), src=c(h.src),
                    parent=c(h.parent), hparent=c(h.hparent))

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        rec = dict(first=first, write_pos=write_pos, t=t, step=step_index, before=state_of(self), beam=self.beam_size, eos=self.eos_index,
                   first_pos=None if self.first_pos is None else self.first_pos.cpu().tolist())
        real_step(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted)
        rec.update(after=state_of(self), pick_idx=c(self.pick_idx), pick_val=c(self.pick_val), first_col=self.first_col, len_w=c(self.len_w))
        steps.append(rec)

    def final(self, len_bias_done, full_len, pad_index=0, **kw):
        finals.append(dict(state=state_of(self), len_bias_done=len_bias_done, full_len=full_len, pad_index=pad_index, pos=kw.get("pos", 0),
                           first_pos=None if self.first_pos is None else self.first_pos.cpu().tolist(), beam=self.beam_size, eos=self.eos_index))
        return real_final(self, len_bias_done, full_len, pad_index, **kw)
    monkeypatch.setattr(BeamSearchHelper, "_draw_and_select", step)
    monkeypatch.setattr(BeamSearchHelper, "finalize", final)
    return steps, finals


def state_from(snap, beam):
    st = R.State.of(snap["tokens"], snap["vals"], snap["ended"], snap["done"], snap["end_step"], beam, snap["src"], snap["parent"], snap["hparent"])
    st.keys = snap["keys"].clone()
    return st


def check_steps(steps, length_penalty, max_len):
    """The restatement applied to every snapshot, with the engine's own picks, gives the next snapshot bit for bit."""
    moved = 0
    for rec in steps:
        assert torch.equal(rec["len_w"], LP.weights(length_penalty, max_len))
        if rec["write_pos"] >= rec["before"]["tokens"].shape[1]:             # the Transformer decoders' last step writes no token: skipped
            st = state_from(rec["before"], rec["beam"])
        else:
            st = state_from(rec["before"], rec["beam"])
            LP.select_best_norm(st, rec["pick_idx"], rec["pick_val"], rec["first"], rec["write_pos"], rec["t"], rec["step"], rec["eos"],
                                rec["len_w"], first_col=rec["first_col"], first_pos=rec["first_pos"])
            moved += 1
        same_state(rec["after"], st, rec["step"])
    return moved


def same_captions(beams, fin):
    want = LP.finalize_norm(state_from(fin["state"], fin["beam"]), fin["len_bias_done"], fin["full_len"], fin["pad_index"], fin["eos"],
                            fin["pos"], fin["first_pos"])
    for k in ("tokens", "lengths", "beam_index", "drawn", "row_lengths"):
        assert torch.equal(getattr(beams, k).cpu(), want[k]), k
    assert torch.equal(bits(beams.scores.cpu()), bits(want["scores"]))


def sorted_desc(scores):
    s = torch.where(torch.isinf(scores), torch.full_like(scores, -3e38), scores)
    return bool((s[:, :-1] >= s[:, 1:]).all())


def same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    flat = lambda xs: [t for x in xs for t in (x if isinstance(x, tuple) else (x,))]
    return len(flat(a)) == len(flat(b)) and all(torch.equal(bits(x), bits(y)) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_by_step_on_the_engines_own_snapshots(kind, dtype, images, monkeypatch):
    model = build(kind, images, dtype)
    args = model_args(kind, images)
    steps, finals = snapshots(monkeypatch)
    with torch.no_grad():
        zero = model.generate_batch(*args, return_beams=True, **KW)
    del steps[:], finals[:]
    changed = ended_early = 0
    for lp in (1.0, -0.75):
        with torch.no_grad():
            beams = model.generate_batch(*args, return_beams=True, length_penalty=lp, **KW)
        assert len(steps) == MAX_LEN + (0 if "LSTM" in kind else 1) and len(finals) == 1
        assert check_steps(steps, lp, MAX_LEN) == MAX_LEN
        same_captions(beams, finals[0])
        assert beams.drawn.tolist() == [0] * N_IMG and sorted_desc(beams.scores.cpu())
        lengths = beams.lengths.cpu().flatten().tolist()
        print(f"{kind} {dtype} penalty {lp}: lengths {beams.lengths.cpu().tolist()}, slot 0 differs from penalty 0 in "
              f"{int((beams.tokens[:, 0] != zero.tokens[:, 0]).any(-1).sum())} of {N_IMG} images")
        ended_early += min(lengths) < MAX_LEN and len(set(lengths)) > 1
        changed += int((beams.tokens != zero.tokens).any())
        del steps[:], finals[:]
        with torch.no_grad():                                               # no noise anywhere: another seed, another generator, the same bits
            again = model.generate_batch(*args, return_beams=True, length_penalty=lp, seed=7, rng="torch", **KW)
            third = model.generate_batch(*args, return_beams=True, length_penalty=lp, seed=11, rng="philox", streams=2, **KW)
        assert same(beams, again) and same(beams, third)
        del steps[:], finals[:]
    print(f"{kind} {dtype}: the kept beams differ from penalty 0 under {changed} of 2 penalties")
    assert ended_early > 0                               # beams ended at different lengths: carried keys stood against recomputed ones


# ---- 3. the log-prob identity -------------------------------------------------------------------------------------------------------
def first_eos_length(row, first, width):
    """Columns from ``first`` through the row's own first ``<eos>`` at or behind it, inclusive; up to ``width`` without one."""
    hits = [c for c in range(first, width) if int(row[c]) == EOS]
    return (hits[0] + 1 if hits else width) - first


@pytest.mark.parametrize("kind", KINDS)
def test_logprobs_times_the_weight_of_the_length_are_the_scores(kind, images, monkeypatch):
    """``return_logprobs=True`` on the ``<eos>``-boosted weights, dense, behind a prefix and prompted.  For EVERY live beam the score is
    the engine's raw cumulative log-probability times ``w[L]``, one fp32 multiply, with ``L`` counted on the engine's own token row
    (from the image's first generated column through the beam's first ``<eos>``).  Wherever the returned row holds all of those
    columns, ``L`` is ``lengths - first generated column`` and the fp32 left-to-right sum of the returned log-probabilities over the
    beam's own columns IS that raw score, so ``sum * w[lengths - first]`` is the score bit for bit.  The one place it does not: a
    Transformer image whose beams have ALL ended returns its rows without the last ``<eos>`` column (``len_bias_done = 0``, the
    reference's convention, with or without a penalty), so the beam that ended last has ``lengths`` one below its ``L``; there the
    difference must be exactly that one column."""
    model = build(kind, images)
    args = model_args(kind, images)
    cap = torch.randint(6, 1000, (N_IMG, 3), generator=torch.Generator().manual_seed(2)).cuda()
    lens = [0, 2, 1, 3]
    w = LP.weights(1.0, MAX_LEN).numpy()
    steps, finals = snapshots(monkeypatch)
    live = ended_early = summed = cut = 0
    for name, extra, first in (("plain", {}, [0] * N_IMG), ("prefix", dict(caption=cap), [3] * N_IMG),
                               ("prompted", dict(caption=cap, caption_lengths=torch.tensor(lens)), lens)):
        del steps[:], finals[:]
        with torch.no_grad():
            beams, lp = model.generate_batch(*args, return_beams=True, return_logprobs=True, length_penalty=1.0, **KW, **extra)
        assert len(finals) == 1
        state = finals[0]["state"]
        scores, lengths, vals = beams.scores.cpu().numpy(), beams.lengths.cpu(), lp.cpu().numpy()
        index = beams.beam_index.cpu()
        for i in range(N_IMG):
            for j in range(BEAM):
                if not np.isfinite(scores[i, j]):
                    continue
                live += 1
                row = i * BEAM + int(index[i, j])
                n_cols = first_eos_length(state["tokens"][row], first[i], MAX_LEN)          # the engine's own L
                raw = state["vals"][row].numpy()
                assert np.float32(raw * w[n_cols]).tobytes() == scores[i, j].tobytes(), (name, i, j)
                acc = np.float32(0.0)
                for c in range(first[i], int(lengths[i, j])):
                    acc = np.float32(acc + vals[i, j, c])
                shown = int(lengths[i, j]) - first[i]
                if shown == n_cols:                                          # every column the search wrote is returned
                    assert acc.tobytes() == raw.tobytes(), (name, i, j)
                    assert np.float32(acc * w[shown]).tobytes() == scores[i, j].tobytes(), (name, i, j, float(acc), float(scores[i, j]))
                    summed += 1
                else:                                                        # the finished Transformer image's last <eos> column
                    assert "LSTM" not in kind and bool(state["done"][i]) and shown == n_cols - 1, (name, i, j, shown, n_cols)
                    assert int(lengths[i, j]) == int(beams.row_lengths[i]) and int(state["tokens"][row, int(lengths[i, j])]) == EOS
                    cut += 1
                ended_early += n_cols < MAX_LEN - first[i]
    print(f"{kind}: {live} live beams, {summed} summed over all their columns, {cut} cut by one column, {ended_early} ended early")
    assert live > 0.9 * 3 * N_IMG * BEAM and ended_early > 0 and summed > 0.5 * live


# ---- 4. the default is unchanged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_zero_is_the_call_without_the_keyword(kind, images, monkeypatch):
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
    for tag, extra in (("beam", dict(search="beam")), ("beam 0", dict(search="beam", length_penalty=0.0)),
                       ("beam 1", dict(search="beam", length_penalty=1.0)), ("sample", {}), ("sample 0", dict(length_penalty=0))):
        del names[:]
        with torch.no_grad():
            out = model.generate_batch(*args, return_beams=True, max_len=MAX_LEN, beam_size=BEAM, top_k=20, seed=1, **extra)
        runs[tag] = (out, list(names))
    assert same(runs["beam"][0], runs["beam 0"][0]) and runs["beam"][1] == runs["beam 0"][1]
    assert same(runs["sample"][0], runs["sample 0"][0]) and runs["sample"][1] == runs["sample 0"][1]
    assert "dh_beam_select_best_norm" not in runs["beam"][1] + runs["sample"][1] and "dh_beam_select_best" not in runs["beam 1"][1]
    assert runs["beam 1"][1] == ["dh_beam_select_best_norm" if n == "dh_beam_select_best" else n for n in runs["beam"][1]]
    assert runs["beam 1"][1].count("dh_beam_select_best_norm") == MAX_LEN


# ---- 5. the carriers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graphed_and_pipeline(kind, images):
    from deephumor_amd.pipeline import CaptionPipeline
    model = build(kind, images, torch.bfloat16)
    args = model_args(kind, images)
    with torch.no_grad():
        eager = {lp: model.generate_batch(*args, return_beams=True, length_penalty=lp, **KW) for lp in (0.0, 1.0)}
        pair = model.generate_batch(*args, length_penalty=1.0, **KW)
        for _ in range(2):                                                   # capture, then replay
            for lp in (0.0, 1.0):
                g = model.generate_batch_graphed(*args, return_beams=True, length_penalty=lp, seed=3, **KW)
                assert same(g, eager[lp]), lp
        assert same(model.generate_batch_graphed(*args, return_beams=True, **KW), eager[0.0])
    keys = [dict(k[2]).get("length_penalty") for k in model._graphs]
    assert sorted(keys, key=str) == [1.0, None]                              # two graphs: 0.0 is the graph of the call without the keyword
    # the captured nodes point at the weight table: the graph's state owns it, so a cache that has moved on cannot free it
    from deephumor_amd.models import beam as B
    state = [v for k, v in model._graphs.items() if dict(k[2]).get("length_penalty") == 1.0][0]
    table = B._LEN_W_CACHE[(str(args[0].device), 1.0, MAX_LEN)]
    assert any(t is table for t in state[8]) and all(v[8] == () for k, v in model._graphs.items() if "length_penalty" not in dict(k[2]))
    for n in range(B._LEN_W_CACHE_SIZE + 1):
        B.compile_length_weights(0.25, 40 + n, args[0].device)
    assert (str(args[0].device), 1.0, MAX_LEN) not in B._LEN_W_CACHE and any(t is table for t in state[8])
    del table
    with torch.no_grad():
        assert same(model.generate_batch_graphed(*args, return_beams=True, length_penalty=1.0, seed=5, **KW), eager[1.0])      # a replay
    assert len(model._graphs) == 2
    assert torch.equal(pair[0], eager[1.0].tokens[:, 0]) and torch.equal(pair[1], eager[1.0].row_lengths)
    batches = [(images[:2],), (images[2:],)]
    got = [tuple(t.clone() for t in r) for r in CaptionPipeline(model, length_penalty=1.0, **KW).run(batches)]
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
    model.decoder.classifier.bias[3] += 4.0
images = synth_images(4, seed=0).to(dev)
kw = dict(max_len=10, beam_size=3, top_k=20, search="beam", length_penalty=1.0)
fn = lambda lo, hi: model.generate_batch(images[lo:hi], img0=lo, **kw)
with torch.no_grad():
    want = model.generate_batch(images, **kw)
    halves = [generate_sharded(lambda lo, hi, a=a: fn(a + lo, a + hi), 2, always=True) for a in (0, 2)]
    got = tuple(torch.cat(ts, 0) for ts in zip(*halves))
    micro = generate_micro_sharded(fn, 4, 2, always=True)
same = lambda x, y: all(bool(torch.equal(a, b)) for a, b in zip(x, y))
print("RESULT " + json.dumps({"backend": dist.get_backend(), "halves": same(got, want), "micro": same(micro, want)}))
dist.barrier()
dist.destroy_process_group()
"""


def test_sharded_through_the_one_rank_group_equals_the_plain_call():
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True}


@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningTransformerWithLabels"))
def test_composes_with_prompts_bans_edits_and_attention(kind, images, monkeypatch):
    """Prompts of unequal lengths, ``min_len``, ``no_repeat_ngram_size`` and ``return_attention`` with the penalty: every select and the
    final order are the restatement's (so the tokens are), an image counts its length from its own first column, and the attention rows
    below each beam's length sum to 1."""
    model = build(kind, images)
    args = model_args(kind, images)
    cap = torch.randint(6, 1000, (N_IMG, 3), generator=torch.Generator().manual_seed(2)).cuda()
    lens = [0, 2, 1, 3]
    extra = dict(caption=cap, caption_lengths=torch.tensor(lens), min_len=5, no_repeat_ngram_size=2, length_penalty=1.0)
    steps, finals = snapshots(monkeypatch)
    with torch.no_grad():
        beams, att = model.generate_batch(*args, return_beams=True, return_attention=True, **KW, **extra)
    assert check_steps(steps, 1.0, MAX_LEN) == MAX_LEN and all(rec["first_pos"] == lens for rec in steps)
    same_captions(beams, finals[0])
    for i, n in enumerate(lens):
        assert beams.tokens[i, :, :n].tolist() == [cap[i, :n].tolist()] * BEAM
        for j in range(BEAM):
            if torch.isfinite(beams.scores[i, j]):
                row, ln = beams.tokens[i, j].tolist(), int(beams.lengths[i, j])
                assert EOS not in row[n:5] and ln >= min(5 + 1, int(beams.row_lengths[i]))                 # min_len held
                grams = [tuple(row[c:c + 2]) for c in range(ln - 1)]
                assert all(grams.index(gr) == c or c + 2 <= n for c, gr in enumerate(grams))               # no generated bigram repeats
    sums = att.sum(-1).cpu()
    for i in range(N_IMG):
        for j in range(BEAM):
            n = int(beams.lengths[i, j])
            assert torch.allclose(sums[i, j, :n], torch.ones(n), atol=1e-5) and bool((att[i, j, n:] == 0).all())
    del steps[:], finals[:]
    with torch.no_grad():
        plain = model.generate_batch(*args, **KW, **extra)
    assert torch.equal(plain[0], beams.tokens[:, 0]) and torch.equal(plain[1], beams.row_lengths)
