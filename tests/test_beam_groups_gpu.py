"""``search="beam"`` with ``num_beam_groups`` / ``diversity_penalty`` on a real MI355X: ``dh_beam_select_groups`` against the torch-CPU
restatement (``tests/beam_groups_ref.py``) bit for bit on every state tensor, ``generate_batch`` end to end -- every select and the final
order replayed on the engine's own snapshots, bit for bit --, the log-prob identity, the attention rows, the unchanged default, every
carrier of the keywords, and ``experiments.group_best``.

The models, the ``<eos>`` boost and the snapshot machinery are those of ``test_length_penalty_gpu.py`` (one calibration per kind for both
files).  Nothing here is compared within a tolerance: the select's inputs are the engine's own ``pick_idx`` / ``pick_val``, and one fp32
add, one multiply by ``w[L]`` and the two rounded operations of the penalty have one answer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_groups_ref as GR  # noqa: E402
import length_penalty_ref as LP  # noqa: E402
import test_length_penalty_gpu as T  # noqa: E402
from helpers import KINDS  # noqa: E402

NINF = float("-inf")
UNK, EOS = 1, 3
FIELDS = T.FIELDS
bits, same, same_state = T.bits, T.same, T.same_state


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


@pytest.fixture(scope="module")
def images():
    return T.synth_images(T.N_IMG, seed=0)


# ---- 1. dh_beam_select_groups against the restatement, bit for bit -------------------------------------------------------------------
N_SEL, TOK_LD = 3, 12
ALPHABET = torch.tensor([EOS, 4, 5, 6, 7, 8, 9, 10], dtype=torch.int32)      # eight tokens: every step has collisions across groups


def random_state(beam, with_src, seed, len_w, write_pos, first_cols, first, done_img):
    """A mid-search state of 3 images: live beams, beams that ended earlier (each with the key of its OWN length), dead beams at
    ``-inf``, quarter-valued scores and picks (many equal candidates, before and behind the penalty), one row whose picks are all
    ``-inf`` and single ``-inf`` picks elsewhere (TOO_FEW), image ``done_img`` already done."""
    g = torch.Generator().manual_seed(seed)
    r = N_SEL * beam
    st = LP.new_state(N_SEL, beam, TOK_LD, src_len=TOK_LD + 1 if with_src else 0)
    st.tokens = torch.randint(4, 40, (r, TOK_LD), generator=g, dtype=torch.int32)
    st.vals = torch.randint(-12, 0, (r,), generator=g).float() * 0.25
    st.ended = (torch.rand(r, generator=g) < 0.3).to(torch.uint8)
    st.vals[torch.rand(r, generator=g) < 0.1] = NINF
    if with_src:
        st.src = (torch.randint(0, beam, (r, TOK_LD + 1), generator=g, dtype=torch.int32)
                  + (torch.arange(r, dtype=torch.int32) // beam * beam)[:, None])
    st.parent = torch.full((r,), -5, dtype=torch.int32)
    st.hparent = torch.full((r,), -5, dtype=torch.int32)
    if done_img is not None:
        st.done[done_img], st.end_step[done_img] = 1, 1
    for row in range(r):
        cur = max(write_pos - first_cols[row // beam], 1)
        ln = int(torch.randint(1, cur + 1, (), generator=g)) if st.ended[row] else cur
        st.keys[row] = float(LP.key_of(st.vals[row].item(), len_w[ln]))
    pick_idx = ALPHABET[torch.randint(0, len(ALPHABET), (r, beam), generator=g)]
    pick_val = torch.sort(torch.randint(-8, 0, (r, beam), generator=g).float() * 0.25, dim=1, descending=True).values
    pick_val[torch.rand(r, beam, generator=g) < 0.05] = NINF
    pick_val[r - 1] = NINF                                                    # the last row of the last image: nothing but -inf picks
    st.ended[r - 1] = 0
    if first:
        st.vals.zero_()
        st.keys.zero_()
        st.ended.zero_()
        st.done.zero_()
        pick_val[beam * (N_SEL - 1)] = NINF                                   # (a first step reads the base row's picks: that row then)
        pick_val[N_SEL - 1] = NINF                                            # (dense: flat row `img`)
    return st, pick_idx, pick_val


def run_select(h, st, pick_idx, pick_val, first, write_pos, t, step, len_w, first_col, first_pos, n_groups, lam):
    dev = {k: None if getattr(st, k) is None else getattr(st, k).clone().cuda() for k in FIELDS}
    fp = None if first_pos is None else torch.tensor(first_pos, dtype=torch.int32, device="cuda")
    h.beam_select_groups(pick_idx.cuda(), pick_val.cuda(), dev["tokens"], dev["vals"], dev["keys"], dev["ended"], dev["src"], dev["parent"],
                         dev["hparent"], dev["done"], dev["end_step"], st.n_img, st.beam, first, True, write_pos, t, step, EOS,
                         len_w.cuda(), first_col=first_col, first_pos=fp, n_groups=n_groups, diversity_penalty=lam)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in dev.items()}


#         first  write_pos  first_col  first_pos (prompted: one image still forced, one at its first step, one at its own L)
CASES = [(True, 0, 0, None), (True, 3, 3, None), (False, 3, 0, None), (False, 6, 3, None), (False, TOK_LD - 1, 0, None),
         (False, 4, 0, [6, 4, 1]), (False, 9, 0, [2, 10, 9])]


@pytest.mark.parametrize("with_src", (False, True), ids=("lstm", "src"))
@pytest.mark.parametrize("beam,groups", ((2, 2), (4, 2), (6, 3), (16, 4), (18, 3), (64, 2), (64, 64)))
def test_select_groups_is_the_restatement_bit_for_bit(hip, beam, groups, with_src):
    t = 3
    penalised = 0
    for lam, lp in ((0.5, 0.0), (1e6, 0.0), (0.5, 1.0)):
        len_w = LP.weights(lp, TOK_LD)
        for case, (first, write_pos, first_col, first_pos) in enumerate(CASES):
            cols = first_pos if first_pos is not None else [first_col] * N_SEL
            done_img = 0 if (not first and first_pos is None) else None
            st, pick_idx, pick_val = random_state(beam, with_src, 1000 * beam + 10 * case + groups, len_w, write_pos, cols, first, done_img)
            before = {k: None if getattr(st, k) is None else getattr(st, k).clone() for k in FIELDS}
            args = (pick_idx, pick_val, first, write_pos, t, write_pos, len_w, first_col, first_pos, groups, lam)
            got = run_select(hip, st, *args)
            again = run_select(hip, st, *args)
            plain = LP.select_best_norm(LP_copy(st), pick_idx, pick_val, first, write_pos, t, write_pos, EOS, len_w, first_col=first_col,
                                        first_pos=first_pos)
            GR.select_groups(st, pick_idx, pick_val, first, write_pos, t, write_pos, EOS, len_w, groups, lam, first_col=first_col,
                             first_pos=first_pos)
            same_state(got, st, (lam, lp, case))
            same_state(again, st, (lam, lp, case, "second run"))
            penalised += not torch.equal(plain.tokens, st.tokens)
            if done_img is not None:                                         # the done image is frozen
                sl = slice(done_img * beam, done_img * beam + beam)
                assert all(torch.equal(bits(getattr(st, k))[sl], bits(before[k])[sl]) for k in ("tokens", "vals", "keys", "ended"))
            if first_pos is not None:                                        # the forced image kept its scores and its keys
                f = first_pos.index(max(first_pos))
                assert torch.equal(st.keys[f * beam:(f + 1) * beam], before["keys"][f * beam:(f + 1) * beam])
    assert penalised > 0                                                     # the groups chose differently from the plain select


def LP_copy(st):
    import copy
    return copy.deepcopy(st)


def test_a_huge_penalty_spreads_the_first_picks_over_the_groups(hip):
    """The hand-worked first step of tests/test_beam_groups_cpu.py on the device: with a penalty no key survives, group g takes the
    picks the groups before it left, so the six slots hold the row's six picks in pick order; what is stored is not penalised."""
    st = LP.new_state(1, 6, 4)
    pi = torch.tensor([[9, 8, 7, 6, 5, 4]] + [[0] * 6] * 5, dtype=torch.int32)
    pv = torch.tensor([[-0.5, -1.0, -1.5, -2.0, -2.5, -3.0]] + [[0.0] * 6] * 5)
    got = run_select(hip, st, pi, pv, True, 0, 0, 0, LP.weights(0.0, 4), 0, None, 3, 1e6)
    assert got["tokens"][:, 0].tolist() == [9, 8, 7, 6, 5, 4]
    assert got["vals"].tolist() == [-0.5, -1.0, -1.5, -2.0, -2.5, -3.0] and got["keys"].tolist() == got["vals"].tolist()
    tiny = run_select(hip, st, pi, pv, True, 0, 0, 0, LP.weights(0.0, 4), 0, None, 3, 1e-9)      # q - d rounds to q: every group is group 0
    assert tiny["tokens"][:, 0].tolist() == [9, 8, 9, 8, 9, 8]


# ---- 2. end to end on the engine's own snapshots ------------------------------------------------------------------------------------
N_IMG, BEAM, GROUPS, MAX_LEN, LAM = T.N_IMG, 6, 3, 10, 0.75
KW = dict(max_len=MAX_LEN, beam_size=BEAM, top_k=20, search="beam")
GKW = dict(num_beam_groups=GROUPS, diversity_penalty=LAM)


def check_steps(steps, length_penalty, max_len, groups=GROUPS, lam=LAM):
    """The restatement applied to every snapshot, with the engine's own picks, gives the next snapshot bit for bit."""
    moved = differs = 0
    for rec in steps:
        assert torch.equal(rec["len_w"], LP.weights(length_penalty, max_len))
        st = T.state_from(rec["before"], rec["beam"])
        if rec["write_pos"] < rec["before"]["tokens"].shape[1]:              # (the Transformer decoders' last step writes no token: skipped)
            plain = LP.select_best_norm(T.state_from(rec["before"], rec["beam"]), rec["pick_idx"], rec["pick_val"], rec["first"],
                                        rec["write_pos"], rec["t"], rec["step"], rec["eos"], rec["len_w"], first_col=rec["first_col"],
                                        first_pos=rec["first_pos"])
            GR.select_groups(st, rec["pick_idx"], rec["pick_val"], rec["first"], rec["write_pos"], rec["t"], rec["step"], rec["eos"],
                             rec["len_w"], groups, lam, first_col=rec["first_col"], first_pos=rec["first_pos"])
            moved += 1
            differs += not torch.equal(plain.tokens, st.tokens)
        same_state(rec["after"], st, rec["step"])
    return moved, differs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_by_step_on_the_engines_own_snapshots(kind, dtype, images, monkeypatch):
    model = T.build(kind, images, dtype)
    args = T.model_args(kind, images)
    steps, finals = T.snapshots(monkeypatch)
    with torch.no_grad():
        beams = model.generate_batch(*args, return_beams=True, **KW, **GKW)
    assert len(steps) == MAX_LEN + (0 if "LSTM" in kind else 1) and len(finals) == 1
    moved, differs = check_steps(steps, 0.0, MAX_LEN)
    assert moved == MAX_LEN and differs > 0                                   # the penalty decided at least one step
    T.same_captions(beams, finals[0])
    assert beams.drawn.tolist() == [0] * N_IMG and T.sorted_desc(beams.scores.cpu())
    assert sorted(beams.beam_index[0].tolist()) == list(range(BEAM))
    first_tokens = beams.tokens[:, :, 0].cpu()
    print(f"{kind} {dtype}: first tokens per beam {first_tokens.tolist()}, lengths {beams.lengths.cpu().tolist()}")
    del steps[:], finals[:]
    with torch.no_grad():
        again = model.generate_batch(*args, return_beams=True, seed=7, rng="torch", **KW, **GKW)
        pair = model.generate_batch(*args, **KW, **GKW)
    assert same(beams, again)
    assert torch.equal(pair[0], beams.tokens[:, 0]) and torch.equal(pair[1], beams.row_lengths)


# ---- 3. the log-prob identity and the attention rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_logprobs_times_the_weight_of_the_length_are_the_scores(kind, images, monkeypatch):
    """The penalty is never stored: for every live beam the fp32 left-to-right sum of its own columns' log-probabilities is the engine's
    raw score, and times ``w[L]`` (``length_penalty=1.0`` here, so that the weight is not 1) it is ``scores``, bit for bit -- wherever the
    returned row holds every column the search wrote (``test_length_penalty_gpu.py`` says where it does not)."""
    model = T.build(kind, images)
    args = T.model_args(kind, images)
    w = LP.weights(1.0, MAX_LEN).numpy()
    steps, finals = T.snapshots(monkeypatch)
    with torch.no_grad():
        beams, lp = model.generate_batch(*args, return_beams=True, return_logprobs=True, length_penalty=1.0, **KW, **GKW)
    state = finals[0]["state"]
    scores, lengths, vals, index = beams.scores.cpu().numpy(), beams.lengths.cpu(), lp.cpu().numpy(), beams.beam_index.cpu()
    live = summed = 0
    for i in range(N_IMG):
        for j in range(BEAM):
            if not np.isfinite(scores[i, j]):
                continue
            live += 1
            row = i * BEAM + int(index[i, j])
            n_cols = T.first_eos_length(state["tokens"][row], 0, MAX_LEN)
            raw = state["vals"][row].numpy()
            assert np.float32(raw * w[n_cols]).tobytes() == scores[i, j].tobytes(), (i, j)
            if int(lengths[i, j]) != n_cols:
                assert "LSTM" not in kind and bool(state["done"][i]) and int(lengths[i, j]) == n_cols - 1
                continue
            acc = np.float32(0.0)
            for c in range(n_cols):
                acc = np.float32(acc + vals[i, j, c])
            assert acc.tobytes() == raw.tobytes(), (i, j)
            assert np.float32(acc * w[n_cols]).tobytes() == scores[i, j].tobytes(), (i, j)
            summed += 1
    print(f"{kind}: {live} live beams, {summed} summed over all their columns")
    assert live > 0.9 * N_IMG * BEAM and summed > 0.5 * live


@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningTransformerWithLabels"))
def test_attention_rows_of_a_beams_own_columns_sum_to_one(kind, images):
    model = T.build(kind, images)
    with torch.no_grad():
        beams, att = model.generate_batch(*T.model_args(kind, images), return_beams=True, return_attention=True, **KW, **GKW)
    sums = att.sum(-1).cpu()
    for i in range(N_IMG):
        for j in range(BEAM):
            n = int(beams.lengths[i, j])
            assert torch.allclose(sums[i, j, :n], torch.ones(n), atol=1e-5) and bool((att[i, j, n:] == 0).all())


# ---- 4. the default is unchanged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_one_group_is_the_call_without_the_keyword(kind, images, monkeypatch):
    from deephumor_amd import hip
    model = T.build(kind, images)
    args = T.model_args(kind, images)
    names = []
    real = hip._launch

    def launch(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "_launch", launch)
    runs = {}
    for tag, extra in (("beam", dict(search="beam")), ("beam 1", dict(search="beam", num_beam_groups=1)),
                       ("beam 1 0", dict(search="beam", num_beam_groups=1, diversity_penalty=0.0)),
                       ("groups", dict(search="beam", **GKW)), ("sample", {}), ("sample 1", dict(num_beam_groups=1))):
        del names[:]
        with torch.no_grad():
            out = model.generate_batch(*args, return_beams=True, max_len=MAX_LEN, beam_size=BEAM, top_k=20, seed=1, **extra)
        runs[tag] = (out, list(names))
    for tag in ("beam 1", "beam 1 0"):
        assert same(runs["beam"][0], runs[tag][0]) and runs["beam"][1] == runs[tag][1]
    assert same(runs["sample"][0], runs["sample 1"][0]) and runs["sample"][1] == runs["sample 1"][1]
    assert "dh_beam_select_groups" not in runs["beam"][1] + runs["sample"][1] and "dh_beam_select_best" not in runs["groups"][1]
    assert runs["groups"][1] == ["dh_beam_select_groups" if n == "dh_beam_select_best" else n for n in runs["beam"][1]]
    assert runs["groups"][1].count("dh_beam_select_groups") == MAX_LEN


# ---- 5. the carriers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_graphed_and_pipeline(kind, images):
    from deephumor_amd.pipeline import CaptionPipeline
    model = T.build(kind, images, torch.bfloat16)
    args = T.model_args(kind, images)
    settings = {2: dict(num_beam_groups=2, diversity_penalty=LAM), 3: dict(num_beam_groups=3, diversity_penalty=LAM)}
    with torch.no_grad():
        eager = {g: model.generate_batch(*args, return_beams=True, **KW, **kw) for g, kw in settings.items()}
        pair = model.generate_batch(*args, **KW, **GKW)
        for _ in range(2):                                                   # capture, then replay
            for g, kw in settings.items():
                assert same(model.generate_batch_graphed(*args, return_beams=True, seed=3, **KW, **kw), eager[g]), g
        plain = model.generate_batch(*args, return_beams=True, **KW)
        assert same(model.generate_batch_graphed(*args, return_beams=True, num_beam_groups=1, **KW), plain)
    keys = sorted(str(dict(k[2]).get("num_beam_groups")) for k in model._graphs)
    assert keys == ["2", "3", "None"]                                        # a graph per group count; one group is the plain graph
    assert not same(eager[2], eager[3])
    # the captured nodes point at the table of ones: the graph's state owns it
    for k, v in model._graphs.items():
        assert (len(v[8]) > 0) == ("num_beam_groups" in dict(k[2]))
    assert torch.equal(pair[0], eager[3].tokens[:, 0]) and torch.equal(pair[1], eager[3].row_lengths)
    batches = [(images[:2],), (images[2:],)]
    got = [tuple(t.clone() for t in r) for r in CaptionPipeline(model, **KW, **GKW).run(batches)]
    assert torch.equal(torch.cat([g[0] for g in got]).cpu(), pair[0].cpu()) and torch.equal(torch.cat([g[1] for g in got]).cpu(), pair[1].cpu())


def test_sharded_through_the_one_rank_group_equals_the_plain_call():
    import json
    import subprocess
    import sys
    child = T.CHILD.replace('search="beam", length_penalty=1.0)', 'search="beam", num_beam_groups=3, diversity_penalty=0.75)')
    child = child.replace("beam_size=3", "beam_size=6")
    assert "num_beam_groups=3" in child and "beam_size=6" in child
    p = subprocess.run([sys.executable, "-c", child % {"root": T.ROOT}], capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    assert json.loads(line[7:]) == {"backend": "nccl", "halves": True, "micro": True}


# ---- 6. composition and group_best ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_composes_with_length_penalty_prompts_bans_and_edits(kind, images, monkeypatch):
    """``length_penalty=1.0``, prompts of unequal lengths, ``min_len``, ``no_repeat_ngram_size`` and ``bad_words_ids`` with the groups:
    every select and the final order are the restatement's on the engine's own snapshots (so the tokens are)."""
    model = T.build(kind, images)
    args = T.model_args(kind, images)
    cap = torch.randint(6, 1000, (N_IMG, 3), generator=torch.Generator().manual_seed(2)).cuda()
    lens = [0, 2, 1, 3]
    extra = dict(caption=cap, caption_lengths=torch.tensor(lens), min_len=5, no_repeat_ngram_size=2, bad_words_ids=[[17], [230, 45]],
                 length_penalty=1.0)
    steps, finals = T.snapshots(monkeypatch)
    with torch.no_grad():
        beams = model.generate_batch(*args, return_beams=True, **KW, **GKW, **extra)
    moved, _ = check_steps(steps, 1.0, MAX_LEN)
    assert moved == MAX_LEN and all(rec["first_pos"] == lens for rec in steps)
    T.same_captions(beams, finals[0])
    for i, n in enumerate(lens):
        assert beams.tokens[i, :, :n].tolist() == [cap[i, :n].tolist()] * BEAM
        for j in range(BEAM):
            if torch.isfinite(beams.scores[i, j]):
                row = beams.tokens[i, j].tolist()
                assert EOS not in row[n:5] and 17 not in row[n:int(beams.lengths[i, j])]


def test_group_best_returns_each_groups_top_beam(images):
    from deephumor_amd.experiments import group_best
    model = T.build("CaptioningLSTM", images)
    with torch.no_grad():
        beams = model.generate_batch(*T.model_args("CaptioningLSTM", images), return_beams=True, **KW, **GKW)
    best = group_best(beams, GROUPS)
    bg = BEAM // GROUPS
    assert best.tokens.shape == (N_IMG, GROUPS, MAX_LEN) and best.scores.shape == (N_IMG, GROUPS)
    want = GR.group_best(dict(beam_index=beams.beam_index.cpu()), GROUPS)
    for i in range(N_IMG):
        for g in range(GROUPS):
            slot = int(want[i, g])
            assert int(beams.beam_index[i, slot]) // bg == g
            assert all(int(beams.beam_index[i, s]) // bg != g for s in range(slot))       # no better beam of the group in front of it
            assert torch.equal(best.tokens[i, g], beams.tokens[i, slot]) and int(best.lengths[i, g]) == int(beams.lengths[i, slot])
            assert bits(best.scores[i, g].cpu()).item() == bits(beams.scores[i, slot].cpu()).item()
            assert int(best.beam_index[i, g]) == int(beams.beam_index[i, slot])
        assert int(best.drawn[i]) == int(beams.beam_index[i, 0]) // bg
