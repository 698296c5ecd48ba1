"""``experiments.token_alternatives`` on a real MI355X: tokens and ranks EQUAL the restatement of ``alternatives_ref`` on the model's own
teacher-forced logits (taken through ``scoring._pass_logits`` for the same captions), the values are within a measured gate of its
fp64 ``log_softmax``; five kinds, fp32 / fp16 / bf16.

Shapes: V = 301 (``V % 64 != 0``, ``V % 4 != 0``: in the classifier's dense output all rows but every fourth start off a 16-byte boundary,
where the sweep's scalar head would make a row's last bit depend on its index in the pass -- the product brings every row onto a boundary,
and the batch-size, ``n`` and order tests below are what fails if it does not; the sweep's scalar tail runs),
25 positions, 21 and 20 captions (525 and 500 rows, either side of 512), ``top`` 1 / 5 / 64, ``batch_size`` n / 7 / 1, the caption order
permuted, captions with pads, ``temperature`` 0.7, ``unk_index``, tied classifier rows, a classifier of zeros at V = 1101 (more columns
at the bound than the kernel's 1,024-candidate buffer holds: its flat branch), a NaN weight.

Every gate is 1.25 x the worst value seen on an MI355X (``alternatives_ref.WORST``; the tests print what they see before they assert;
profiles/alternatives/errors.txt) under a ceiling that is no measurement: 2e-5 against the fp64 restatement (``beam_best.hip``'s stated
bound at ``|x / T| <= 32``), 1e-3 against the reference (G28), ``explain_captions`` and generation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import alternatives_ref as A  # noqa: E402
import explain_ref as E  # noqa: E402
from helpers import synth_images  # noqa: E402

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES, DT_IDS = (F32, F16, BF16), ("f32", "f16", "bf16")
NAME = dict(zip(DTYPES, DT_IDS))
N = 21                                     # 21 x 25 = 525 rows; 20 captions: 500 rows


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


_MODELS = {}


def fresh(kind, dt, hp=None, seed=E.SEED, edit=None):
    """A model of its own (not cached): ``edit(model)`` changes weights before the first forward builds the decoder's plan."""
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_state_dict
    model = getattr(M, kind)(**(hp or A.HP[kind])).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed))
    if edit is not None:
        with torch.no_grad():
            edit(model)
    return model.to(dt).cuda()


def build(kind, dt):
    if (kind, dt) not in _MODELS:
        _MODELS[(kind, dt)] = fresh(kind, dt)
    return _MODELS[(kind, dt)]


@pytest.fixture(scope="module", autouse=True)
def drop_models():
    yield
    _MODELS.clear()


@pytest.fixture(scope="module")
def images():
    return synth_images(A.N_TEMPLATES, seed=0).cuda()


def split(hip, dt, on=1):
    return hip.option_scope(**(dict(f32_split=on) if dt == F32 else {}))


def alternatives(model, kind, images, dt, inputs, **kw):
    from deephumor_amd.experiments import token_alternatives
    cap, lengths, index, labels = inputs
    return token_alternatives(model, images.to(dt), index.cuda(), cap.cuda(), lengths.cuda(),
                              labels=labels.cuda() if "WithLabels" in kind else None, **kw)


def own_logits(model, kind, images, dt, inputs):
    """The model's teacher-forced fp32 logits of all the captions in ONE pass, through the product's helper -> CPU [n * L, V]."""
    from deephumor_amd.experiments.scoring import _pass_logits
    cap, _, index, labels = inputs
    with torch.no_grad():
        feats = model.encoder(images.to(dt), labels.cuda()) if "WithLabels" in kind else model.encoder(images.to(dt))
        spatial = None
        if isinstance(feats, tuple):
            feats, spatial = feats
        idx = index.cuda()
        logits, _ = _pass_logits(model.decoder, feats.index_select(0, idx), None if spatial is None else spatial.index_select(0, idx),
                                 cap.cuda())
    assert logits.dtype == torch.float32 and tuple(logits.shape[:2]) == tuple(cap.shape)
    return logits.cpu().reshape(cap.numel(), -1).contiguous()


def against_restatement(got, logits, cap, top, what, **kw):
    """Tokens and rank EXACTLY; -> the largest value error over the live entries (dead slots and pads must match exactly)."""
    n, l = cap.shape
    toks, vals, rank = A.alternatives(logits, cap.reshape(-1), top, **kw)
    g_t, g_v, g_r = (t.cpu() for t in got)
    assert g_t.shape == (n, l, top) and g_t.dtype == torch.int64 and g_v.shape == (n, l, top) and g_v.dtype == torch.float32
    assert g_r.shape == (n, l) and g_r.dtype == torch.int64
    assert torch.equal(g_t.view(n * l, top), toks), (what, int((g_t.view(n * l, top) != toks).sum()))
    assert torch.equal(g_r.view(-1), rank), what
    g_v = g_v.view(n * l, top).double()
    fixed = torch.isinf(vals) | (toks < 0)
    assert torch.equal(g_v[fixed], vals[fixed]), what
    pad = cap == E.PAD
    assert bool((g_t[pad] == -1).all()) and bool((g_v.view(n, l, top)[pad] == 0.0).all()) and bool((g_r[pad] == -1).all())
    return float((g_v - vals)[~fixed].abs().max()) if bool((~fixed).any()) else 0.0


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. every kind and type against the restatement on its own logits -------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_against_the_restatement(hip, images, kind, dt):
    from deephumor_amd.experiments import explain_captions
    model = build(kind, dt)
    inputs = A.captions(N)
    cap = inputs[0]
    assert bool((cap == E.PAD).any()) and bool((cap[0] != E.PAD).all()) and N * A.L > 512 > (N - 1) * A.L and A.V % 64 and A.V % 4
    worst = 0.0
    for on in ((1, 0) if dt == F32 else (1,)):
        with split(hip, dt, on):
            logits = own_logits(model, kind, images, dt, inputs)
            got = alternatives(model, kind, images, dt, inputs)
            err = against_restatement(got, logits, cap, 5, (kind, dt, on))
            print(f"[alternatives restatement] {kind} {NAME[dt]} f32_split={on if dt == F32 else '-'}: top 5, 525 rows: {err:.3e}")
            worst = max(worst, err)
            if on == 0:
                continue
            for top in (1, 64):
                e = against_restatement(alternatives(model, kind, images, dt, inputs, top=top), logits, cap, top, (kind, dt, top))
                print(f"[alternatives restatement] {kind} {NAME[dt]}: top {top}: {e:.3e}")
                worst = max(worst, e)
            e = against_restatement(alternatives(model, kind, images, dt, inputs, temperature=0.7), logits, cap, 5, (kind, dt, "T"),
                                    temperature=0.7)
            print(f"[alternatives restatement] {kind} {NAME[dt]}: temperature 0.7: {e:.3e}")
            worst = max(worst, e)
            # the other side of 512 rows
            fewer = tuple(t[:N - 1] if t.shape[0] == N else t for t in inputs)
            e = against_restatement(alternatives(model, kind, images, dt, fewer), own_logits(model, kind, images, dt, fewer), fewer[0], 5,
                                    (kind, dt, "500 rows"))
            print(f"[alternatives restatement] {kind} {NAME[dt]}: 500 rows: {e:.3e}")
            worst = max(worst, e)
            # where the target is among the picks, its value is explain_captions' log-prob of it
            cap_d = cap.cuda()
            lp = explain_captions(model, images.to(dt), inputs[2].cuda(), cap_d, inputs[1].cuda(),
                                  labels=inputs[3].cuda() if "WithLabels" in kind else None).logprobs
            found = got.rank >= 0
            assert bool(found.any()) and not bool((found & (cap_d == E.PAD)).any())
            mine = got.logprobs.gather(-1, got.rank.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            d = float((mine - lp)[found].abs().max())
            g_e = min(A.gate(A.WORST["explain"][NAME[dt]]), A.REFERENCE_CEILING)
            print(f"[alternatives explain] {kind} {NAME[dt]}: logprobs[..., rank] vs explain_captions {d:.3e} over {int(found.sum())} "
                  f"positions (gate {g_e:.3e})")
            assert d <= g_e
    g_r = min(A.gate(A.WORST["restatement"][NAME[dt]]), A.RESTATEMENT_CEILING)
    print(f"[alternatives restatement] {kind} {NAME[dt]}: worst {worst:.3e} (gate {g_r:.3e})")
    assert worst <= g_r


# ---- 1b. a caption's bits depend on nothing but the caption ----------------------------------------------------------------------------
def differing(a, b):
    """'' when the two results hold the same bits, else which fields differ and by how much."""
    out = []
    for name, x, y in zip(a._fields, a, b):
        if not torch.equal(x, y):
            both = torch.isfinite(x.double()) & torch.isfinite(y.double())
            out.append(f"{name}: {int((x != y).sum())} entries, up to {float((x.double() - y.double())[both].abs().max()):.3e}")
    return "; ".join(out)


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_batch_size_n_and_order_change_no_bit(hip, images, kind, dt):
    from deephumor_amd.experiments import TokenAlternatives
    model = build(kind, dt)
    inputs = A.captions(N)
    fewer = tuple(t[:N - 1] if t.shape[0] == N else t for t in inputs)
    with split(hip, dt):
        got = alternatives(model, kind, images, dt, inputs)
        assert same(got, alternatives(model, kind, images, dt, inputs))              # run to run
        found = {"batch_size 7": differing(got, alternatives(model, kind, images, dt, inputs, batch_size=7)),
                 "batch_size 1": differing(got, alternatives(model, kind, images, dt, inputs, batch_size=1)),
                 "n": differing(TokenAlternatives(*(t[:N - 1] for t in got)), alternatives(model, kind, images, dt, fewer))}
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
        moved = alternatives(model, kind, images, dt, (inputs[0][perm], inputs[1][perm], inputs[2][perm], inputs[3]), batch_size=8)
        found["order"] = differing(TokenAlternatives(*(t[perm.cuda()] for t in got)), moved)
    print(f"[alternatives bits] {kind} {NAME[dt]}: {found}")
    assert not any(found.values()), found


# ---- 2. unk_index, ties, the flat branch, NaN -------------------------------------------------------------------------------------------
EDIT_KINDS = ("CaptioningLSTM", "CaptioningTransformer")


@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("dt", (F32, BF16), ids=("f32", "bf16"))
def test_unk_index(hip, images, kind, dt):
    model = build(kind, dt)
    inputs = A.captions(5)
    cap = inputs[0]
    unk = int(cap[0, 3])
    assert unk != E.PAD and int((cap == unk).sum()) >= 1
    with split(hip, dt):
        logits = own_logits(model, kind, images, dt, inputs)
        free = alternatives(model, kind, images, dt, inputs, top=64)
        got = alternatives(model, kind, images, dt, inputs, top=64, unk_index=unk)
    against_restatement(got, logits, cap, 64, (kind, dt, "unk"), unk=unk)
    assert bool((free.tokens == unk).any())                                          # (it would have been listed)
    assert not bool((got.tokens == unk).any()) and bool((got.rank[cap.cuda() == unk] == -1).all())
    # the other picks move up one slot and keep their values: the logsumexp still counts unk
    row = (free.tokens[0, 3] != unk).nonzero().squeeze(1)[:63]
    assert torch.equal(got.tokens[0, 3, :63], free.tokens[0, 3][row]) and torch.equal(got.logprobs[0, 3, :63], free.logprobs[0, 3][row])


@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("dt", (F32, BF16), ids=("f32", "bf16"))
def test_tied_classifier_rows(hip, images, kind, dt):
    """Classifier rows 200 and 9 made identical, weight and bias (the bias raised so that the pair is near the top): their logits tie
    bit for bit and id 9 comes first."""
    def edit(model):
        c = model.decoder.classifier
        c.bias[200] += 8.0
        c.weight[9], c.bias[9] = c.weight[200], c.bias[200]
    model = fresh(kind, dt, edit=edit)
    inputs = A.captions(5)
    with split(hip, dt):
        logits = own_logits(model, kind, images, dt, inputs)
        got = alternatives(model, kind, images, dt, inputs, top=5)
    assert torch.equal(logits[:, 9], logits[:, 200])
    against_restatement(got, logits, inputs[0], 5, (kind, dt, "ties"))
    real = (inputs[0] != E.PAD).cuda()
    at9 = (got.tokens == 9).int().argmax(-1)
    has9, has200 = (got.tokens == 9).any(-1), (got.tokens[..., 1:] == 200).any(-1)
    assert not bool((got.tokens[..., 0] == 200).any())                               # never in front of its twin
    nxt = got.tokens.gather(-1, (at9 + 1).clamp(max=4).unsqueeze(-1)).squeeze(-1)
    both = real & has9 & (at9 < 4)
    assert bool(both.any()) and bool((nxt[both] == 200).all()) and bool((has200 == (has9 & (at9 < 4)))[real].all())
    vals = got.logprobs.gather(-1, torch.stack([at9, (at9 + 1).clamp(max=4)], -1))
    assert torch.equal(vals[..., 0][both], vals[..., 1][both])


@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("dt", (F32, BF16), ids=("f32", "bf16"))
def test_classifier_of_zeros(hip, images, kind, dt):
    """Every logit 0 at V = 1101: more columns at the bound than the kernel's candidate buffer holds.  The ``top`` lowest ids."""
    v = 1101

    def edit(model):
        model.decoder.classifier.weight.zero_()
        model.decoder.classifier.bias.zero_()
    model = fresh(kind, dt, hp=dict(A.HP[kind], num_tokens=v), edit=edit)
    cap, lengths, index, labels = A.captions(3)
    inputs = (cap, lengths, index, labels)
    want = float(-np.log(float(v)))
    with split(hip, dt):
        logits = own_logits(model, kind, images, dt, inputs)
        assert logits.shape[1] == v and bool((logits == 0).all())
        for top, unk, ids in ((5, None, [0, 1, 2, 3, 4]), (5, 2, [0, 1, 3, 4, 5]), (64, 0, list(range(1, 65))), (1, None, [0])):
            got = alternatives(model, kind, images, dt, inputs, top=top, unk_index=unk)
            err = against_restatement(got, logits, cap, top, (kind, dt, top, unk), unk=unk)
            real = (cap != E.PAD).cuda()
            assert bool((got.tokens[real] == torch.tensor(ids).cuda()).all())
            off = float((got.logprobs[real].double() - want).abs().max())
            print(f"[alternatives flat] {kind} {NAME[dt]} top {top} unk {unk}: vs the restatement {err:.3e}, vs -log V {off:.3e}")
            assert err <= A.RESTATEMENT_CEILING


@pytest.mark.parametrize("kind", EDIT_KINDS)
@pytest.mark.parametrize("dt", (F32, BF16), ids=("f32", "bf16"))
def test_nan_weight_raises(hip, images, kind, dt):
    def edit(model):
        model.decoder.classifier.weight[5, 3] = float("nan")
    model = fresh(kind, dt, edit=edit)
    with split(hip, dt):
        with pytest.raises(RuntimeError, match="a row's logits hold NaN or \\+inf"):
            alternatives(model, kind, images, dt, A.captions(2))
        ok = alternatives(build(kind, dt), kind, images, dt, A.captions(2))          # the next call is clean: the word is per call
    assert bool(torch.isfinite(ok.logprobs).all())


# ---- 3. cross-check with generation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_generation_cross_check(hip, images, kind, dt):
    """Every beam of ``search="beam"`` fed back teacher-forced with ``top = beam_size`` and the search's ``unk_index``: every generated
    token is among the picks of its position, and its value is the log-prob generation recorded (temperature 1, no edits)."""
    model = build(kind, dt)
    _, _, _, labels = A.captions(1)
    args = (images.to(dt), labels.cuda()) if "WithLabels" in kind else (images.to(dt),)
    with split(hip, dt), torch.no_grad():
        beams, lps = model.generate_batch(*args, search="beam", beam_size=3, max_len=8, return_beams=True, return_logprobs=True)
        n, b, t = beams.tokens.shape
        assert (n, b, t) == (3, 3, 8)
        lens = beams.lengths.reshape(n * b)
        keep = torch.arange(t, device=lens.device)[None, :] < lens[:, None]
        rows = torch.where(keep, beams.tokens.reshape(n * b, t), torch.zeros((), dtype=torch.int64, device=lens.device))
        # the search does not ban id 0, and an LSTM beam may hold it (bf16 CaptioningLSTMWithLabels does): pad_index=-1 makes no
        # position a pad, so every generated token is compared; a decoder that masks id 0 as a key must not have generated it
        assert hasattr(model.decoder, "lstm") or bool((rows[keep] != E.PAD).all())
        index = torch.arange(n).repeat_interleave(b)
        got = alternatives(model, kind, images, dt, (rows, lens, index, labels), top=b, unk_index=1, pad_index=-1)
    assert bool((got.rank[keep] >= 0).all())
    mine = got.logprobs.gather(-1, got.rank.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    d = float((mine - lps.reshape(n * b, t))[keep].abs().max())
    g = min(A.gate(A.WORST["generation"][NAME[dt]]), A.REFERENCE_CEILING)
    print(f"[alternatives generation] {kind} {NAME[dt]}: {int(keep.sum())} generated tokens, all ranked; values {d:.3e} (gate {g:.3e})")
    assert d <= g


# ---- 4. golden G28 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_g28(hip, kind, dt):
    """fp32: the reference's ids on every entry whose stored gap exceeds 2e-3, its values within the gate on all entries.  fp16 / bf16:
    recorded only -- their weights are rounded, their binding check is the exact comparison on their own logits above."""
    g = A.golden(kind)
    model = fresh(kind, dt, hp=E.HP[kind], seed=int(g["seed"]))
    images4, cap, lengths, index, labels = A.g28_inputs(synth_images(3, seed=0))
    real = torch.from_numpy(g["captions"] != E.PAD)
    sure = real[..., None] & torch.from_numpy(g["gaps"] > A.GAP)
    want_t, want_v = torch.from_numpy(g["tokens"]), torch.from_numpy(g["logprobs"]).double()
    for on in ((1, 0) if dt == F32 else (1,)):
        with split(hip, dt, on):
            got = alternatives(model, kind, images4.cuda(), dt, (cap, lengths, index, labels), top=A.G28_TOP).map(lambda t: t.cpu())
        wrong = int((got.tokens != want_t)[sure].sum())
        err = float((got.logprobs.double() - want_v)[real].abs().max())
        print(f"[alternatives g28] {kind} {NAME[dt]} f32_split={on if dt == F32 else '-'}: {wrong} of {int(sure.sum())} sure ids differ, "
              f"values {err:.3e}")
        assert torch.equal(got.tokens[0::4], got.tokens[3::4]) and torch.equal(got.logprobs[0::4], got.logprobs[3::4])      # the second copy
        if dt == F32:
            g28 = min(A.gate(A.WORST["g28"]), A.REFERENCE_CEILING)
            print(f"[alternatives g28] fp32 gate {g28:.3e}")
            assert wrong == 0 and err <= g28
