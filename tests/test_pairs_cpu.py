"""``experiments.score_pairs`` and the readers of its matrix without a GPU: ``rank_templates`` / ``rank_captions`` /
``template_accuracy`` against the fp64 numpy restatements of ``pairs_ref`` (random matrices, planted ties, priors, PMI), their refusals,
the ``PairScores`` record, ``score_pairs``' argument checks (which run before the encoder), golden G26's own consistency with G25, and
the pins this feature must not move: 129 prototypes, ABI 35, 15 options.

Bounds.  The readers compute their keys in fp64 and round once to fp32: ``score`` is compared with the fp64 restatement at 1 fp32
ulp (the rounding is half an ulp; torch's and numpy's fp64 ``log`` / ``exp`` may differ in the last fp64 bit, far below it), the
probabilities (<= 1) at 1e-7 absolute, the orders exactly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import explain_ref as E
import pairs_ref as P
from deephumor_amd.experiments import (CaptionRanks, PairScores, TemplateRanks, rank_captions, rank_templates, score_pairs,
                                       template_accuracy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROB_ATOL = 1e-7


def random_matrix(n, t, seed):
    g = torch.Generator().manual_seed(seed)
    return (-40.0 * torch.rand(n, t, generator=g) - 5.0).float(), torch.randint(1, 10, (n,), generator=g)


# ---- rank_templates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,top", [(1, 1, 1), (5, 3, 2), (9, 17, 17), (4, 300, 5)])
def test_rank_templates_matches_the_restatement(n, t, top):
    lp, _ = random_matrix(n, t, 100 + t)
    g = torch.Generator().manual_seed(t)
    for prior in (None, torch.rand(t, generator=g) + 0.05):
        got = rank_templates(lp, top=top, prior=prior)
        index, score, prob = P.rank_templates(lp.numpy(), top, None if prior is None else prior.numpy())
        assert isinstance(got, TemplateRanks) and got.index.dtype == torch.int64 and got.score.dtype == got.probability.dtype == torch.float32
        assert got.index.shape == got.score.shape == got.probability.shape == (n, top)
        assert np.array_equal(got.index.numpy(), index)
        assert P.ulps32(got.score.numpy(), score) <= 1.0
        assert float(np.abs(got.probability.double().numpy() - prob).max()) <= PROB_ATOL
        assert torch.equal(rank_templates(PairScores(lp, lp.neg().exp()), top=top, prior=prior).index, got.index)   # the record or its logprob
    full = rank_templates(lp, top=t)
    assert float((full.probability.double().sum(1) - 1).abs().max()) <= 1e-6        # top = T: the whole posterior
    assert bool((full.score[:, :-1] >= full.score[:, 1:]).all())


def test_rank_templates_ties_go_to_the_lower_index():
    lp, _ = random_matrix(6, 5, 7)
    lp[:, 3] = lp[:, 0]                                                              # a second copy of template 0
    lp[:, 4] = lp[:, 1]
    got = rank_templates(lp, top=5)
    pos = lambda row, j: row.tolist().index(j)                                       # noqa: E731
    for row in got.index:
        assert pos(row, 0) + 1 == pos(row, 3) and pos(row, 1) + 1 == pos(row, 4)
    assert np.array_equal(got.index.numpy(), P.rank_templates(lp.numpy(), 5)[0])
    assert torch.equal(rank_templates(torch.zeros(3, 4), top=4).index, torch.arange(4).expand(3, 4))     # all equal: 0, 1, 2, 3
    assert torch.equal(got.index, rank_templates(lp, top=5).index)                   # deterministic


def test_prior_reorders_as_the_formula_says():
    lp = torch.tensor([[-10.0, -10.5, -12.0]])
    assert rank_templates(lp, top=3).index.tolist() == [[0, 1, 2]]
    got = rank_templates(lp, top=3, prior=torch.tensor([1.0, 2.0, 1.0]))             # log 2 = 0.69 > 0.5: template 1 overtakes
    assert got.index.tolist() == [[1, 0, 2]]
    key = np.array([-10.0 + np.log(0.25), -10.5 + np.log(0.5), -12.0 + np.log(0.25)])
    assert P.ulps32(got.score.numpy()[0], key[[1, 0, 2]]) <= 1.0
    assert rank_templates(lp, top=3, prior=torch.tensor([1.0, 1.6, 1.0])).index.tolist() == [[0, 1, 2]]     # log 1.6 = 0.47 < 0.5
    scaled = rank_templates(lp, top=3, prior=torch.tensor([10.0, 20.0, 10.0]))       # normalised: the scale of the prior is nothing
    assert torch.equal(scaled.score, got.score) and torch.equal(scaled.probability, got.probability)
    uniform = rank_templates(lp, top=3, prior=torch.ones(3))
    assert torch.equal(uniform.score, rank_templates(lp, top=3).score)               # None is the uniform prior
    assert P.ulps32(uniform.score.numpy()[0], lp.numpy()[0].astype(np.float64) - np.log(3.0)) <= 1.0


def test_rank_templates_refusals():
    lp, _ = random_matrix(4, 3, 1)
    with pytest.raises(ValueError, match="top = 4 exceeds the 3 templates"):
        rank_templates(lp, top=4)
    with pytest.raises(ValueError, match="top must be an int >= 1"):
        rank_templates(lp, top=0)
    with pytest.raises(ValueError, match="top must be an int >= 1"):
        rank_templates(lp, top=True)
    for bad in (torch.tensor([1.0, 0.0, 1.0]), torch.tensor([1.0, -0.5, 1.0]), torch.tensor([1.0, float("nan"), 1.0])):
        with pytest.raises(ValueError, match="prior must be positive"):
            rank_templates(lp, top=2, prior=bad)
    with pytest.raises(ValueError, match=r"prior must have shape \[3\]"):
        rank_templates(lp, top=2, prior=torch.ones(4))
    with pytest.raises(ValueError, match="scores must be a PairScores or its logprob"):
        rank_templates(lp[0], top=1)


# ---- rank_captions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", (None, "length", "pmi"))
@pytest.mark.parametrize("n,t,top", [(1, 1, 1), (7, 4, 7), (40, 6, 5)])
def test_rank_captions_matches_the_restatement(n, t, top, normalize):
    lp, lengths = random_matrix(n, t, 200 + n)
    got = rank_captions(lp, lengths, top=top, normalize=normalize)
    index, score = P.rank_captions(lp.numpy(), lengths.numpy(), top, normalize)
    assert isinstance(got, CaptionRanks) and got.index.dtype == torch.int64 and got.score.dtype == torch.float32
    assert got.index.shape == got.score.shape == (t, top)
    assert np.array_equal(got.index.numpy(), index)
    if normalize == "pmi" and t == 1:
        assert bool((got.score == 0).all())                                          # one template: nothing is specific to it
    else:
        assert P.ulps32(got.score.numpy(), score) <= 1.0
    assert torch.equal(rank_captions(PairScores(lp, lp), lengths, top=top, normalize=normalize).index, got.index)


def test_rank_captions_ties_go_to_the_lower_index():
    lp, lengths = random_matrix(6, 3, 9)
    lp[4] = lp[1]                                                                    # a duplicate caption
    lengths[4] = lengths[1]
    for normalize in (None, "length", "pmi"):
        got = rank_captions(lp, lengths, top=6, normalize=normalize)
        for row in got.index.tolist():
            assert row.index(1) + 1 == row.index(4), normalize
        assert np.array_equal(got.index.numpy(), P.rank_captions(lp.numpy(), lengths.numpy(), 6, normalize)[0])


def test_pmi_prefers_the_specific_caption():
    """Caption 0 is likely under every template (-5 everywhere); caption t + 1 is unlikely except under template t (-8 there, -40
    elsewhere).  By log-probability the generic caption leads every template; by PMI it scores exactly 0 and every template's own
    caption leads: log(3) - log(1 + 2 exp(-32)) = 1.0986 above the average template."""
    lp = torch.full((4, 3), -40.0)
    lp[0] = -5.0
    for t in range(3):
        lp[t + 1, t] = -8.0
    lengths = torch.tensor([3, 3, 3, 3])
    plain = rank_captions(lp, lengths, top=2)
    pmi = rank_captions(lp, lengths, top=2, normalize="pmi")
    assert plain.index[:, 0].tolist() == [0, 0, 0]
    assert pmi.index.tolist() == [[1, 0], [2, 0], [3, 0]] and not torch.equal(pmi.index, plain.index)
    assert bool((pmi.score[:, 1] == 0).all())
    assert P.ulps32(pmi.score[:, 0].numpy(), np.full(3, np.log(3.0) - np.log1p(2 * np.exp(-32.0)))) <= 1.0


def test_length_normalisation_prefers_the_longer_caption_with_the_better_tokens():
    lp = torch.tensor([[-6.0], [-12.0]])
    lengths = torch.tensor([2, 6])                                                   # -3 per token against -2 per token
    assert rank_captions(lp, lengths, top=2).index.tolist() == [[0, 1]]
    got = rank_captions(lp, lengths, top=2, normalize="length")
    assert got.index.tolist() == [[1, 0]] and got.score.tolist() == [[-2.0, -3.0]]


def test_rank_captions_refusals():
    lp, lengths = random_matrix(4, 3, 2)
    with pytest.raises(ValueError, match="top = 5 exceeds the 4 captions"):
        rank_captions(lp, lengths, top=5)
    with pytest.raises(ValueError, match="normalize must be None, 'length' or 'pmi'"):
        rank_captions(lp, lengths, top=2, normalize="mean")
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[4\]"):
        rank_captions(lp, lengths[:3], top=2)
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[4\]"):
        rank_captions(lp, lengths.float(), top=2)
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[4\]"):
        rank_captions(lp, lengths * 0, top=2, normalize="length")


# ---- template_accuracy ------------------------------------------------------------------------------------------------------------
def test_template_accuracy_by_hand():
    """4 captions, 3 templates.  True templates 0, 1, 2, 1.  Ranks: caption 0 -> (0, 1, 2): hit at 1; caption 1 -> (2, 1, 0): hit at 2;
    caption 2 -> (0, 1, 2): hit at 3; caption 3 -> (1, 0, 2): hit at 1.  So top-1 = 2/4, top-2 = 3/4, top-3 = 4/4."""
    lp = torch.tensor([[-1.0, -2.0, -3.0], [-3.0, -2.0, -1.0], [-1.0, -2.0, -3.0], [-2.0, -1.0, -3.0]])
    ranks = rank_templates(lp, top=3)
    assert ranks.index.tolist() == [[0, 1, 2], [2, 1, 0], [0, 1, 2], [1, 0, 2]]
    true = torch.tensor([0, 1, 2, 1])
    assert template_accuracy(ranks, true, ks=(1, 2, 3)) == {1: 0.5, 2: 0.75, 3: 1.0}
    assert template_accuracy(ranks.index, true, ks=(2,)) == {2: 0.75}
    assert template_accuracy(ranks, true, ks=(1, 3)) == P.template_accuracy(ranks.index.numpy(), true.numpy(), (1, 3))
    with pytest.raises(ValueError, match=r"every k must be an int in 1 .. top = 2"):
        template_accuracy(rank_templates(lp, top=2), true)                           # the default ks = (1, 5)
    with pytest.raises(ValueError, match=r"true_index must be an integer tensor of shape \[4\]"):
        template_accuracy(ranks, true[:3], ks=(1,))


# ---- PairScores -------------------------------------------------------------------------------------------------------------------
def test_pair_scores_record():
    a = PairScores(torch.zeros(2, 3), torch.ones(2, 3))
    assert a._fields == ("logprob", "perplexity")
    d = a.map(lambda t: t.double())
    assert isinstance(d, PairScores) and all(t.dtype == torch.float64 for t in d)
    c = PairScores.cat([a, a.map(lambda t: t + 1)])
    assert isinstance(c, PairScores) and c.logprob.shape == (4, 3) and c.perplexity[:, 0].tolist() == [1, 1, 2, 2]


# ---- score_pairs: validation, before the encoder runs -----------------------------------------------------------------------------
class Reached(Exception):
    pass


def build(kind, **extra):
    import deephumor_amd.models as M
    from deephumor_amd.synth import synth_state_dict
    model = getattr(M, kind)(**dict(E.HP[kind], **extra)).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=E.SEED))
    return model


@pytest.mark.parametrize("kind", ("CaptioningTransformer", "CaptioningLSTM", "CaptioningTransformerBase"))
def test_arguments_are_checked_before_the_encoder_runs(kind, monkeypatch):
    cap, lengths, _, _ = E.captions()
    images = torch.zeros(P.N_TEMPLATES, 3, 8, 8)
    model = build(kind)
    entered = []

    def encoder(*a, **kw):
        entered.append(1)
        raise Reached
    monkeypatch.setattr(model.encoder, "forward", encoder)
    call = lambda **kw: score_pairs(model, kw.pop("images", images), kw.pop("cap", cap), kw.pop("lengths", lengths), **kw)      # noqa: E731
    bad = cap.clone()
    bad[1, 2] = E.V
    with pytest.raises(IndexError, match="index out of range in self"):
        call(cap=bad)
    bad[1, 2] = -1
    with pytest.raises(IndexError, match="index out of range in self"):
        call(cap=bad)
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[7\]"):
        call(lengths=lengths[:6])
    with pytest.raises(ValueError, match=r"lengths must be an integer tensor of shape \[7\]"):
        call(lengths=lengths.float())
    with pytest.raises(ValueError, match="lengths must be >= 1"):
        call(lengths=lengths - 1)
    with pytest.raises(ValueError, match="captions must be an int64 tensor"):
        call(cap=cap.int())
    with pytest.raises(ValueError, match="captions must be an int64 tensor"):
        call(cap=cap[0])
    with pytest.raises(ValueError, match="captions must be an int64 tensor"):
        call(cap=cap[:0])
    with pytest.raises(ValueError, match="batch_size must be an int >= 1"):
        call(batch_size=0)
    with pytest.raises(ValueError, match="batch_size must be an int >= 1"):
        call(batch_size=2.0)
    with pytest.raises(TypeError, match="pad_index must be an int"):
        call(pad_index=0.0)
    with pytest.raises(ValueError, match="T >= 1 templates"):
        call(images=images[:0])
    assert not entered
    with pytest.raises(Reached):                                                     # valid arguments reach it
        call()
    assert entered == [1]


# ---- golden G26 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", E.KINDS)
def test_g26_holds_what_it_says(kind):
    """The fixture's inputs are the shared ones; its copy column repeats column 0; on the pairs G25 scored (caption i under
    ``template_index[i]`` of the first three templates) it is G25's per-token values summed, to fp64 rounding."""
    g = P.golden(kind)
    cap, lengths, index, labels = E.captions()
    assert int(g["seed"]) == E.SEED and np.array_equal(g["captions"], cap.numpy()) and np.array_equal(g["lengths"], lengths.numpy())
    assert tuple(g["templates"]) == P.TEMPLATES and np.array_equal(g["labels"], labels[torch.tensor(P.TEMPLATES)].numpy())
    lp, pp = g["logprob"], g["perplexity"]
    assert lp.shape == pp.shape == (P.N_CAPTIONS, P.N_TEMPLATES) and lp.dtype == pp.dtype == np.float64
    assert np.array_equal(lp[:, 0], lp[:, 3]) and np.array_equal(pp[:, 0], pp[:, 3])
    assert np.array_equal(pp, np.exp(-lp / lengths.numpy()[:, None]))
    g25 = torch.from_numpy(E.golden(kind)["logprobs"]).masked_fill(cap == E.PAD, 0.0).sum(-1).numpy()
    assert float(np.abs(lp[np.arange(7), index.numpy()] - g25).max()) <= 1e-12
    ranks = rank_templates(torch.from_numpy(lp), top=4)
    for row in ranks.index.tolist():
        assert row.index(0) + 1 == row.index(3)                                      # the copy ranks right behind its original


# ---- the pins ---------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_did_not_grow():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    n_protos = len(re.findall(r"^(?:int|const char\*|void|unsigned long long|double|float)\s+\*?dh_\w+\s*\(", text, flags=re.M))
    assert n_protos == 129 and "129 entry points" in open(os.path.join(ROOT, "README.md")).read()
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    assert len(hip.SIGNATURES) == len(_abi.SIGNATURES) == 124                       # (the Python-side table: unchanged in length)
    assert len(_abi.SIGNATURES["dh_attn_cross_prefill"]) == 13 and len(_abi.SIGNATURES["dh_attn_cross_prefill_packed"]) == 15
    assert len(_abi.SIGNATURES["dh_attn_cross_pack"]) == 10 and len(_abi.SIGNATURES["dh_attn_cross_decode_packed"]) == 15
    lib = ctypes.CDLL(_build.build())
    lib.dh_abi_version.restype = ctypes.c_int
    lib.dh_option_count.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35 and lib.dh_option_count() == 15
