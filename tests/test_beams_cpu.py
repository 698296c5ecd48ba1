"""n-best output (``return_beams=True``) without a GPU: the ABI of ``dh_beam_finalize_beams``, the ``BeamCaptions`` type, argument
validation, the multi-rank gather, the text helper, and golden G19 pinned to the CPU restatement of the reference."""
import ctypes
import datetime
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import KINDS, PREFIX, captions_and_lengths, golden, synthetic_sd, synth_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G5_KW = dict(max_len=12, beam_size=3, top_k=20, temperature=1.3)


def g19_cases(kind):
    """(tag, image index, caption prefix or None) of the cases golden G19 holds for ``kind``."""
    cases = [("0", 0, None), ("1", 1, None)]
    if kind in ("CaptioningLSTM", "CaptioningTransformer"):
        cases.append(("prefix_0", 0, PREFIX))
    return cases


def test_abi_header_table_and_library_agree():
    from deephumor_amd import _abi, _build
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+dh_beam_finalize_beams\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "dh_beam_finalize_beams is not declared in the header"
    assert len(m.group(1).split(",")) == len(_abi.SIGNATURES["dh_beam_finalize_beams"]) == 26
    assert "rnn_models.py:139-141" in header and "transformers.py:571-577" in header
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION >= 33
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, "dh_beam_finalize_beams") and hasattr(lib, "dh_beam_finalize")
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == version
    # the argument contract is checked before anything is launched
    from deephumor_amd import hip
    args = [0.0 if t is ctypes.c_float else (None if t is ctypes.c_void_p else 0) for t in _abi.SIGNATURES["dh_beam_finalize_beams"]]
    assert getattr(hip.load(), "dh_beam_finalize_beams")(*args) != 0


def _toy_beams():
    from deephumor_amd.models.beam import BeamCaptions
    tokens = torch.arange(2 * 3 * 5).view(2, 3, 5)
    return BeamCaptions(tokens, torch.tensor([[5, 3, 4], [2, 5, 5]]), torch.tensor([[-1.0, -2.5, -3.0], [-0.5, -0.75, float("-inf")]]),
                        torch.tensor([[2, 0, 1], [0, 1, 2]]), torch.tensor([1, 0]), torch.tensor([5, 4]))


def test_beam_captions_best_and_helpers():
    from deephumor_amd.models.beam import BeamCaptions
    b = _toy_beams()
    toks, lens = b.best()
    assert torch.equal(toks, torch.stack([b.tokens[0, 1], b.tokens[1, 0]])) and torch.equal(lens, torch.tensor([5, 4]))
    assert b._fields == ("tokens", "lengths", "scores", "beam_index", "drawn", "row_lengths")
    both = BeamCaptions.cat([b, b])
    assert both.tokens.shape == (4, 3, 5) and both.drawn.tolist() == [1, 0, 1, 0]
    c = b.map(torch.Tensor.clone)
    assert all(torch.equal(x, y) and x.data_ptr() != y.data_ptr() for x, y in zip(b, c))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_non_bool_return_beams_is_a_type_error_before_the_encoder(kind):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    model.encode = boom
    images = torch.zeros(1, 3, 224, 224)
    for bad in (1, "yes", None, torch.tensor(True)):
        with pytest.raises(TypeError):
            model.generate_batch(images, return_beams=bad)
        with pytest.raises(TypeError):
            model.generate(images, return_beams=bad)
        with pytest.raises(TypeError):
            model.generate_batch_graphed(images, return_beams=bad)
    dec = model.decoder
    with pytest.raises(TypeError):
        if kind == "CaptioningLSTM":
            dec.generate_batch(torch.zeros(1, 256), return_beams=1)
        else:
            dec.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), return_beams=1)


def _fake_beams(lo, hi, b=3, t=6):
    """Stands in for generate_batch(..., return_beams=True): every field a pure function of the GLOBAL image index."""
    from deephumor_amd.models.beam import BeamCaptions
    idx = torch.arange(lo, hi)
    toks = (idx[:, None, None] * 100 + torch.arange(b)[None, :, None] * 10 + torch.arange(t)[None, None, :]) % 97
    lens = (idx[:, None] + torch.arange(b)[None, :]) % t + 1
    scores = -(idx[:, None].float() * 0.37 + torch.arange(b)[None, :].float() * 1.0000001 + 1e-30)
    scores[:, -1] = float("-inf")                    # a dead beam
    scores[idx % 2 == 1, 0] = -1.1754944e-38 * 0.5   # a subnormal: bit patterns, not values, travel
    index = (torch.arange(b)[None, :] + idx[:, None]) % b
    return BeamCaptions(toks, lens, scores, index, idx % b, lens.max(1).values)


def _gather_worker(rank, world, port, n_total, ret):
    from deephumor_amd.dist import gather_beams, generate_micro_sharded, generate_sharded, shard_range
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    calls = []
    orig = dist.all_gather_into_tensor

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    dist.all_gather_into_tensor = counted
    a = generate_sharded(_fake_beams, n_total)
    n_one = len(calls)
    b = gather_beams(_fake_beams(*shard_range(n_total, rank, world)), n_total)
    c = generate_micro_sharded(_fake_beams, n_total, 4)
    ret[rank] = (tuple(t.clone() for t in a), tuple(t.clone() for t in b), tuple(t.clone() for t in c), n_one)
    dist.barrier()
    dist.destroy_process_group()


def test_gather_beams_two_ranks_uneven_shards_bit_for_bit():
    from test_dist_cpu import _free_port
    for n_total in (7, 8):
        with mp.Manager() as mgr:
            ret = mgr.dict()
            mp.spawn(_gather_worker, args=(2, _free_port(), n_total, ret), nprocs=2, join=True)
            want = _fake_beams(0, n_total)
            for r in range(2):
                a, b, c, n_one = ret[r]
                assert n_one == 1                                   # one all_gather_into_tensor per batch
                for got in (a, b, c):
                    for name, x, y in zip(want._fields, got, want):
                        assert x.dtype == y.dtype and x.shape == y.shape, name
                        if name == "scores":
                            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
                            assert torch.isinf(x[:, -1]).all()
                        else:
                            assert torch.equal(x, y), name


def test_beams_to_texts_on_a_toy_vocabulary():
    from deephumor_amd.experiments import beams_to_texts
    from deephumor_amd.models.beam import BeamCaptions

    class Vocab:
        itos = ["<pad>", "<unk>", "<bos>", "<eos>", "such", "wow", "much", "kernel"]
        stoi = {t: i for i, t in enumerate(itos)}
    tokens = torch.tensor([[[4, 5, 3, 0], [6, 7, 4, 5]], [[5, 3, 6, 3], [7, 7, 7, 3]]])
    beams = BeamCaptions(tokens, torch.tensor([[3, 2], [2, 4]]), torch.tensor([[-0.5, -1.5], [-0.25, float("-inf")]]),
                         torch.tensor([[0, 1], [1, 0]]), torch.tensor([0, 1]), torch.tensor([4, 4]))
    texts = beams_to_texts(beams, Vocab)
    assert texts[0] == [("such wow", -0.5), ("much kernel", -1.5)]            # cut at the row's own length, then before <eos>
    assert texts[1] == [("wow", -0.25), ("kernel kernel kernel", float("-inf"))]


def _oracle_beams(R, kind, sd, hp, image, label, seed, caption):
    """Every row the restatement's final draw chooses from: the recorder's forcing trick on ``BeamBook.draw`` (its ``n == 1``
    call is the final draw, ref_path.py:231 / :331)."""
    orig = R.BeamBook.draw
    state = {}

    def run(force):
        def draw(book, scores, n):
            if n != 1:
                return orig(book, scores, n)
            state["scores"] = scores.detach().reshape(-1).clone()
            ind = orig(book, scores, n)
            state["drawn"] = int(ind.reshape(-1)[0])
            return ind if force is None else torch.full_like(ind, force)
        R.BeamBook.draw = draw
        try:
            torch.manual_seed(seed)
            return R.model_generate(kind, sd, hp, image, label, caption=caption, **G5_KW).reshape(-1).numpy()
        finally:
            R.BeamBook.draw = orig
    out = run(None)
    scores, drawn = state["scores"].numpy(), state["drawn"]
    rows = np.stack([run(j) for j in range(G5_KW["beam_size"])])
    return rows, scores, drawn, out


@pytest.mark.parametrize("kind", KINDS)
def test_g19_is_pinned_to_the_restatement(kind, monkeypatch):
    """The committed G19 arrays (recorded from the real reference by tools/make_beams_golden.py) re-derived from
    ``oracle.ref_path.model_generate``: rows, draw and output exact, scores to the restatement's fp32 agreement with the reference."""
    from oracle import ref_path as R
    g = golden(f"g19_beams_{kind}.npz")
    sd, hp = synthetic_sd(kind)
    images = synth_images(4, seed=0)
    _, _, labels = captions_and_lengths()
    cache = {}
    encode = R._encode

    def encode_once(kind_, sd_, images_, labels_):       # the forced re-runs share one encoder pass per image
        key = (kind_, images_.data_ptr())
        if key not in cache:
            cache[key] = encode(kind_, sd_, images_, labels_)
        return cache[key]
    monkeypatch.setattr(R, "_encode", encode_once)
    for tag, i, cap in g19_cases(kind):
        lab = labels[i:i + 1] if "WithLabels" in kind else None
        img = images[i:i + 1]
        rows, scores, drawn, out = _oracle_beams(R, kind, sd, hp, img, lab, int(g[f"seed_{tag}"]), cap)
        assert rows.tolist() == g[f"rows_{tag}"].tolist(), (kind, tag)
        assert drawn == int(g[f"drawn_{tag}"]) and out.tolist() == g[f"out_{tag}"].tolist()
        np.testing.assert_allclose(scores, g[f"scores_{tag}"], rtol=0, atol=1e-4)
        assert len(set(g[f"scores_{tag}"].tolist())) == G5_KW["beam_size"]           # the order is unambiguous
        assert int(g[f"first_col_{tag}"]) == (0 if cap is None else cap.shape[1])


def test_g19_meets_the_recorder_conditions():
    varied = not_top = 0
    for kind in KINDS:
        g = golden(f"g19_beams_{kind}.npz")
        for tag, _, cap in g19_cases(kind):
            first = 0 if cap is None else cap.shape[1]
            lens = set()
            for row in g[f"rows_{tag}"]:
                hits = np.nonzero(row[first:] == 3)[0]
                lens.add(first + int(hits[0]) + 1 if hits.size else len(row))
            varied += len(lens) > 1
            not_top += int(g[f"drawn_{tag}"]) != int(np.argmax(g[f"scores_{tag}"]))
    assert varied >= 1 and not_top >= 1
