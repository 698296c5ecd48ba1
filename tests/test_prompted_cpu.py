"""Prompted batches (``generate_batch(..., caption=C, caption_lengths=L)``), the part that needs no GPU: the validation function, the
keyword-only interface, the host text step, the ABI table, and the fixture ``g19_prompted.npz`` against the CPU oracle."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, KINDS, golden, synthetic_sd, synth_images


def test_check_prompts_raises_on_every_invalid_combination():
    from deephumor_amd.models.beam import check_prompts
    cap = torch.randint(6, 100, (3, 5))
    ok = check_prompts(cap, torch.tensor([0, 5, 2]), 32, 100)
    assert ok.dtype == torch.int64 and ok.tolist() == [0, 5, 2]
    assert check_prompts(cap, torch.tensor([0, 5, 2], dtype=torch.int32), 32, 100).tolist() == [0, 5, 2]
    assert check_prompts(cap, None, 32, 100) is None and check_prompts(None, None, 32, 100) is None
    with pytest.raises(ValueError, match="without caption"):
        check_prompts(None, torch.tensor([0, 1, 2]), 32, 100)
    for bad in (torch.tensor([1, 2]), torch.tensor([[1, 2, 3]]), torch.tensor(2)):
        with pytest.raises(ValueError, match="shape"):
            check_prompts(cap, bad, 32, 100)
    with pytest.raises(ValueError, match="shape"):
        check_prompts(cap[0], torch.tensor([1]), 32, 100)                     # caption must be [N, P]
    with pytest.raises(ValueError, match="int64 or int32"):
        check_prompts(cap, torch.tensor([1.0, 2.0, 3.0]), 32, 100)
    for bad in ([0, 6, 2], [-1, 2, 2]):
        with pytest.raises(ValueError, match=r"\[0, 5\]"):
            check_prompts(cap, torch.tensor(bad), 32, 100)
    # no decode step left: L + 1 >= max_len
    with pytest.raises(ValueError, match="no decode step"):
        check_prompts(cap, torch.tensor([0, 5, 2]), 6, 100)
    assert check_prompts(cap, torch.tensor([0, 5, 2]), 7, 100).tolist() == [0, 5, 2]


def test_ids_are_checked_over_the_used_part_of_each_row_only():
    from deephumor_amd.models.beam import check_ids, check_prompts
    cap = torch.tensor([[7, 8, 10 ** 6, -5], [9, 9, 9, 9], [-1, 500, 500, 500]])
    lens = torch.tensor([2, 4, 0])
    check_prompts(cap, lens, 32, 100)                                         # the bad ids all lie in the ignored tails
    check_ids(cap, 100, lengths=lens)
    with pytest.raises(IndexError):
        check_ids(cap, 100)                                                   # the dense call looks at everything, as before
    with pytest.raises(IndexError):
        check_prompts(cap, torch.tensor([3, 4, 0]), 32, 100)
    with pytest.raises(IndexError):
        check_prompts(cap, torch.tensor([2, 4, 1]), 32, 100)
    with pytest.raises(IndexError):
        check_prompts(cap, lens, 32, 9)                                       # 9 is outside a 9-token vocabulary
    check_prompts(torch.zeros((2, 0), dtype=torch.int64), torch.tensor([0, 0]), 32, 100)


def test_options_out_of_scope_raise():
    from deephumor_amd.models.beam import prompt_session_inputs
    cap, lens = torch.randint(6, 100, (2, 4)), torch.tensor([1, 4])
    with pytest.raises(ValueError, match="Philox"):
        prompt_session_inputs(cap, lens, 32, 100, "cpu", rng="torch")
    with pytest.raises(ValueError, match="Philox"):
        prompt_session_inputs(cap, lens, 32, 100, "cpu", noise_source=lambda *a: None)
    assert prompt_session_inputs(cap, None, 32, 100, "cpu", rng="torch") is None          # dense calls are not touched
    c, fp, host = prompt_session_inputs(cap[:, :3], torch.tensor([1, 3]), 5, 100, "cpu")
    assert c.shape == (2, 3) and fp.dtype == torch.int32 and fp.tolist() == [1, 3] and host == [1, 3]
    import deephumor_amd.models as M
    model = M.CaptioningTransformer(100, n_layers=1, pad_index=1)
    with pytest.raises(NotImplementedError, match="pad_index == 1"):
        model.generate_batch(torch.zeros(2, 3, 224, 224), caption=cap, caption_lengths=lens)
    with pytest.raises(ValueError, match="Philox"):                          # validated before the encoder runs: no GPU needed
        M.CaptioningLSTM(100).generate_batch(torch.zeros(2, 3, 224, 224), caption=cap, caption_lengths=lens, rng="torch")
    with pytest.raises(ValueError, match="without caption"):
        M.CaptioningLSTM(100).generate_batch(torch.zeros(2, 3, 224, 224), caption_lengths=lens)
    with pytest.raises(ValueError, match="no decode step"):
        M.CaptioningLSTMWithLabels(100).generate_batch(torch.zeros(2, 3, 224, 224), torch.zeros(2, 3, dtype=torch.long), caption=cap,
                                                       caption_lengths=lens, max_len=5)


def test_caption_lengths_is_keyword_only_wherever_it_was_added():
    import deephumor_amd.models as M
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder
    fns = [getattr(getattr(M, kind), name) for kind in KINDS for name in ("generate_batch", "decode", "generate_batch_graphed")]
    fns += [LSTMDecoder.generate_batch, TransformerDecoder.generate_batch, SelfAttentionTransformerDecoder.generate_batch]
    for fn in fns:
        p = inspect.signature(fn).parameters["caption_lengths"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    # ... and nowhere else: the single-image methods keep the reference's signature
    for kind in KINDS:
        assert "caption_lengths" not in inspect.signature(getattr(M, kind).generate).parameters
    # no positional argument moved
    assert list(inspect.signature(M.CaptioningLSTM.generate_batch).parameters)[:8] == [
        "self", "images", "caption", "max_len", "temperature", "beam_size", "top_k", "eos_index"]
    assert list(inspect.signature(LSTMDecoder.generate_batch).parameters)[:19] == [
        "self", "image_emb", "caption", "max_len", "temperature", "beam_size", "top_k", "eos_index", "seed", "img0", "noise_source",
        "logits_hook", "streams", "seed_tensor", "defer_check", "early_stop_every", "exact", "rng", "caption_lengths"]


def test_prompts_to_batch():
    from deephumor_amd.data import SPECIAL_TOKENS, WordPunctTokenizer, build_vocab
    from deephumor_amd.experiments import prompts_to_batch
    from deephumor_amd.experiments.inference import text_to_seq
    G = json.load(open(os.path.join(GOLDEN, "g8_text_and_metrics.json")))
    tok = WordPunctTokenizer()
    vocab = build_vocab(G["docs"], tok, min_df=2)
    texts = [c["text"] for c in G["cases"]]
    eos = SPECIAL_TOKENS["EOS"]
    batch = texts + [None, "", texts[0] + " " + eos]
    cap, lens = prompts_to_batch(batch, vocab, tok)
    assert cap.dtype == torch.int64 and lens.dtype == torch.int64 and cap.shape == (len(batch), int(lens.max()))
    for i, c in enumerate(G["cases"]):
        assert cap[i, :int(lens[i])].tolist() == c["word_seq"] == text_to_seq(c["text"], vocab, tok)[0].tolist()
        assert (cap[i, int(lens[i]):] == vocab.stoi[SPECIAL_TOKENS["PAD"]]).all()
    n = len(texts)
    assert lens[n:n + 2].tolist() == [0, 0]
    with_eos = text_to_seq(batch[-1], vocab, tok)[0].tolist()
    if with_eos and with_eos[-1] == vocab.stoi[eos]:           # (the tokenizer keeps "<eos>" whole): stripped, as the notebook does
        assert cap[-1, :int(lens[-1])].tolist() == with_eos[:-1]
    else:
        assert cap[-1, :int(lens[-1])].tolist() == with_eos
    empty, zero = prompts_to_batch([None, ""], vocab, tok)
    assert empty.shape == (2, 0) and zero.tolist() == [0, 0]


def test_abi_table_holds_the_prompted_entry_points():
    import re
    from deephumor_amd import _abi
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "deephumor_hip.h")).read()
    assert int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1)) == _abi.ABI_VERSION >= 32
    dense = {"dh_beam_row_sample_prompted": "dh_beam_row_sample", "dh_beam_row_sample_exact_prompted": "dh_beam_row_sample_exact",
             "dh_beam_row_sample_groups_prompted": "dh_beam_row_sample_groups", "dh_beam_select_prompted": "dh_beam_select"}
    for name, twin in dense.items():
        assert name in _abi.SIGNATURES and re.search(r"\bint\s+%s\s*\(" % name, header), name
        # samplers: first_pos is one more pointer; select: the int `first` became a pointer
        extra = 0 if name == "dh_beam_select_prompted" else 1
        assert len(_abi.SIGNATURES[name]) == len(_abi.SIGNATURES[twin]) + extra
    sel, twin = _abi.SIGNATURES["dh_beam_select_prompted"], _abi.SIGNATURES["dh_beam_select"]
    changed = [i for i, (a, b) in enumerate(zip(sel, twin)) if a is not b]
    assert changed == [14] and sel[14] is _abi._P and twin[14] is _abi._I


def test_prompted_entry_points_reject_bad_arguments_without_a_gpu():
    from deephumor_amd import hip
    lib = hip.load()
    # a NULL first_pos, and rows_per_img != beam, are argument errors (code 1) before anything is launched
    assert lib.dh_beam_row_sample_prompted(1, 16, 10, 3, 3, 3, 5, 1.0, 1, None, 0, None, 0, 0, None, 1, 1, 1, None) == 1
    assert lib.dh_beam_row_sample_prompted(1, 16, 10, 4, 2, 3, 5, 1.0, 1, None, 0, None, 0, 0, 1, 1, 1, 1, None) == 1
    assert lib.dh_beam_select_prompted(1, 1, 1, 8, 1, 1, None, 0, 1, 1, 1, 1, 2, 3, None, 0, 0, 0, 0, 1.0, 3, None, 0, None, 0, None) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_g19_prompted_fixture_matches_the_oracle(kind):
    """``g19_prompted.npz`` (recorded from the real reference by ``tools/make_prompted_golden.py``): the CPU oracle returns the same
    greedy caption for every image under its own prompt, and sees the recorded top-2 margins."""
    from oracle import ref_path as R
    g = golden("g19_prompted.npz")
    assert g["lengths"].tolist() == [0, 1, 3, 3, 7, 12, 5, 0]
    sd, hp = synthetic_sd(kind)
    images = synth_images(8, seed=0)
    prompts, labels = torch.from_numpy(g["prompts"]), torch.from_numpy(g["labels"])
    assert int(prompts.min()) >= 6 and int(prompts.max()) < hp["num_tokens"]
    for i, n in enumerate(g["lengths"].tolist()):
        trace = []
        ids = R.model_generate(kind, sd, hp, images[i:i + 1], label=labels[i:i + 1] if "WithLabels" in kind else None,
                               caption=prompts[i:i + 1, :n] if n else None, max_len=32, beam_size=1, top_k=1, trace=trace)
        assert ids.reshape(-1).tolist() == g[f"{kind}_ids_{i}"].tolist(), (kind, i)
        margins = np.array([float(t["top2_val"][0, 0] - t["top2_val"][0, 1]) for t in trace])
        np.testing.assert_allclose(margins, g[f"{kind}_margins_{i}"], atol=1e-4)
        assert float(g[f"{kind}_margins_{i}"].min()) >= float(g["min_margin"][0]) - 1e-7
