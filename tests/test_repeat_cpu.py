"""``no_repeat_ngram_size`` / ``repetition_penalty`` without a GPU: the restatement (``tests/repeat_ref.py``) against its brute-force
scan and on its edge cases, ``beam.check_repeat`` on every public entry before the encoder runs, the signatures, the ABI of
``dh_beam_history_logits`` and its argument contract, and golden G21's own rule."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import KINDS, golden, synthetic_sd
from repeat_ref import banned_tokens, brute_edit_row, edit_logits, repeated_ngrams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dh_beam_history_logits"
INF = float("inf")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bit-level equality up to the sign of zero and the payload of NaN (``torch.equal`` semantics plus NaN == NaN)."""
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("penalty", [1.0, 1.3, 0.8])
def test_restatement_equals_the_brute_force_scan(n, penalty):
    g = torch.Generator().manual_seed(100 * n + int(penalty * 10))
    for v, L, alphabet in ((130, 37, 6), (200, 9, 3), (70, 64, 70), (130, 5, 140)):
        rows = 5
        logits = torch.randn(rows, v, generator=g) * 3
        logits[0, :4] = torch.tensor([0.0, -0.0, -INF, -2.5])
        hist = torch.randint(0, alphabet, (rows, L + 3), generator=g)
        hist[1, 2] = -4                                            # ids outside [0, V)
        hist[2, 1] = v + 7
        gm0 = torch.full((rows, (v + 63) // 64 + 1), 777.0)         # poison: one word more than there are groups
        out, gm, stored = edit_logits(logits, hist, L, n, penalty, gm0, 64)
        for r in range(rows):
            bx, bgm, bst = brute_edit_row(logits[r], hist[r, :L].tolist(), n, penalty, gm0[r], 64)
            assert same(out[r], bx), (v, L, r)
            assert torch.equal(gm[r], bgm) and stored[r].nonzero().flatten().tolist() == bst
        assert bool((gm[:, -1] == 777.0).all())


def test_short_histories():
    x = torch.arange(8.0)[None, :]
    h = torch.tensor([[3, 3, 3, 5, 3, 5]])
    # L < n - 1 and L == n - 1: nothing is banned (no complete n-gram lies in the history yet)
    for L, n in ((0, 1), (0, 2), (1, 3), (2, 3), (1, 2), (3, 4)):
        out, _, stored = edit_logits(x, h, L, n)
        assert torch.equal(out, x) and not stored.any(), (L, n)
        assert banned_tokens(h[0, :L].tolist(), n) == set()
    # L == n: one candidate start, j = 0
    assert banned_tokens([3, 3], 2) == {3} and banned_tokens([3, 5], 2) == set() and banned_tokens([3, 3, 3], 3) == {3}
    out, _, _ = edit_logits(x, h, 2, 2)
    assert out[0, 3] == -INF and int(torch.isinf(out).sum()) == 1
    # n == 1 bans every token of the history
    out, _, stored = edit_logits(x, h, 6, 1)
    assert stored[0].nonzero().flatten().tolist() == [3, 5] and bool((out[0, [3, 5]] == -INF).all())
    # the classic: "3 5 3 5 3" + 5 would repeat the bigram (3, 5)
    assert banned_tokens([3, 5, 3], 2) == {5} and banned_tokens([3, 5, 3, 5, 3], 3) == {5} and banned_tokens([1, 2, 3, 4], 2) == set()


def test_penalty_once_per_distinct_token_and_special_values():
    x = torch.tensor([[0.0, -2.0, 3.0, -INF, 5.0, -0.5]])
    h = torch.tensor([[2, 2, 2, 2, 1, 0, 3, 2, 9, -1]])             # token 2 five times; ids 9 and -1 lie outside [0, 6)
    out, gm, stored = edit_logits(x, h, 10, 0, 1.3, torch.full((1, 1), 777.0), 64)
    p = torch.tensor(1.3, dtype=torch.float32)
    assert out[0, 2] == torch.tensor(3.0) / p                      # once, not (3 / 1.3) / 1.3 ...
    assert out[0, 1] == torch.tensor(-2.0) * p and out[0, 0] == 0.0 and out[0, 3] == -INF
    assert out[0, 4] == 5.0 and out[0, 5] == -0.5                  # not in the history
    assert stored[0].tolist() == [True, True, True, True, False, False]
    assert gm[0, 0] == 5.0
    # penalty < 1 RAISES a positive logit: the group maximum goes up
    out, gm, _ = edit_logits(x, torch.tensor([[4]]), 1, 0, 0.8, torch.full((1, 1), 5.0), 64)
    assert out[0, 4] == torch.tensor(5.0) / torch.tensor(0.8) and gm[0, 0] == out[0, 4] and gm[0, 0] > 5.0
    # penalty first, ban second: a banned column is -inf whatever the penalty did
    out, _, _ = edit_logits(x, torch.tensor([[2, 2]]), 2, 2, 0.5)
    assert out[0, 2] == -INF
    # a group whose columns are all banned
    out, gm, _ = edit_logits(torch.zeros(1, 70), torch.arange(64)[None, :], 64, 1, 1.0, torch.full((1, 2), 777.0), 64)
    assert gm[0].tolist() == [-INF, 777.0]
    # inactive rows keep every word
    out, gm, stored = edit_logits(x.repeat(2, 1), h.repeat(2, 1), 10, 1, 1.3, torch.full((2, 1), 777.0), 64, active=torch.tensor([False, True]))
    assert torch.equal(out[0], x[0]) and gm[0, 0] == 777.0 and not stored[0].any() and stored[1].any()


# ---- validation -----------------------------------------------------------------------------------------------------------------
def test_check_repeat():
    from deephumor_amd import hip
    from deephumor_amd.models.beam import check_repeat
    assert check_repeat() == (0, 1.0) and check_repeat(3, 1) == (3, 1.0) and check_repeat(np.int64(2), np.float32(0.5)) == (2, 0.5)
    assert isinstance(check_repeat(2, 1)[1], float) and isinstance(check_repeat(np.int32(2))[0], int)
    for bad in (True, False, -1):
        with pytest.raises(ValueError):
            check_repeat(bad)
    for bad in (2.0, "2", None, [2], torch.tensor(2)):
        with pytest.raises(TypeError):
            check_repeat(bad)
    for bad in (True, False, 0, 0.0, -1.3, float("nan"), INF):
        with pytest.raises(ValueError):
            check_repeat(0, bad)
    for bad in ("1.3", None, [1.3], torch.tensor(1.3), 1.3 + 0j):
        with pytest.raises(TypeError):
            check_repeat(0, bad)
    # a history longer than the kernel looks at: only with a control on
    assert hip.MAX_HISTORY >= 256
    check_repeat(0, 1.0, hip.MAX_HISTORY + 1)
    check_repeat(2, 1.3, hip.MAX_HISTORY)
    for n, p in ((2, 1.0), (0, 1.3)):
        with pytest.raises(ValueError, match="max_len"):
            check_repeat(n, p, hip.MAX_HISTORY + 1)


BAD = (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=True), dict(repetition_penalty=0), dict(repetition_penalty=float("nan")),
       dict(repetition_penalty=True), dict(no_repeat_ngram_size=2, max_len=5000), dict(repetition_penalty=1.2, max_len=5000))
BAD_TYPE = (dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size="2"), dict(repetition_penalty="1.3"))


@pytest.mark.parametrize("kind", ("CaptioningLSTM", "CaptioningTransformer"))
def test_bad_values_fail_before_the_encoder(kind):
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**hp).eval()                    # (CaptionPipeline needs a device: tests/test_repeat_gpu.py)

    def boom(*a, **k):
        raise AssertionError("the encoder ran")
    model.encode = boom
    images = torch.zeros(1, 3, 224, 224)
    for group, exc in ((BAD, ValueError), (BAD_TYPE, TypeError)):
        for bad in group:
            for call in (model.generate_batch, model.generate, model.generate_batch_graphed):
                with pytest.raises(exc):
                    call(images, **bad)
            with pytest.raises(exc):
                model.decode((None,) if kind == "CaptioningLSTM" else (None, None), **bad)    # (the decoder's own check)
            with pytest.raises(exc):
                if kind == "CaptioningLSTM":
                    model.decoder.generate_batch(torch.zeros(1, 256), **bad)
                else:
                    model.decoder.generate_batch(torch.zeros(1, 512), torch.zeros(1, 49, 512), **bad)


def test_keyword_only_and_positional_prefixes():
    import deephumor_amd.models as M
    from deephumor_amd.models.beam import BeamSearchHelper, DecodeSettings
    from deephumor_amd.models.rnn_models import LSTMDecoder
    from deephumor_amd.models.transformers import SelfAttentionTransformerDecoder, TransformerDecoder
    for name, default in (("no_repeat_ngram_size", 0), ("repetition_penalty", 1.0)):
        p = inspect.signature(LSTMDecoder.generate_batch).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
        assert getattr(DecodeSettings(), name) == default        # (the signatures and the keyword's way down: test_decode_settings_cpu)
        # everywhere else the keywords ride in **kw: they cannot be passed by position
        fns = [getattr(getattr(M, kind), fn) for kind in KINDS for fn in ("generate_batch", "decode", "generate", "generate_batch_graphed")]
        fns += [TransformerDecoder.generate_batch, SelfAttentionTransformerDecoder.generate_batch, LSTMDecoder.generate]
        for fn in fns:
            ps = inspect.signature(fn).parameters
            assert name not in ps and any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ps.values()), fn
    # no positional argument moved
    assert list(inspect.signature(M.CaptioningLSTM.generate_batch).parameters)[:8] == [
        "self", "images", "caption", "max_len", "temperature", "beam_size", "top_k", "eos_index"]
    names = list(inspect.signature(LSTMDecoder.generate_batch).parameters)
    assert names[:19] == ["self", "image_emb", "caption", "max_len", "temperature", "beam_size", "top_k", "eos_index", "seed", "img0",
                          "noise_source", "logits_hook", "streams", "seed_tensor", "defer_check", "early_stop_every", "exact", "rng",
                          "caption_lengths"]
    assert names[19:] == ["return_beams", "top_p", "no_repeat_ngram_size", "repetition_penalty", "kw"]
    names = list(inspect.signature(BeamSearchHelper.__init__).parameters)
    assert names[1:7] == ["temperature", "beam_size", "top_k", "unk_index", "eos_index", "device"]
    assert names[names.index("top_p") + 1:] == ["no_repeat_ngram_size", "repetition_penalty"]


def test_helper_keywords_and_method_surface():
    from deephumor_amd.models.beam import BeamSearchHelper
    h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu")
    assert (h.no_repeat_ngram_size, h.repetition_penalty) == (0, 1.0)
    logits = torch.zeros(3, 8)
    for kw in (dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.3)):
        h = BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", **kw)
        with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
            h.sample_k_indices(logits)
        with pytest.raises(NotImplementedError):
            h.process_logits(logits, torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", no_repeat_ngram_size=-2)
    with pytest.raises(ValueError):
        BeamSearchHelper(1.0, 3, 5, 1, 3, "cpu", max_len=5000, repetition_penalty=1.3)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_header_table_and_library_agree():
    from deephumor_amd import _abi, _build, hip
    header = open(os.path.join(ROOT, "include", "deephumor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NAME + " is not declared in the header"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = _abi.SIGNATURES[NAME]
    assert len(args) == len(sig) == 17
    for a, t in zip(args, sig):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int
        assert t is want, (a, t)
    assert [a.split()[-1].lstrip("*") for a in args] == ["logits", "ldl", "V", "group_max", "gm_ld", "n_groups", "group_cols", "tokens",
                                                          "tok_ld", "tok_row_mult", "pos", "rows", "rows_per_img", "first_pos", "ngram",
                                                          "penalty", "stream"]
    version = int(re.search(r"#define DH_ABI_VERSION (\d+)", header).group(1))
    assert version == _abi.ABI_VERSION == hip.ABI_VERSION == 35
    assert int(re.search(r"#define DH_BEAM_MAX_HISTORY (\d+)", header).group(1)) == _abi.MAX_HISTORY == hip.MAX_HISTORY
    lib = ctypes.CDLL(_build.build())
    assert hasattr(lib, NAME)
    lib.dh_abi_version.restype = ctypes.c_int
    assert lib.dh_abi_version() == 35
    # one new symbol, no prototype moved
    assert len(_abi.SIGNATURES["dh_beam_row_sample"]) == 18 and len(_abi.SIGNATURES["dh_beam_row_sample_groups"]) == 22
    assert len(_abi.SIGNATURES["dh_beam_row_sample_nucleus"]) == 25 and len(_abi.SIGNATURES["dh_beam_select"]) == 26


def test_entry_point_argument_contract():
    """Checked before any HIP call (pointers are never dereferenced on the host): every case returns DH_ERR_BAD_ARG."""
    from deephumor_amd import hip
    fn = getattr(hip.load(), NAME)
    #           logits ldl  V    gmax gm ng gc tokens tok_ld mult pos rows rpi first_pos ngram penalty stream
    good = [64, 128, 100, None, 0, 0, 0, 64, 12, 1, 5, 2, 1, None, 2, 1.3, None]

    def call(**over):
        names = ["logits", "ldl", "V", "group_max", "gm_ld", "n_groups", "group_cols", "tokens", "tok_ld", "tok_row_mult", "pos", "rows",
                 "rows_per_img", "first_pos", "ngram", "penalty", "stream"]
        a = list(good)
        for k, val in over.items():
            a[names.index(k)] = val
        return fn(*a)
    for over in (dict(ngram=-1), dict(penalty=0.0), dict(penalty=-1.3), dict(penalty=float("nan")), dict(penalty=INF),
                 dict(ngram=0, penalty=1.0), dict(pos=13), dict(pos=-1), dict(logits=None), dict(tokens=None),
                 dict(pos=hip.MAX_HISTORY + 1, tok_ld=4096), dict(tok_row_mult=0), dict(rows=0), dict(ldl=99),
                 dict(group_max=64, gm_ld=2, n_groups=1, group_cols=64),          # 64 columns of groups for V = 100
                 dict(group_max=64, gm_ld=1, n_groups=2, group_cols=64),          # gm_ld < n_groups
                 dict(group_max=64, gm_ld=2, n_groups=2, group_cols=65),
                 dict(group_max=64, gm_ld=2000, n_groups=1025, group_cols=64),
                 dict(first_pos=64, rows=3, rows_per_img=2)):
        assert call(**over) == 1, over


# ---- golden G21 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_g21_satisfies_its_own_rule(kind):
    g = golden(f"g21_repeat_{kind}.npz")
    assert int(g["n_configs"]) == 2
    assert (int(g["ngram_0"]), float(g["penalty_0"])) == (2, 1.0)
    assert int(g["ngram_1"]) == 3 and abs(float(g["penalty_1"]) - 1.3) < 1e-6
    assert int(g["max_len"]) == (6 if kind in ("CaptioningTransformer", "CaptioningTransformerWithLabels") else 12)
    for c in range(2):
        n = int(g[f"ngram_{c}"])
        for slot in range(2):
            out = g[f"c{c}_out_{slot}"].tolist()
            assert 1 <= len(out) <= int(g["max_len"]) and not repeated_ngrams(out, n), (kind, c, slot, out)
            assert len(g[f"c{c}_plain_{slot}"].tolist()) >= 1 and int(g[f"c{c}_edited_{slot}"]) >= 0
    assert sum(int(g[f"c1_edited_{slot}"]) for slot in range(2)) > 0          # the penalty stores to every history token


def test_g21_differs_from_the_plain_captions():
    """At least one fixture caption is not the plain caption of its seed: G21 cannot pass without the feature."""
    n = 0
    for kind in KINDS:
        g = golden(f"g21_repeat_{kind}.npz")
        n += sum(g[f"c{c}_out_{s}"].tolist() != g[f"c{c}_plain_{s}"].tolist() for c in range(2) for s in range(2))
    assert n >= 1
