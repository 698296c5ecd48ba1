"""Batched, device-resident beam-search bookkeeping.

Mirror of ``deephumor.models.beam.BeamSearchHelper`` (reference beam.py:4-112): same constructor
arguments and the same selection rules, but the state of ALL images of a batch lives in HBM and
every step is two kernel launches (``dh_beam_row_sample`` + ``dh_beam_select``; opt-in one: ``dh_beam_step_groups``) with no host
synchronisation, instead of per-image torch ops and a ``torch.all`` sync per token.

Randomness: the reference draws with ``torch.multinomial`` from the global CPU generator.  On
CPU that is exactly "top-k of p / Exp(1) noise" (SURVEY.md section 7), so the kernels take the
noise either from a counter-based Philox stream keyed by ``(seed, global image index, step, row,
token)`` -- results do not depend on batch composition or rank layout -- or, for RNG-replay parity
tests, from caller-supplied tensors (``noise_source``).
"""
import dataclasses
import math
import numbers
import os
from typing import NamedTuple

import torch

from .. import hip


class BeamCaptions(NamedTuple):
    """What ``generate_batch(..., return_beams=True)`` returns: EVERY beam the search holds at its end (the plain call draws one of
    them and drops the rest), per image in descending order of score.  Device tensors, ``N`` images, ``B = beam_size`` slots,
    ``T`` = the width of the plain call's ``tokens``:

    ``tokens`` int64 ``[N, B, T]``   slot ``j`` of image ``i`` is a complete beam row (padded like the plain call's row);
    ``lengths`` int64 ``[N, B]``     the beam's OWN length: up to and including its first ``<eos>`` at or after the image's first
                                     generated column, never more than ``row_lengths[i]``; ``row_lengths[i]`` without one;
    ``scores`` float32 ``[N, B]``    the engine's ``vals`` -- the reference's cumulative ``sample_val`` -- non-increasing along ``B``
                                     (equal scores keep the engine's order; a dead beam, score ``-inf``, comes last);
    ``beam_index`` int64 ``[N, B]``  the engine beam each slot holds (a permutation of ``0 .. B-1``);
    ``drawn`` int64 ``[N]``          the slot of the beam the plain call returns (its final draw, same noise);
    ``row_lengths`` int64 ``[N]``    the plain call's ``lengths``.

    ``scores`` are re-normalised over the drawn candidates at every step (``log_softmax`` over each row's ``B`` picks, reference
    beam.py:79): they order the beams the way the search does, but are NOT model log-probabilities.  Those come with
    ``return_logprobs=True``: one more tensor behind the ``BeamCaptions``, ``logprobs`` fp32 ``[N, B, T]`` in this slot order --
    ``log_softmax(logits / temperature)`` at every token the search wrote, from the image's first generated column up to ``lengths``,
    exactly 0 elsewhere (``LSTMDecoder.generate_batch``) --, which ``experiments.beam_logprob_scores`` sums per candidate without a
    second decoder pass; ``experiments.rank_beams`` scores the raw model teacher-forced instead.

    Under ``search="beam"`` nothing is drawn and nothing is re-normalised: ``scores`` ARE the beams' cumulative model log-probabilities
    (the sum over the beam's generated tokens of ``log_softmax(logits / temperature)``, history edits and bans applied), slot 0 is the
    caption the plain call returns and ``drawn`` is 0 for every image."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    scores: torch.Tensor
    beam_index: torch.Tensor
    drawn: torch.Tensor
    row_lengths: torch.Tensor

    def best(self):
        """``(tokens [N, T], lengths [N])`` of the drawn beams: exactly the plain call's pair."""
        n = self.tokens.shape[0]
        return self.tokens[torch.arange(n, device=self.tokens.device), self.drawn], self.row_lengths

    def map(self, fn):
        """``BeamCaptions`` of ``fn(field)`` for every field (``clone``, ``cpu`` ...)."""
        return BeamCaptions(*(fn(t) for t in self))

    @staticmethod
    def cat(parts):
        """The images of several results, in order."""
        return BeamCaptions(*(torch.cat(ts, 0) for ts in zip(*parts)))


def check_return_beams(return_beams):
    """``return_beams`` is a plain bool (a tensor or an int here is a misplaced positional argument): checked before anything runs."""
    if not isinstance(return_beams, bool):
        raise TypeError(f"return_beams must be a bool, not {type(return_beams).__name__}")
    return return_beams


def check_return_attention(return_attention, model=None):
    """``return_attention`` is a plain bool, checked where ``check_return_beams`` is, before anything runs.  With ``model`` (a captioning
    model or its decoder) and the keyword on: a decoder without encoder attention (the LSTM kinds, ``CaptioningTransformerBase``) has no
    map to return -- a ``TypeError`` that says so; ``pad_index == 1`` decodes by full re-forward on the module path, which keeps no
    per-position queries -- ``NotImplementedError``, as ``caption_lengths`` there."""
    if not isinstance(return_attention, bool):
        raise TypeError(f"return_attention must be a bool, not {type(return_attention).__name__}")
    if return_attention and model is not None:
        dec = getattr(model, "decoder", model)
        if not getattr(dec, "_cross", False):
            raise TypeError(f"return_attention: {type(model).__name__} has no encoder attention (only CaptioningTransformer and "
                            "CaptioningTransformerWithLabels attend over the image features)")
        if getattr(dec, "pad_index", 0) == 1:
            raise NotImplementedError("return_attention with pad_index == 1: that decoder re-runs the whole sequence per token on the "
                                      "module path (_generate_reforward), which keeps no per-position attention weights")
    return return_attention


def check_return_logprobs(return_logprobs, model=None):
    """``return_logprobs`` is a plain bool, checked where ``check_return_attention`` is, before anything runs.  Every decoder kind has
    logits, so with ``model`` (a captioning model or its decoder) and the keyword on only ``pad_index == 1`` is refused: that decoder
    re-runs the whole sequence per token on the module path -- ``NotImplementedError``, as ``return_attention`` there."""
    if not isinstance(return_logprobs, bool):
        raise TypeError(f"return_logprobs must be a bool, not {type(return_logprobs).__name__}")
    if return_logprobs and model is not None:
        dec = getattr(model, "decoder", model)
        if getattr(dec, "pad_index", 0) == 1:
            raise NotImplementedError("return_logprobs with pad_index == 1: that decoder re-runs the whole sequence per token on the "
                                      "module path (_generate_reforward), which records no per-token log-probabilities")
    return return_logprobs


def check_top_p(top_p):
    """``top_p`` is a real number in ``(0, 1]`` (1.0: no nucleus, today's kernels): checked where ``check_return_beams`` is, before
    anything runs.  A ``bool`` is a misplaced flag, not a probability.  Returns it as a float."""
    if isinstance(top_p, bool):
        raise ValueError("top_p must be a number in (0, 1], not a bool")
    if not isinstance(top_p, numbers.Real):
        raise TypeError(f"top_p must be a real number in (0, 1], not {type(top_p).__name__}")
    top_p = float(top_p)
    if math.isnan(top_p) or not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
    return top_p


SEARCHES = ("sample", "beam")


def check_search(search, top_p=1.0):
    """``search`` is the ``str`` ``"sample"`` (the reference's sampled search, the default) or ``"beam"`` (the ``beam_size`` most likely
    continuations, no noise): anything that is not a ``str`` is a ``TypeError``, another string a ``ValueError`` that names the two.
    ``"beam"`` with ``top_p < 1`` is a ``ValueError``: a nucleus restricts a draw, and nothing is drawn there.  Returns it."""
    if not isinstance(search, str):
        raise TypeError(f'search must be "sample" or "beam", not {type(search).__name__}')
    if search not in SEARCHES:
        raise ValueError(f'search must be "sample" or "beam", got {search!r}')
    if search == "beam" and top_p < 1.0:
        raise ValueError(f'search="beam" keeps the most likely tokens and draws nothing: top_p={top_p} (a nucleus) has no meaning there -- '
                         "use top_p=1.0")
    return search


MAX_LENGTH_PENALTY = 8.0


def length_weights(length_penalty, max_len):
    """The weight table of ``length_penalty``: ``w[0] = 1`` and ``w[L] = float32(float64(L) ** -length_penalty)`` for ``L = 1 ..
    max_len`` -- the power in fp64 on the host, rounded ONCE to fp32 -- as an fp32 CPU tensor of ``max_len + 1`` entries.  The select
    kernel multiplies by it and computes no power itself, so a CPU restatement is bit-exact."""
    w = [1.0] + [math.pow(float(n), -float(length_penalty)) for n in range(1, int(max_len) + 1)]
    return torch.tensor(w, dtype=torch.float64).to(torch.float32)


def check_length_penalty(length_penalty, max_len=None, search=None):
    """``length_penalty`` is a finite real number with ``abs(length_penalty) <= 8`` (0.0: off, the call without it; a ``bool`` or a
    non-number is a ``TypeError``): checked where ``check_search`` is, before anything runs.  With ``max_len``, a value for which some
    ``w[1 .. max_len]`` (``length_weights``) is not a normal, finite fp32 number is a ``ValueError``; with ``search``, a non-zero value
    under anything but ``"beam"`` is one too -- the sampled search draws its candidates and ranks nothing.  Returns it as a float."""
    lp = length_penalty
    if isinstance(lp, bool) or not isinstance(lp, numbers.Real):
        raise TypeError(f"length_penalty must be a real number, not {type(lp).__name__}")
    lp = float(lp)
    if not math.isfinite(lp) or abs(lp) > MAX_LENGTH_PENALTY:
        raise ValueError(f"length_penalty must be finite with abs(length_penalty) <= {MAX_LENGTH_PENALTY:g}, got {lp}")
    lp += 0.0                                               # (-0.0 is 0.0: one key, one graph)
    if lp != 0.0 and search is not None and search != "beam":
        raise ValueError(f'length_penalty={lp} belongs to search="beam" (it ranks the candidates the deterministic search keeps); '
                         f'search="{search}" draws its candidates and ranks nothing -- use length_penalty=0.0 there')
    if lp != 0.0 and max_len is not None:
        w = length_weights(lp, max_len)[1:]
        tiny = float(torch.finfo(torch.float32).tiny)
        if not bool((torch.isfinite(w) & (w >= tiny)).all()):
            raise ValueError(f"length_penalty={lp} at max_len={int(max_len)}: a weight L ** -length_penalty leaves the normal fp32 range")
    return lp


def check_early_stopping(early_stopping, search=None, return_attention=False, return_logprobs=False):
    """``early_stopping`` is ``None`` (off, the call without it), ``True`` or ``False`` -- both keep a finished-hypothesis pool; ``True``
    stops an image as soon as its pool is full, ``False`` when no live beam can still enter it --: anything else, 0 and 1 included, is a
    ``TypeError``; checked where ``check_length_penalty`` is, before anything runs.  With ``search``, a non-``None`` value under
    anything but ``"beam"`` is a ``ValueError``, like ``length_penalty``.  With ``return_attention`` / ``return_logprobs`` on it is a
    ``NotImplementedError``: both gathers walk tables from a live engine row, and a pooled hypothesis has none.  Returns it."""
    es = early_stopping
    if es is not None and not isinstance(es, bool):
        raise TypeError(f"early_stopping must be None, True or False, not {type(es).__name__} {es!r}")
    if es is None:
        return None
    if search is not None and search != "beam":
        raise ValueError(f'early_stopping={es} belongs to search="beam" (it pools the hypotheses the deterministic search finishes); '
                         f'search="{search}" draws its candidates and finishes none -- use early_stopping=None there')
    for name, on in (("return_attention", return_attention), ("return_logprobs", return_logprobs)):
        if on:
            raise NotImplementedError(f"early_stopping={es} with {name}=True: the gather walks its tables from a live engine row, and a "
                                      f"hypothesis in the pool has none -- the follow-up is a pool that records each entry's row tables; "
                                      f"use early_stopping=None with {name}")
    return es


MAX_DIVERSITY_PENALTY = 1e6     # times at most MAX_BEAMS earlier uses of a token: finite in fp32


def check_beam_groups(num_beam_groups=1, diversity_penalty=0.0, search=None, beam_size=None, early_stopping=None):
    """``num_beam_groups`` is an ``int >= 1`` (1: off, the call without it; a ``bool`` or a float is a ``TypeError``) and
    ``diversity_penalty`` a real number (no ``bool``; 0.0 with one group): checked behind ``check_early_stopping``, before anything
    runs.  With more than one group the penalty must be finite with ``0 < diversity_penalty <= 1e6`` -- without one every group
    repeats group 0 for ever, and the cap keeps ``diversity_penalty * beam_size`` finite in fp32 --; with one group a non-zero penalty
    is a ``ValueError`` (there is no earlier group to differ from).  With ``beam_size``, ``num_beam_groups`` must divide it (so it is
    ``<= beam_size``); with ``search``, more than one group under anything but ``"beam"`` is a ``ValueError``; with ``early_stopping``
    not ``None`` it is a ``NotImplementedError``: a pool per group is the follow-up.  Returns ``(int, float)``."""
    g, lam = num_beam_groups, diversity_penalty
    if isinstance(g, bool) or not isinstance(g, numbers.Integral):
        raise TypeError(f"num_beam_groups must be an int >= 1, not {type(g).__name__}")
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real):
        raise TypeError(f"diversity_penalty must be a real number, not {type(lam).__name__}")
    g, lam = int(g), float(lam)
    if g < 1:
        raise ValueError(f"num_beam_groups must be >= 1, got {g}")
    if beam_size is not None and (g > int(beam_size) or int(beam_size) % g != 0):
        raise ValueError(f"num_beam_groups must divide beam_size: num_beam_groups={g}, beam_size={int(beam_size)}")
    if g == 1:
        if lam != 0.0:
            raise ValueError(f"diversity_penalty={lam} needs num_beam_groups > 1: with one group there is no earlier group to differ from")
        return 1, 0.0
    if search is not None and search != "beam":
        raise ValueError(f'num_beam_groups={g} belongs to search="beam" (it splits the beams the deterministic search keeps into groups); '
                         f'search="{search}" draws its candidates -- use num_beam_groups=1 there')
    if not (math.isfinite(lam) and 0.0 < lam <= MAX_DIVERSITY_PENALTY):
        raise ValueError(f"num_beam_groups={g} needs a finite diversity_penalty with 0 < diversity_penalty <= {MAX_DIVERSITY_PENALTY:g} "
                         f"(without one every group repeats the first), got {lam}")
    if early_stopping is not None:
        raise NotImplementedError(f"num_beam_groups={g} with early_stopping={early_stopping}: the finished-hypothesis pool is one per image, "
                                  "and groups need one per group -- that is the follow-up; use early_stopping=None with groups")
    return g, lam


_LEN_W_CACHE = {}               # (device, length_penalty, max_len) -> fp32 device table: uploaded once, not once per session
_LEN_W_CACHE_SIZE = 16          # least recently used out; a table in use is owned by its helper (and by a captured graph's state)


def compile_length_weights(length_penalty, max_len, device="cuda"):
    """``length_weights`` on ``device``, uploaded once per ``(device, length_penalty, max_len)`` (a small cache, like
    ``compile_bad_words``; a hit makes the entry the most recently used one).  Not inside a hipGraph capture (a host-to-device copy):
    ``generate_batch_graphed`` uploads in front of it.  The cache owns a table only until it is evicted: whoever launches with it
    holds the tensor -- the helper for its session, a captured graph through ``held_length_weights``."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), float(length_penalty), int(max_len))
    w = _LEN_W_CACHE.get(key)
    if w is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("compile_length_weights inside a hipGraph capture: upload the table before the capture")
        w = length_weights(length_penalty, max_len).to(device)
        while len(_LEN_W_CACHE) >= _LEN_W_CACHE_SIZE:
            _LEN_W_CACHE.pop(next(iter(_LEN_W_CACHE)))
    else:
        _LEN_W_CACHE.pop(key)                               # most recently used last
    _LEN_W_CACHE[key] = w
    return w


def held_length_weights(length_penalty, device, early_stopping=None, num_beam_groups=1):
    """Every cached table of ``length_penalty`` on ``device``, for a captured hipGraph to keep: its ``dh_beam_select_best_norm`` nodes
    hold the raw pointer of the table their session found here, and the cache alone would free it at the next eviction.  ``()`` for
    0.0 -- unless ``early_stopping`` is on or ``num_beam_groups > 1``: ``dh_beam_select_pool`` / ``dh_beam_select_groups`` nodes point
    at the table of ones then."""
    if float(length_penalty) == 0.0 and early_stopping is None and int(num_beam_groups) == 1:
        return ()
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return tuple(w for (dev, lp, _), w in _LEN_W_CACHE.items() if dev == str(device) and lp == float(length_penalty))


def check_repeat(no_repeat_ngram_size=0, repetition_penalty=1.0, max_len=None):
    """``no_repeat_ngram_size`` is an ``int >= 0`` (0: off; a ``bool`` is a misplaced flag, a float a ``TypeError``) and
    ``repetition_penalty`` a finite real number ``> 0`` (1.0: off; no ``bool``): checked where ``check_top_p`` is, before anything
    runs.  With ``max_len`` and a control on, a history longer than the kernel looks at (``hip.MAX_HISTORY`` columns) is a
    ``ValueError`` here, not a failed launch in the middle of a batch.  Returns ``(int, float)``."""
    n, pen = no_repeat_ngram_size, repetition_penalty
    if isinstance(n, bool):
        raise ValueError("no_repeat_ngram_size must be an int >= 0, not a bool")
    if not isinstance(n, numbers.Integral):
        raise TypeError(f"no_repeat_ngram_size must be an int >= 0, not {type(n).__name__}")
    n = int(n)
    if n < 0:
        raise ValueError(f"no_repeat_ngram_size must be >= 0, got {n}")
    if isinstance(pen, bool):
        raise ValueError("repetition_penalty must be a finite number > 0, not a bool")
    if not isinstance(pen, numbers.Real):
        raise TypeError(f"repetition_penalty must be a finite real number > 0, not {type(pen).__name__}")
    pen = float(pen)
    if not (math.isfinite(pen) and pen > 0.0):
        raise ValueError(f"repetition_penalty must be finite and > 0, got {pen}")
    if max_len is not None and (n > 0 or pen != 1.0) and int(max_len) > hip.MAX_HISTORY:
        raise ValueError(f"no_repeat_ngram_size / repetition_penalty look at a row history of at most {hip.MAX_HISTORY} tokens "
                         f"(DH_BEAM_MAX_HISTORY): max_len={int(max_len)} is above it")
    return n, pen


class BadWords:
    """A banned-phrase list compiled for ``dh_beam_constrain_logits`` (``compile_bad_words``): ``ids`` -- a tuple of tuples of ints,
    the phrases as given, duplicates kept --, and two int32 tensors on ``device``, uploaded once: ``words`` (the phrases flat) and
    ``offsets`` (``n_words + 1`` entries; phrase ``w`` is ``words[offsets[w]:offsets[w + 1]]``).  Immutable; hashable and equal by
    ``ids`` and device, so it can sit in a graph cache key, and whoever holds it keeps the tensors alive."""
    __slots__ = ("ids", "num_tokens", "device", "words", "offsets")

    def __init__(self, ids, num_tokens, device, words, offsets):
        for name, val in zip(self.__slots__, (ids, num_tokens, device, words, offsets)):
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value):
        raise AttributeError("BadWords is immutable")

    def __delattr__(self, name):
        raise AttributeError("BadWords is immutable")

    @property
    def n_words(self):
        return len(self.ids)

    def __len__(self):
        return len(self.ids)

    def __hash__(self):
        return hash((self.ids, str(self.device)))

    def __eq__(self, other):
        return isinstance(other, BadWords) and self.ids == other.ids and str(self.device) == str(other.device)

    def __repr__(self):
        return f"BadWords({len(self.ids)} phrases, device={self.device})"


def _phrases(bad_words_ids, num_tokens=None, what="bad_words_ids"):
    """``bad_words_ids`` as a tuple of tuples of ints, every rule of ``check_constraints`` applied (``what``: the keyword the
    messages name -- ``check_sequence_bias`` checks its phrases here too)."""
    if isinstance(bad_words_ids, (str, bytes)) or not hasattr(bad_words_ids, "__iter__"):
        raise TypeError(f"bad_words_ids must be None or a sequence of sequences of token ids, not {type(bad_words_ids).__name__} "
                        "(strings go through experiments.bad_words_to_ids)")
    out = []
    for w, phrase in enumerate(bad_words_ids):
        if hasattr(phrase, "tolist"):                       # (a tensor or an array: its Python numbers)
            phrase = phrase.tolist()
        if isinstance(phrase, (str, bytes)) or not hasattr(phrase, "__iter__"):
            raise ValueError(f"{what}: phrase {w} ({phrase!r}) is not a sequence of token ids")
        phrase = tuple(phrase)
        if not phrase:
            raise ValueError(f"{what}: phrase {w} is empty")
        if len(phrase) > hip.MAX_BAD_LEN:
            raise ValueError(f"{what}: phrase {w} has {len(phrase)} tokens, more than {hip.MAX_BAD_LEN} (DH_BEAM_MAX_BAD_LEN)")
        for t in phrase:
            if isinstance(t, bool) or not isinstance(t, numbers.Integral):
                raise ValueError(f"{what}: phrase {w} {phrase!r} holds {t!r}, which is not an integer token id")
            if t < 0 or (num_tokens is not None and t >= num_tokens):
                raise ValueError(f"{what}: phrase {w} {phrase!r} holds id {int(t)} outside [0, "
                                 f"{'num_tokens' if num_tokens is None else num_tokens})")
        out.append(tuple(int(t) for t in phrase))
        if len(out) > hip.MAX_BAD_WORDS:
            raise ValueError(f"{what}: phrase {w} is one more than the {hip.MAX_BAD_WORDS} a list may hold (DH_BEAM_MAX_BAD_WORDS)")
    return tuple(out)


def check_constraints(min_len=0, bad_words_ids=None, max_len=None, num_tokens=None):
    """ALL validation of ``min_len`` and ``bad_words_ids``, checked where ``check_repeat`` is, before anything runs.

    ``min_len`` is an ``int`` with ``0 <= min_len < max_len`` (0: off; a ``bool`` is a misplaced flag -> ``ValueError``, a float a
    ``TypeError``).  ``bad_words_ids`` is ``None``, a ``BadWords``, or a sequence of non-empty sequences of token ids: at most
    ``hip.MAX_BAD_WORDS`` phrases of at most ``hip.MAX_BAD_LEN`` ids, every id an integer in ``[0, num_tokens)`` -- otherwise a
    ``ValueError`` that names the phrase.  Duplicates are allowed; ``[]`` is ``None``.  Returns ``(int, None | BadWords | tuple of
    tuples)``."""
    m = min_len
    if isinstance(m, bool):
        raise ValueError("min_len must be an int >= 0, not a bool")
    if not isinstance(m, numbers.Integral):
        raise TypeError(f"min_len must be an int >= 0, not {type(m).__name__}")
    m = int(m)
    if m < 0:
        raise ValueError(f"min_len must be >= 0, got {m}")
    if max_len is not None and m > 0 and m >= int(max_len):
        raise ValueError(f"min_len must be below max_len: min_len={m}, max_len={int(max_len)}")
    if bad_words_ids is None:
        return m, None
    if isinstance(bad_words_ids, BadWords):
        bw = bad_words_ids
        if num_tokens is not None and (bw.num_tokens is None or bw.num_tokens > num_tokens):
            _phrases(bw.ids, num_tokens)                    # compiled for a larger vocabulary: the ids against this one
        return m, (bw if len(bw) else None)
    ids = _phrases(bad_words_ids, num_tokens)
    return m, (ids or None)


_BAD_WORDS_CACHE = {}           # (device, num_tokens, ids) -> BadWords: a list is uploaded once, not once per call
_BAD_WORDS_CACHE_SIZE = 16


def compile_bad_words(ids, num_tokens=None, device="cuda"):
    """``bad_words_ids`` -> ``BadWords`` on ``device`` (``None`` for ``None`` / ``[]``; a ``BadWords`` of that device as it is).
    Validates like ``check_constraints`` and uploads the flat phrases and their offsets once; a small per-device cache keyed by the
    tuple of tuples gives repeated calls with one list the same tensors.  Not inside a hipGraph capture (a host-to-device copy):
    ``generate_batch_graphed`` compiles in front of it."""
    _, ids = check_constraints(0, ids, None, num_tokens)
    if ids is None:
        return None
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(ids, BadWords):
        if str(ids.device) == str(device):
            return ids
        ids = ids.ids
    key = (str(device), num_tokens, ids)
    bw = _BAD_WORDS_CACHE.get(key)
    if bw is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("compile_bad_words inside a hipGraph capture: compile the list before the capture and pass the BadWords")
        offs = [0]
        for w in ids:
            offs.append(offs[-1] + len(w))
        words = torch.tensor([t for w in ids for t in w], dtype=torch.int32).to(device)
        offsets = torch.tensor(offs, dtype=torch.int32).to(device)
        bw = BadWords(ids, num_tokens, device, words, offsets)
        while len(_BAD_WORDS_CACHE) >= _BAD_WORDS_CACHE_SIZE:
            _BAD_WORDS_CACHE.pop(next(iter(_BAD_WORDS_CACHE)))
        _BAD_WORDS_CACHE[key] = bw
    return bw


MAX_SEQUENCE_BIAS = 1e4         # |bias| <= 1e4: 4,096 of them on one column sum to 4.1e7, far inside fp32


class SequenceBias:
    """A phrase-to-bias list compiled for ``dh_beam_bias_logits`` (``compile_sequence_bias``): ``pairs`` -- a tuple of ``(phrase,
    bias)`` pairs, the phrases tuples of ints and the biases floats, in the order given, duplicates kept --, and four tensors on
    ``device``, uploaded once, that hold the list STABLY SORTED BY LAST ID (so the phrases of one column are neighbours, in the order
    given): ``words`` int32 (the phrases flat), ``offsets`` int32 (``n + 1`` entries), ``bias`` fp32 ``[n]`` and ``run_off`` int32
    (``n_runs + 1`` entries: the starts of the runs of phrases that share a last id).  ``order``: the sort as a tuple of list
    indices.  Immutable; hashable and equal by ``pairs`` and device, so it can sit in a graph cache key, and whoever holds it keeps
    the tensors alive."""
    __slots__ = ("pairs", "num_tokens", "device", "order", "words", "offsets", "bias", "run_off")

    def __init__(self, pairs, num_tokens, device, order, words, offsets, bias, run_off):
        for name, val in zip(self.__slots__, (pairs, num_tokens, device, order, words, offsets, bias, run_off)):
            object.__setattr__(self, name, val)

    def __setattr__(self, name, value):
        raise AttributeError("SequenceBias is immutable")

    def __delattr__(self, name):
        raise AttributeError("SequenceBias is immutable")

    @property
    def n_words(self):
        return len(self.pairs)

    @property
    def n_runs(self):
        return self.run_off.numel() - 1

    def __len__(self):
        return len(self.pairs)

    def __hash__(self):
        return hash((self.pairs, str(self.device)))

    def __eq__(self, other):
        return isinstance(other, SequenceBias) and self.pairs == other.pairs and str(self.device) == str(other.device)

    def __repr__(self):
        return f"SequenceBias({len(self.pairs)} phrases, {self.n_runs} columns, device={self.device})"


def check_sequence_bias(sequence_bias=None, num_tokens=None, model=None):
    """ALL validation of ``sequence_bias``, checked where ``check_constraints`` is, before anything runs.

    ``None`` (off, the call without the keyword), a ``SequenceBias``, a mapping ``{tuple of token ids: bias}`` or a sequence of
    ``(phrase, bias)`` pairs -- in a defined order: the dict's insertion order, the list's own.  The phrases obey ``bad_words_ids``'
    limits (at most ``hip.MAX_BAD_WORDS`` phrases of at most ``hip.MAX_BAD_LEN`` ids, every id an integer in ``[0, num_tokens)``);
    every bias is a finite real number with ``abs(bias) <= MAX_SEQUENCE_BIAS`` -- a ``bool``, NaN or an infinity is a ``ValueError``
    that names the phrase (a ban is ``bad_words_ids``' business).  Duplicated phrases are allowed and each one counts; an empty
    mapping is ``None``.  With ``model`` (a captioning model or its decoder) and a list that is not empty, ``pad_index == 1`` is
    refused: that decoder re-runs the whole sequence per token on the module path -- ``NotImplementedError``, as ``return_logprobs``
    there.  Returns ``None | SequenceBias | tuple of (tuple of ints, float) pairs``."""
    sb = _checked_sequence_bias(sequence_bias, num_tokens)
    if sb is not None and model is not None and getattr(getattr(model, "decoder", model), "pad_index", 0) == 1:
        raise NotImplementedError("sequence_bias with pad_index == 1: that decoder re-runs the whole sequence per token on the module "
                                  "path (_generate_reforward); the biases live in the batched engine's per-position row draw")
    return sb


def _checked_sequence_bias(sb, num_tokens):
    if sb is None:
        return None
    if isinstance(sb, SequenceBias):
        if num_tokens is not None and (sb.num_tokens is None or sb.num_tokens > num_tokens):
            _phrases([w for w, _ in sb.pairs], num_tokens, "sequence_bias")      # compiled for a larger vocabulary: the ids against this one
        return sb if len(sb) else None
    if isinstance(sb, (str, bytes)) or not hasattr(sb, "__iter__"):
        raise TypeError(f"sequence_bias must be None, a mapping {{tuple of token ids: bias}} or a sequence of (phrase, bias) pairs, not "
                        f"{type(sb).__name__} (strings go through experiments.sequence_bias_from_words)")
    items = list(sb.items()) if hasattr(sb, "items") else list(sb)
    for w, item in enumerate(items):
        if isinstance(item, (str, bytes)) or not hasattr(item, "__len__") or len(item) != 2:
            raise ValueError(f"sequence_bias: entry {w} ({item!r}) is not a (phrase, bias) pair")
    phrases = _phrases([item[0] for item in items], num_tokens, "sequence_bias")
    out = []
    for w, (phrase, (_, b)) in enumerate(zip(phrases, items)):
        if hasattr(b, "item") and getattr(b, "ndim", 1) == 0:              # (a 0-d tensor or a numpy scalar: its Python number)
            b = b.item()
        if isinstance(b, bool) or not isinstance(b, numbers.Real) or not math.isfinite(b) or abs(b) > MAX_SEQUENCE_BIAS:
            raise ValueError(f"sequence_bias: phrase {w} {phrase!r} has bias {b!r}: a bias is a finite real number with abs(bias) <= "
                             f"{MAX_SEQUENCE_BIAS:g} (to forbid a phrase outright, list it in bad_words_ids)")
        out.append((phrase, float(b)))
    return tuple(out) or None


def sort_sequence_bias(pairs):
    """The host side of ``dh_beam_bias_logits``' layout: ``(order, run_off)`` -- the indices of ``pairs`` stably sorted by the
    phrases' last ids, and the starts of the runs of equal last ids in that order, with the list's length as the last entry."""
    order = sorted(range(len(pairs)), key=lambda i: pairs[i][0][-1])            # (sorted is stable)
    run_off = [i for i in range(len(order)) if i == 0 or pairs[order[i]][0][-1] != pairs[order[i - 1]][0][-1]]
    return tuple(order), run_off + [len(order)]


_SEQ_BIAS_CACHE = {}            # (device, num_tokens, pairs) -> SequenceBias: a list is uploaded once, not once per call
_SEQ_BIAS_CACHE_SIZE = 16


def compile_sequence_bias(sequence_bias, num_tokens=None, device="cuda"):
    """``sequence_bias`` -> ``SequenceBias`` on ``device`` (``None`` for ``None`` / an empty mapping; a ``SequenceBias`` of that
    device as it is).  Validates like ``check_sequence_bias``, sorts the list (``sort_sequence_bias``) and uploads it once; a small
    per-device cache keyed by the pairs gives repeated calls with one list the same tensors.  Not inside a hipGraph capture (a
    host-to-device copy): ``generate_batch_graphed`` compiles in front of it."""
    pairs = check_sequence_bias(sequence_bias, num_tokens)
    if pairs is None:
        return None
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(pairs, SequenceBias):
        if str(pairs.device) == str(device):
            return pairs
        pairs = pairs.pairs
    key = (str(device), num_tokens, pairs)
    sb = _SEQ_BIAS_CACHE.get(key)
    if sb is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("compile_sequence_bias inside a hipGraph capture: compile the list before the capture and pass the "
                               "SequenceBias")
        order, run_off = sort_sequence_bias(pairs)
        offs = [0]
        for i in order:
            offs.append(offs[-1] + len(pairs[i][0]))
        words = torch.tensor([t for i in order for t in pairs[i][0]], dtype=torch.int32).to(device)
        offsets = torch.tensor(offs, dtype=torch.int32).to(device)
        bias = torch.tensor([pairs[i][1] for i in order], dtype=torch.float64).to(torch.float32).to(device)
        sb = SequenceBias(pairs, num_tokens, device, order, words, offsets, bias, torch.tensor(run_off, dtype=torch.int32).to(device))
        while len(_SEQ_BIAS_CACHE) >= _SEQ_BIAS_CACHE_SIZE:
            _SEQ_BIAS_CACHE.pop(next(iter(_SEQ_BIAS_CACHE)))
        _SEQ_BIAS_CACHE[key] = sb
    return sb


@dataclasses.dataclass(frozen=True, eq=False)
class DecodeSettings:
    """The validated decode settings of one call, one field each, as the ``check_*`` functions return them (``bad_words_ids``:
    ``None``, a tuple of tuples or a ``BadWords``; ``sequence_bias``: ``None``, a tuple of pairs or a ``SequenceBias``), and
    ``num_tokens``, the vocabulary the lists were checked against.  The defaults are the settings switched off.  Built by
    ``from_kw`` / ``from_call``.  Immutable; equal and hashed by the settings, a list by its ids or pairs whether compiled or not."""
    return_beams: bool = False
    return_attention: bool = False
    top_p: float = 1.0
    no_repeat_ngram_size: int = 0
    repetition_penalty: float = 1.0
    min_len: int = 0
    bad_words_ids: object = None
    num_tokens: object = dataclasses.field(default=None, compare=False)
    search: str = "sample"
    return_logprobs: bool = False
    length_penalty: float = 0.0
    early_stopping: object = None
    num_beam_groups: int = 1
    diversity_penalty: float = 0.0
    sequence_bias: object = None

    @classmethod
    def names(cls):
        """The keywords that are decode settings: every field but ``num_tokens``."""
        return tuple(f.name for f in dataclasses.fields(cls) if f.compare)

    @classmethod
    def from_kw(cls, kw, max_len, num_tokens=None, model=None):
        """Reads the settings out of the keyword dictionary ``kw`` (which keeps them; ``beam_size`` is read for the groups) and checks
        them in the order below, so a call with two bad values raises for the earlier one; ``model``: see ``check_return_attention``
        / ``check_return_logprobs``."""
        return_beams = check_return_beams(kw.get("return_beams", False))
        return_attention = check_return_attention(kw.get("return_attention", False), model)
        top_p = check_top_p(kw.get("top_p", 1.0))
        ngram, penalty = check_repeat(kw.get("no_repeat_ngram_size", 0), kw.get("repetition_penalty", 1.0), max_len)
        min_len, bad_words = check_constraints(kw.get("min_len", 0), kw.get("bad_words_ids"), max_len, num_tokens)
        search = check_search(kw.get("search", "sample"), top_p)
        return_logprobs = check_return_logprobs(kw.get("return_logprobs", False), model)
        length_penalty = check_length_penalty(kw.get("length_penalty", 0.0), max_len, search)
        early_stopping = check_early_stopping(kw.get("early_stopping"), search, return_attention, return_logprobs)
        groups, diversity = check_beam_groups(kw.get("num_beam_groups", 1), kw.get("diversity_penalty", 0.0), search, kw.get("beam_size"),
                                              early_stopping)
        bias = check_sequence_bias(kw.get("sequence_bias"), num_tokens, model)
        return cls(return_beams, return_attention, top_p, ngram, penalty, min_len, bad_words, num_tokens, str(search), return_logprobs,
                   length_penalty, early_stopping, groups, diversity, bias)

    @classmethod
    def from_call(cls, kw, beam_size, max_len, decoder):
        """``from_kw`` for a decoder's ``generate_batch(..., **kw)``: ``kw`` holds settings only -- any other name is the ``TypeError`` of
        an unexpected keyword argument, and so is ``return_attention`` for a decoder kind without attention maps (no ``_cross``)."""
        for name in kw:
            if name not in cls.names() or (name == "return_attention" and not hasattr(decoder, "_cross")):
                raise TypeError(f"generate_batch() got an unexpected keyword argument {name!r}")
        return cls.from_kw(dict(kw, beam_size=beam_size), max_len, decoder.num_tokens, decoder)

    def call_kw(self, kw):
        """``kw`` as the call that means the same spells it with the fewest keywords: every setting read by ``from_kw`` that is off --
        ``return_attention`` / ``return_logprobs`` ``False``, ``length_penalty`` 0.0, ``early_stopping`` ``None``, one beam group,
        ``sequence_bias`` ``None`` or empty, ``search`` ``"sample"`` -- is removed, and ``length_penalty``, ``early_stopping`` and the
        group pair are the checked values.  One call, one spelling: one graph-cache key.  Returns ``kw``."""
        for name in ("return_attention", "return_logprobs", "length_penalty", "early_stopping", "sequence_bias"):
            if getattr(self, name) == getattr(type(self), name):
                kw.pop(name, None)
            elif name in ("length_penalty", "early_stopping"):
                kw[name] = getattr(self, name)
        if self.search == "sample":
            kw.pop("search", None)
        kw.pop("num_beam_groups", None)
        kw.pop("diversity_penalty", None)
        if self.num_beam_groups > 1:
            kw["num_beam_groups"], kw["diversity_penalty"] = self.num_beam_groups, self.diversity_penalty
        return kw

    def _key(self):
        vals = (getattr(self, name) for name in self.names())
        return tuple(v.ids if isinstance(v, BadWords) else v.pairs if isinstance(v, SequenceBias) else v for v in vals)

    def __eq__(self, other):
        return isinstance(other, DecodeSettings) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def compiled(self, device):
        """The record with its two lists uploaded to ``device`` (``compile_bad_words`` / ``compile_sequence_bias``: once per list, not
        inside a capture).  The ``length_penalty`` table is per session length: ``compile_length_weights``."""
        return dataclasses.replace(self, bad_words_ids=compile_bad_words(self.bad_words_ids, self.num_tokens, device),
                                   sequence_bias=compile_sequence_bias(self.sequence_bias, self.num_tokens, device))

    def new_helper(self, **engine_args):
        """The ``BeamSearchHelper`` of one session with every setting applied; ``engine_args``: the constructor's other arguments."""
        return BeamSearchHelper(top_p=self.top_p, no_repeat_ngram_size=self.no_repeat_ngram_size, repetition_penalty=self.repetition_penalty,
                                **engine_args).set_constraints(self.min_len, self.bad_words_ids).set_search(self.search).set_logprobs(
                                    self.return_logprobs).set_length_penalty(self.length_penalty).set_early_stopping(self.early_stopping).set_beam_groups(
                                        self.num_beam_groups, self.diversity_penalty).set_sequence_bias(self.sequence_bias)


class BeamOverflow(RuntimeError):
    """A row had more logits at its top-k threshold than the pre-filtered samplers' candidate buffers hold (flat / constant logits):
    the decoders catch this and repeat the batch with ``exact=True`` (the general sampler, which draws such rows over the whole row).
    With ``top_p < 1`` the general sampler has no such draw (the nucleus is taken among at most 1,024 survivors): the repeated batch
    raises this again, with a message that says so."""


class _TorchCpuStream:
    """Replica of the stream a seeded ``torch.Generator`` (CPU) feeds ``Tensor.exponential_`` with, generated with numpy so that a
    batch's images can be filled on a thread pool (torch fills serially under the GIL, ~27 ns per value: 256 images x 5 rows x
    36,541 values take 1.2 s per decode step).  What the pinned torch (2.x CPU, ``exponential_kernel_default``) does per element:
    two mt19937 draws -> ``random64`` (first draw = high word) -> ``u = (x & (2^53 - 1)) * 2^-53`` -> ``-log1p(-u)`` in double ->
    cast to the tensor's type (ATen/core/TransformationHelper.h:144, DistributionTemplates.h); ``manual_seed(s)`` is mt19937's
    standard ``init_genrand(s & 0xffffffff)``.  numpy's ``log1p`` is not glibc's (1 ulp of a double apart on ~7 % of the inputs),
    which would change the float32 result when the double lies within a few ulps of a float32 rounding boundary (~2^-26 of the
    samples): exactly those samples are recomputed with ``math.log1p`` (the C library's).  ``self_check`` compares a long fill
    against torch itself; ``TorchRngNoise`` falls back to torch's own fill if it ever fails (another torch build)."""

    _ok = None

    def __init__(self, seed):
        import numpy as np
        key = np.empty(624, dtype=np.uint64)
        s = int(seed) & 0xFFFFFFFF
        key[0] = s
        for j in range(1, 624):
            s = (1812433253 * (s ^ (s >> 30)) + j) & 0xFFFFFFFF
            key[j] = s
        self.bg = np.random.MT19937()
        self.bg.state = {"bit_generator": "MT19937", "state": {"key": key.astype(np.uint32), "pos": 624}}

    def exponential(self, n):
        """The next ``n`` values of ``torch.empty(n).exponential_(1, generator=g)`` as a float32 numpy array."""
        import math
        import numpy as np
        raw = self.bg.random_raw(2 * n)
        x = ((raw[0::2] << np.uint64(32)) | raw[1::2]) & np.uint64((1 << 53) - 1)
        u = x.astype(np.float64) * (2.0 ** -53)
        y = -np.log1p(-u)
        out = y.astype(np.float32)
        frac = (y.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64)      # the 29 bits float32 rounds away
        for i in np.nonzero(np.abs(frac - 0x10000000) <= 16)[0].tolist():
            out[i] = np.float32(-math.log1p(-float(u[i])))
        return out

    @classmethod
    def self_check(cls):
        if cls._ok is None:
            g = torch.Generator().manual_seed(20240229)
            mine = cls(20240229)
            cls._ok = all(bool((torch.empty(n).exponential_(1, generator=g).numpy() == mine.exponential(n)).all())
                          for n in (7, 200000, 36541))
        return cls._ok


class TorchRngNoise:
    """``rng="torch"``: the Exp(1) noise of every draw taken from torch CPU generators in the reference's order and shapes, so that
    the sampled caption is the one the reference returns under the same generator state.  ``torch.multinomial(p, k)`` on the CPU
    is ``topk(p / empty_like(p).exponential_(1), k)``: the reference consumes, per decode step, one ``[n_rows, V]`` fill for the
    row draw (beam.py:39-48 via :57-58; one row at the first step), one ``[n_candidates]`` fill for the candidate draw
    (rnn_models.py:116-121, transformers.py:557-562; ``n_candidates = sum(1 if ended else beam)``, beam.py:72-101) and one
    ``[beam]`` fill for the final draw (rnn_models.py:140, transformers.py:576); nothing once every beam has ended (the ``break`` at
    rnn_models.py:131 / transformers.py:585).

    ``seed=None`` (one image only): the draws come from torch's DEFAULT generator -- ``torch.manual_seed(s); model.generate(image,
    rng="torch")`` is then the reference's own call sequence.  ``seed=int``: image ``i`` of the batch (global index ``img0 + i``)
    draws from its own ``torch.Generator().manual_seed(seed + img0 + i)`` -- row ``i`` equals the reference's
    ``torch.manual_seed(seed + img0 + i); model.generate(image_i)``, whatever the batch composition or rank layout.

    A parity feature, not a throughput path: the noise is generated on the host (rows x V floats per step) and the ended flags are
    read back once per step."""

    def __init__(self, seed, n_img, img0=0, state0=None):
        """``state0``: for ``seed=None``, the default generator's state at the start of the ``generate`` call (``torch.get_rng_state()``
        taken ONCE by the caller): a repeated session (``BeamOverflow`` retry builds a new noise source) then replays the same
        draws instead of continuing from wherever the first attempt left the generator."""
        if seed is None and n_img != 1:
            raise ValueError('rng="torch" with seed=None draws from torch\'s default generator, which only one image at a time can '
                             'consume in the reference\'s order: pass seed=<int> (image i then draws from manual_seed(seed + i))')
        self.seed, self.n_img, self.img0 = seed, int(n_img), int(img0)
        self.gens, self.h, self._state0 = None, None, state0

    def attach(self, helper):
        """Called by the helper that will consume the noise; (re-)positions the generators at the start of their streams, so a
        repeated session (``BeamOverflow`` retry) replays the same draws."""
        self.h = helper
        if self.seed is None:
            if self._state0 is None:
                self._state0 = torch.get_rng_state()
            else:
                torch.set_rng_state(self._state0)
        elif self.n_img >= 8 and _TorchCpuStream.self_check():
            self.gens = [_TorchCpuStream(int(self.seed) + self.img0 + i) for i in range(self.n_img)]     # thread-parallel fills
        else:
            self.gens = [torch.Generator().manual_seed(int(self.seed) + self.img0 + i) for i in range(self.n_img)]

    def _exp(self, i, n):
        g = None if self.gens is None else self.gens[i]
        if isinstance(g, _TorchCpuStream):
            return torch.from_numpy(g.exponential(n))
        return torch.empty(n).exponential_(1, generator=g)

    def _each_image(self, fn, todo):
        """``fn(i)`` for every image of ``todo``: the images' generators are independent, so a batch fills its [rows, V] noise on a
        thread pool (``exponential_`` releases the GIL; one generator is only ever touched by one task at a time)."""
        if self.gens is None or len(todo) < 8:
            for i in todo:
                fn(i)
            return
        pool = self.__dict__.get("_pool")
        if pool is None:
            from concurrent.futures import ThreadPoolExecutor
            pool = self._pool = ThreadPoolExecutor(max_workers=max(1, min(32, (os.cpu_count() or 8) - 1)))
        list(pool.map(fn, todo))

    def __call__(self, kind, step, shape):
        h, b = self.h, self.h.beam_size
        if kind == "multinomial":             # the method surface (sample_k_indices): one fill of the argument's shape
            return self._exp(0, int(torch.Size(shape).numel())).view(shape)
        done = h.done.cpu().tolist()
        out = torch.ones(shape)
        if kind == "row":
            rpi, v = shape[0] // self.n_img, shape[1]

            def fill(i):
                out[i * rpi:(i + 1) * rpi] = self._exp(i, rpi * v).view(rpi, v)
            self._each_image(fill, [i for i in range(self.n_img) if not done[i]])
        elif kind == "cand":
            ended = h._ended.cpu().view(self.n_img, b).tolist()
            for i in range(self.n_img):
                if not done[i]:
                    n_cand = sum(1 if e else b for e in ended[i])
                    out[i, :n_cand] = self._exp(i, n_cand)
        else:                                 # "final": one fill over the beams
            for i in range(self.n_img):
                out[i] = self._exp(i, shape[1])
        return out


class BeamSearchHelper:
    """Beam state for ``n_img`` images x ``beam_size`` beams.

    Reference signature kept: ``BeamSearchHelper(temperature, beam_size, top_k, unk_index,
    eos_index, device)`` (beam.py:7-8); ``n_img``, ``max_len`` and the rest are new keyword arguments.

    ``top_p < 1`` (nucleus filtering, not in the reference): every row draw of ``step`` / ``step_prompted`` runs over the row's
    nucleus of the top-k survivors -- with ``p = softmax(survivors / temperature)`` ordered by ``p`` descending (equal ``p``: lower
    token index first), the survivor at sorted position ``j`` stays iff the exclusive prefix ``p[0] + ... + p[j-1]`` is ``< top_p``
    or ``j < beam_size`` -- through ``dh_beam_row_sample_nucleus``; the candidate draw and the final draw are untouched.  The
    default ``top_p=1.0`` makes today's calls.

    ``no_repeat_ngram_size = n > 0`` / ``repetition_penalty != 1`` (not in the reference either): in front of every row draw of
    ``step`` / ``step_prompted`` one launch of ``dh_beam_history_logits`` edits the logits IN PLACE from every row's own history (the
    token table's columns ``< write_pos``): each distinct token of the history is damped CTRL-style (``x < 0 ? x * penalty :
    x / penalty``), then every token that would complete an n-gram the row already holds becomes ``-inf``; the 64-column group
    maxima are repaired when -- and only when -- the sampler that follows reads them.  A caller's ``logits_hook`` runs before
    ``step`` and therefore sees the model's raw logits.  Deterministic, so it composes with ``rng="torch"``, ``noise_source``,
    ``exact``, streams and hipGraph capture (the position is a launch constant).  The defaults ``0`` / ``1.0`` make no launch.

    ``min_len`` / ``bad_words_ids`` (not in the reference either): behind that launch and in front of the row draw, one launch of
    ``dh_beam_constrain_logits`` -- while ``write_pos < min_len`` the ``<eos>`` column is ``-inf``; for every phrase of the list whose
    ids but the last end the row's history, the last id's column is ``-inf`` (a single id: at every position).  The group maxima
    are repaired on the same condition as above.  A launch is made only when the list is not empty or ``write_pos < min_len``; the
    defaults ``0`` / ``None`` make none.  Both are set with ``helper.set_constraints(min_len=, bad_words_ids=)`` after construction
    (``bad_words_ids``: the raw nesting, compiled there by ``compile_bad_words``, or a ``BadWords``).

    ``sequence_bias`` (not in the reference either; Hugging Face's name): between those two launches, one launch of
    ``dh_beam_bias_logits`` -- for every ``(phrase, bias)`` pair of the list whose first ``l - 1`` ids end the row's own history
    (a single id: at every position), ``bias`` is added to the logit of the phrase's last id; several pairs on one column are added
    one after the other in list order, each addition its own fp32 add; ``-inf`` stays ``-inf``, so a banned token stays banned.
    Behind the history edits because the penalty scales the model's logit; the maxima are repaired on the same condition as
    above.  Under ``search="beam"`` the scores, and with ``logprobs`` the log-probabilities, are taken on the biased rows.  A launch
    is made only with a list; ``None``, the default, makes none.  Set with ``helper.set_sequence_bias(mapping or pairs or
    SequenceBias)`` after construction.

    ``search="beam"`` (not in the reference either; ``helper.set_search("beam")`` after construction): nothing is drawn.  Behind the
    history edits and the bans every live row keeps the ``beam_size`` columns with the largest logit (never ``unk_index``; equal
    logits to the lower index), each with its log-probability ``x / temperature - logsumexp(x / temperature)`` over the whole row
    (``dh_beam_row_best``); per image the ``beam_size`` candidates with the largest cumulative score stay, equal scores to the lower
    candidate index (``dh_beam_select_best``: ``hparent`` is the real parent row there, and the first step sets ``ended`` from
    ``<eos>`` for every decoder kind); ``finalize`` returns the beam with the largest score.  ``top_k`` keeps its assertion and has no
    other effect; ``seed``, ``noise_source`` and ``exact`` have none: no noise is generated or consumed, two calls return the same
    bits, and there is no overflow case.  ``vals`` -- ``BeamCaptions.scores`` -- are cumulative model log-probabilities of the tokens
    the rows hold: a step that writes no token column (``write_pos`` past the table: the Transformer decoders' last) is skipped.  All launch
    constants, so it captures into a hipGraph like the rest.

    ``length_penalty`` (with ``search="beam"`` only; ``helper.set_length_penalty(value)`` after construction, behind ``set_search``):
    the select ranks by the length-normalised ``key = fp32(score * w[L])`` in place of the score, inside the pruning.  ``L`` is the
    number of columns the search itself has written to a beam, from the image's first generated column (the dense first step's
    ``write_pos``; ``first_pos[i]`` in a prompted session) through its own first ``<eos>``; ``w[L] = float32(float64(L) **
    -length_penalty)``, ``w[0] = 1``, is computed on the host and uploaded once as ``len_w`` fp32 ``[max_len + 1]`` (no power runs on
    the device).  Scores are ``<= 0``: a value ``> 0`` favours longer captions, ``< 0`` shorter ones.  A live beam's ``beam_size``
    candidates take ``w[write_pos + 1 - first column]``; an ended beam's candidate carries the key it was kept with, never recomputed.
    The candidates with the largest key stay, equal keys to the lower candidate index, ``-inf`` last (``dh_beam_select_best_norm`` in
    place of ``dh_beam_select_best``); the kept keys go to ``keys`` fp32 ``[rows]``, ``vals`` stays the raw cumulative log-probability,
    and ``finalize`` orders by ``keys``: ``BeamCaptions.scores`` are the keys.  With ``return_logprobs`` the left-to-right fp32 sum of a
    live beam's own columns, times ``w[L]``, is its score bit for bit.  ``0.0``, the default: no table, no ``keys``, today's launches
    and bits.

    ``early_stopping`` (with ``search="beam"`` only; ``helper.set_early_stopping(True | False)`` after construction, the last of the
    chain): the finished-hypothesis pool of the usual beam search.  Per image ``beam_size`` entries -- ``pool_tokens`` int32 ``[n_img,
    beam, max_len]``, ``pool_keys`` / ``pool_vals`` fp32 and ``pool_len`` int32 ``[n_img, beam]``, ``pool_n`` int32 ``[n_img]`` --,
    physically sorted: slot 0 the largest key, equal keys in order of arrival.  The select (``dh_beam_select_pool`` in place of
    ``dh_beam_select_best`` / ``_norm``; keys as under ``length_penalty``, from a table of ones without one) ranks the candidates as
    before; down the ranking a candidate whose token is ``<eos>`` never takes a slot -- with rank ``< beam_size`` and key ``> -inf`` it
    is offered to the pool: the parent's row with ``<eos>`` at ``write_pos``, inserted behind every entry whose key is ``>=`` its own,
    entry ``beam_size`` falling off --, the ``beam_size`` best others stay as live beams (``ended = 0``) and a slot nothing is left for
    is dead: ``ended = 1``, ``vals = keys = -inf``.  So the beam keeps its width and a finished caption is never pushed out by a live
    prefix.  ``done`` is set when the pool is full and the mode is ``True``, or no live beam kept at this step has a key above the
    pool's worst (``False``).  ``finalize`` makes ONE launch of ``dh_beam_finalize_pool`` -- never the ``beams`` launch --: the pool
    and, for an image that is not done, its live slots offered the same way; ``lengths`` are each hypothesis' own (``<eos>``
    included: the ``len_bias_done`` convention, which cuts a finished Transformer image's last ``<eos>``, is not applied),
    ``scores`` the keys, ``beam_index`` the live slot or -1 for an entry of the pool.  Refused with ``return_attention`` /
    ``return_logprobs``: both gathers walk tables from a live engine row.  ``None``, the default: no pool, today's launches and bits.

    ``num_beam_groups`` / ``diversity_penalty`` (with ``search="beam"`` only; ``helper.set_beam_groups(G, lam)`` after construction,
    behind ``set_early_stopping``): diverse beam search (Vijayakumar et al. 2016).  Engine slots ``g * Bg .. g * Bg + Bg - 1``, ``Bg =
    beam_size // G``, are group ``g`` from the first step to the last; a beam never changes group.  The select
    (``dh_beam_select_groups`` in place of ``dh_beam_select_best`` / ``_norm``; candidates and keys as under ``length_penalty``, from a
    table of ones without one) ranks the groups one after the other: group ``g`` among the candidates of its own rows (an image's
    first step, with one row: all ``beam_size`` picks) by ``fp32(key - fp32(lam * count))``, ``count`` the times the candidate's token
    was kept at this position by groups ``0 .. g - 1``; an ended beam's candidate and one at ``-inf`` are neither penalised nor
    counted; equal values to the lower candidate index.  The penalty shapes each step's choice and is never stored: ``vals`` and
    ``keys`` hold what they hold without groups, ``BeamCaptions.scores`` stay model log-probabilities (times ``w[L]`` under a
    ``length_penalty``), and ``finalize`` is unchanged -- all beams in score order, ``beam_index // Bg`` a beam's group.  Refused with
    ``early_stopping``.  ``1``, the default: today's launches and bits.

    ``return_logprobs`` (not in the reference either; ``helper.set_logprobs(True)`` after construction): the model log-probability of
    every token the search writes, with nothing shuffled per step.  In front of whichever select a step runs, one launch of
    ``dh_beam_pick_logprobs`` sweeps every logits row once more -- behind the history edits and the bans, in front of the samplers' own
    top-k / nucleus / ``<unk>`` filtering -- and leaves ``pick_lp[r, j] = x[r, pick_idx[r, j]] / temperature - logsumexp(x[r] /
    temperature)`` for the row's picks, zeros for a row that has ended (under ``search="beam"`` no sweep: the bits of ``pick_val``
    under the same mask); behind the select one launch of ``dh_beam_record_logprobs`` writes slab ``step_index`` of two position-major
    tables ``[max_len + 1, rows]`` -- ``par_w``, every row's parent, and ``lp_w``, the ``pick_lp`` of the token the row just received.
    An image that takes no step (forced by its prompt, or done) leaves its slab as ``set_logprobs`` filled it: identity / 0.
    ``finalize`` then takes the ``beams`` launch and one launch of ``dh_beam_gather_logprobs`` walks every kept beam's back-pointers
    once.  Off, the default: no table, no launch.  All launch constants, so it captures into a hipGraph like the rest.
    """

    def __init__(self, temperature=1.0, beam_size=10, top_k=50, unk_index=1, eos_index=3, device='cuda',
                 n_img=1, max_len=25, src_len=0, seed=0, img0=0, noise_source=None, seed_tensor=None, exact=False, top_p=1.0,
                 no_repeat_ngram_size=0, repetition_penalty=1.0):
        assert beam_size <= top_k, '`beam_size` should be less than `top_k`'          # beam.py:9
        self.top_p = check_top_p(top_p)
        self.no_repeat_ngram_size, self.repetition_penalty = check_repeat(no_repeat_ngram_size, repetition_penalty, max_len)
        self._history_edits = self.no_repeat_ngram_size > 0 or self.repetition_penalty != 1.0
        self.min_len, self.bad_words, self._constraints = 0, None, False      # min_len / bad_words_ids: set_constraints
        self.search = "sample"            # "beam": set_search
        self.logprobs, self.pick_lp, self.lp_w, self.par_w = False, None, None, None      # return_logprobs: set_logprobs
        self.length_penalty, self.len_w, self.keys, self.first_col = 0.0, None, None, 0   # length_penalty: set_length_penalty
        self.early_stopping = None        # True / False: the finished-hypothesis pool (set_early_stopping)
        self.pool_tokens = self.pool_keys = self.pool_vals = self.pool_len = self.pool_n = None
        self.num_beam_groups, self.diversity_penalty = 1, 0.0      # diverse groups of beams: set_beam_groups
        self.sequence_bias = None         # a compiled SequenceBias: set_sequence_bias
        self.exact = bool(exact)         # row draws through the general sampler only (see BeamOverflow)
        if beam_size > hip.MAX_BEAMS:     # one wave draws among an image's beams (dh_beam_finalize); the reference has no limit
            raise ValueError(f"beam_size <= {hip.MAX_BEAMS} supported")
        self.temperature, self.beam_size, self.top_k = float(temperature), int(beam_size), int(top_k)
        self.unk_index, self.eos_index, self.device = unk_index, eos_index, device
        self.n_img, self.max_len = n_img, max_len
        self.seed, self.img0, self.noise_source = int(seed), int(img0), noise_source
        if hasattr(noise_source, "attach"):
            noise_source.attach(self)
        # optional device-resident int64 word XOR-ed into the seed by the kernels: lets a captured hipGraph of the
        # whole decode be replayed with a fresh seed (kernel arguments are frozen at capture)
        self.seed_tensor = seed_tensor
        self.first_pos = None             # int32 [n_img] prompt lengths of a prompted session (set_prompts); None: dense
        r = n_img * beam_size
        dev = device
        # all zero-initialised state carved out of ONE zeroed arena (one fill launch instead of eight per generate call)
        words = [r * max_len, r, (r + 3) // 4, r, r, (n_img + 3) // 4, n_img, 1]
        offs = [0]
        for w in words:
            offs.append(offs[-1] + (w + 3) // 4 * 4)                                   # 16-byte aligned pieces
        arena = torch.zeros((offs[-1],), dtype=torch.int32, device=dev)
        piece = lambda i: arena[offs[i]:offs[i] + words[i]]
        self.tokens = piece(0).view(r, max_len)
        self.vals = piece(1).view(torch.float32)
        # engine state (uint8, all images).  `has_ended` starts as the SAME tensor; the reference-style method surface below
        # (process_logits, or a caller assigning `helper.has_ended = ...` as rnn_models.py:103,126 do) rebinds only the public name
        self._ended = piece(2).view(torch.uint8)[:r]
        self.has_ended = self._ended
        self._draws = 0                   # multinomial calls made through the method surface (Philox `draw` counter)
        self.parent, self.hparent = piece(3), piece(4)
        self.done = piece(5).view(torch.uint8)[:n_img]
        self.end_step, self.err = piece(6), piece(7)
        self.pick_idx = torch.empty((r, beam_size), dtype=torch.int32, device=dev)
        self.pick_val = torch.empty((r, beam_size), dtype=torch.float32, device=dev)
        # KV-cache ancestor table (Transformer only): src[r, j] = row holding position j of r's history
        self.src = None
        if src_len:
            base = (torch.arange(r, dtype=torch.int32, device=dev) // beam_size) * beam_size
            self.src = base[:, None].expand(r, src_len).contiguous()

    def set_constraints(self, min_len=0, bad_words_ids=None):
        """``min_len`` / ``bad_words_ids`` of this session (see the class docstring), validated by ``check_constraints`` against the
        helper's ``max_len``; the raw nesting is compiled here (``compile_bad_words``: one upload, so not inside a hipGraph capture),
        a ``BadWords`` is taken as it is.  A method, not two more constructor arguments: the constructor's parameter list ends at
        ``repetition_penalty``.  Returns the helper."""
        self.min_len, bad_words_ids = check_constraints(min_len, bad_words_ids, self.max_len)
        self.bad_words = compile_bad_words(bad_words_ids, None, self.device)
        self._constraints = self.min_len > 0 or self.bad_words is not None
        return self

    def set_search(self, search):
        """``search`` of this session (see the class docstring), validated by ``check_search`` against the helper's ``top_p``.  A method
        like ``set_constraints``: the constructor's parameter list stays as it is.  Returns the helper."""
        self.search = check_search(search, self.top_p)
        return self

    def set_logprobs(self, on=True):
        """``return_logprobs`` of this session (see the class docstring).  On: the picks' log-probabilities ``pick_lp [rows, beam]`` and
        the two position-major tables ``lp_w`` fp32 / ``par_w`` int32 ``[max_len + 1, rows]`` -- one zeroed arena of their own, then
        every row's own index into ``par_w`` -- once per session.  Off, the default: nothing is allocated and no launch is made.  A
        method like ``set_search``: the constructor's parameter list stays as it is.  Returns the helper."""
        self.logprobs = check_return_logprobs(on)
        self.pick_lp = self.lp_w = self.par_w = None
        if self.logprobs:
            r, n_pos = self.n_img * self.beam_size, self.max_len + 1
            arena = torch.zeros((2 * n_pos * r + r * self.beam_size,), dtype=torch.int32, device=self.device)
            self.lp_w = arena[:n_pos * r].view(torch.float32).view(n_pos, r)
            self.par_w = arena[n_pos * r:2 * n_pos * r].view(n_pos, r)
            self.par_w += torch.arange(r, dtype=torch.int32, device=self.device)
            self.pick_lp = arena[2 * n_pos * r:].view(torch.float32).view(r, self.beam_size)
        return self

    def set_length_penalty(self, length_penalty=0.0):
        """``length_penalty`` of this session (see the class docstring), validated by ``check_length_penalty`` against the helper's
        ``max_len`` and ``search`` (so behind ``set_search``).  Non-zero: the weight table ``len_w`` fp32 ``[max_len + 1]`` and the
        zeroed per-row state ``keys`` fp32 ``[rows]`` (``_set_keys``).  Zero, the default: nothing is allocated and no launch changes.
        Returns the helper."""
        self.length_penalty = check_length_penalty(length_penalty, self.max_len, self.search)
        self.len_w = self.keys = None     # (another penalty: another table)
        return self._set_keys()

    def _set_keys(self):
        """``len_w`` / ``keys`` for the three settings whose selects rank by key: with a length penalty, a pool or groups on, the weight
        table of the penalty -- of ones at 0.0: ``x * 1.0f`` is ``x``, so one kernel serves both -- and the zeroed per-row keys, made
        where there are none (``compile_length_weights``: one upload per value and length, so not inside a hipGraph capture unless it
        is cached); with all three off, neither.  Returns the helper."""
        if self.length_penalty == 0.0 and self.early_stopping is None and self.num_beam_groups == 1:
            self.len_w = self.keys = None
        elif self.len_w is None:
            self.len_w = compile_length_weights(self.length_penalty, self.max_len, self.device)
            self.keys = torch.zeros((self.n_img * self.beam_size,), dtype=torch.float32, device=self.device)
        return self

    def set_early_stopping(self, early_stopping=None):
        """``early_stopping`` of this session (see the class docstring), validated by ``check_early_stopping`` against the helper's
        ``search`` and ``logprobs`` (so behind ``set_search``, ``set_logprobs`` and ``set_length_penalty``).  ``True`` / ``False``: the
        per-image pool in ONE zeroed arena -- ``pool_tokens`` int32 ``[n_img, beam, max_len]``, ``pool_keys`` (filled with ``-inf``)
        and ``pool_vals`` fp32 ``[n_img, beam]``, ``pool_len`` int32 ``[n_img, beam]``, ``pool_n`` int32 ``[n_img]`` --, and the keys
        and their weight table (``_set_keys``).  ``None``, the default: nothing is allocated and no launch changes.  Returns the
        helper."""
        self.early_stopping = check_early_stopping(early_stopping, self.search, False, self.logprobs)
        self.pool_tokens = self.pool_keys = self.pool_vals = self.pool_len = self.pool_n = None
        self._set_keys()
        if self.early_stopping is None:
            return self
        n, b, m = self.n_img, self.beam_size, self.max_len
        arena = torch.zeros((n * b * m + 3 * n * b + n,), dtype=torch.int32, device=self.device)
        self.pool_tokens = arena[:n * b * m].view(n, b, m)
        o = n * b * m
        self.pool_keys = arena[o:o + n * b].view(torch.float32).view(n, b)
        self.pool_vals = arena[o + n * b:o + 2 * n * b].view(torch.float32).view(n, b)
        self.pool_len = arena[o + 2 * n * b:o + 3 * n * b].view(n, b)
        self.pool_n = arena[o + 3 * n * b:]
        self.pool_keys.fill_(float("-inf"))
        return self

    def set_beam_groups(self, num_beam_groups=1, diversity_penalty=0.0):
        """``num_beam_groups`` / ``diversity_penalty`` of this session (see the class docstring), validated by ``check_beam_groups``
        against the helper's ``search``, ``beam_size`` and ``early_stopping`` (so behind ``set_early_stopping``).  More than one group:
        the keys and their weight table (``_set_keys``).  One group, the default: nothing is allocated and no launch changes.
        Returns the helper."""
        self.num_beam_groups, self.diversity_penalty = check_beam_groups(num_beam_groups, diversity_penalty, self.search, self.beam_size,
                                                                         self.early_stopping)
        return self._set_keys()

    def set_sequence_bias(self, sequence_bias=None):
        """``sequence_bias`` of this session (see the class docstring), validated by ``check_sequence_bias``; a mapping or a list of
        pairs is compiled here (``compile_sequence_bias``: one upload, so not inside a hipGraph capture), a ``SequenceBias`` is taken
        as it is.  ``None``, the default: no launch is made.  A method like ``set_constraints``: the constructor's parameter list
        stays as it is.  Returns the helper."""
        self.sequence_bias = compile_sequence_bias(sequence_bias, None, self.device)
        return self

    def set_prefix(self, caption):
        """caption int64 [n_img, p]: teacher-forced beginning, copied to every beam row."""
        p = caption.shape[1]
        self.tokens[:, :p] = caption.to(torch.int32).repeat_interleave(self.beam_size, dim=0)

    def set_prompts(self, caption, first_pos, pad_index=0):
        """Prompted batch: ``caption`` int64 ``[n_img, P]`` and ``first_pos`` int32 ``[n_img]`` on the device -- image ``i`` is
        teacher-forced with ``caption[i, :first_pos[i]]``; the rest of its row is the caller's padding and never reaches the token
        table (columns ``>= first_pos[i]`` hold ``pad_index`` until the image's own draws fill them).  Every beam row points at its
        image's base row (``parent`` / ``hparent``, as ``src`` does from the start): the one row with history behind it while the
        image is forced.  From here on the steps go through ``step_prompted``."""
        p = min(caption.shape[1], self.max_len)
        dev = self.device
        cap = caption[:, :p].to(device=dev, dtype=torch.int32)
        used = torch.arange(p, device=dev, dtype=torch.int32)[None, :] < first_pos[:, None]
        cap = torch.where(used, cap, torch.full_like(cap, pad_index))
        self.tokens[:, :p] = cap.repeat_interleave(self.beam_size, dim=0)
        base = (torch.arange(self.n_img * self.beam_size, dtype=torch.int32, device=dev) // self.beam_size) * self.beam_size
        self.parent.copy_(base)
        self.hparent.copy_(base)
        self.first_pos = first_pos

    def step_prompted(self, logits, write_pos, t, step_index, first_sets_ended=False, group_max=None):
        """One beam step of a prompted batch from ``logits [n_img*beam, V]`` at absolute position ``step_index``: per image forced
        (``step_index < first_pos``: nothing happens), first (``==``: ``step(first=True)`` from the image's base row) or normal
        (``>``: ``step(first=False)``) -- ``dh_beam_row_sample*_prompted`` + ``dh_beam_select_prompted``.  Philox noise only."""
        assert self.noise_source is None or self.search == "beam"
        self._draw_and_select(logits, False, write_pos, t, step_index, first_sets_ended, group_max, prompted=True)

    def _noise(self, kind, step, shape, ld=None):
        if self.noise_source is None:
            return None
        t = self.noise_source(kind, step, shape)
        if t is None:
            return None
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if ld is not None and ld != t.shape[1]:          # row noise is indexed with the logits' (padded) row stride
            buf = torch.ones((t.shape[0], ld), dtype=torch.float32, device=self.device)
            buf[:, :t.shape[1]] = t
            t = buf
        return t

    def step(self, logits, first, write_pos, t, step_index, first_sets_ended=False, group_max=None):
        """One beam step from ``logits`` ([n_img, V] if ``first`` else [n_img*beam, V]):
        beam.py:55-108 + the caller-side candidate draw (rnn_models.py:116-128, transformers.py:557-569)."""
        self._draw_and_select(logits, first, write_pos, t, step_index, first_sets_ended, group_max)

    def _draw_and_select(self, logits, first, write_pos, t, step_index, first_sets_ended, group_max, prompted=False):
        """``step`` and ``step_prompted``: the history edits, the biases, the bans, the row draw and the select, in that order."""
        rows, v = logits.shape
        b = self.beam_size
        rpi = 1 if first else b
        assert rows == self.n_img * rpi
        best = self.search == "beam"      # (its row step takes the maxima whenever they are there: it filters nothing by top_k)
        if best and write_pos >= self.tokens.shape[1]:
            # the Transformer decoders' last step writes no token (transformers.py:557) and only re-draws the beams: here it would add
            # the log-probability of a token no caption holds to every live score, so it makes no launch
            return
        mult = b if first else 1          # the token table's row of logits row r: a first step's compact rows sit at img * beam
        first_pos = self.first_pos if prompted else None
        # the general sampler reads the whole row; otherwise k group maxima bound the k-th logit.  Decided ONCE: the history pass and
        # the bans repair the maxima exactly when the sampler below reads them
        gm = group_max if (group_max is not None and (best or (not self.exact and self.top_k <= hip.n_groups(v)))) else None
        if self._history_edits:           # no_repeat_ngram_size / repetition_penalty: the row's own history edits its logits first
            hip.beam_history_logits(logits, v, self.tokens, mult, write_pos, rows, rpi, self.no_repeat_ngram_size,
                                    self.repetition_penalty, group_max=gm, first_pos=first_pos)
        # sequence_bias: behind the history edits (the penalty scales the MODEL's logit) and in front of the bans (they commute:
        # -inf + b = -inf).  A launch only with a list; the maxima are repaired on the same condition
        sb = self.sequence_bias
        if sb is not None:
            hip.beam_bias_logits(logits, v, self.tokens, mult, write_pos, rows, rpi, sb.words, sb.offsets, sb.bias, sb.run_off, len(sb),
                                 sb.n_runs, group_max=gm, first_pos=first_pos)
        # min_len / bad_words_ids: the bans behind the history edits (both store ``-inf`` or map it to itself, so the order does not
        # show).  A launch only when there is something to ban at this position
        bw = self.bad_words
        if bw is not None or write_pos < self.min_len:
            hip.beam_constrain_logits(logits, v, self.tokens, mult, write_pos, rows, rpi, self.eos_index, self.min_len,
                                      None if bw is None else bw.words, None if bw is None else bw.offsets, 0 if bw is None else len(bw),
                                      group_max=gm, first_pos=first_pos)
        if best:                          # search="beam": the most likely tokens and candidates, no noise anywhere
            hip.beam_row_best(logits, v, rows, rpi, b, self.temperature, self.unk_index, step_index, self.pick_idx, self.pick_val, self.err,
                              group_max=gm, first_pos=first_pos)
            if self.logprobs:             # the bits the row step left in pick_val, zero for the rows that have ended
                hip.beam_pick_logprobs(None, v, rows, rpi, b, self.temperature, step_index, self._ended, self.pick_idx, self.pick_val,
                                       self.pick_lp, from_vals=True, first_pos=first_pos)
            if self.early_stopping is not None:
                # the finished-hypothesis pool: the rank on the keys (a table of ones without a penalty), <eos> candidates to the pool
                if first:
                    self.first_col = write_pos
                hip.beam_select_pool(self.pick_idx, self.pick_val, self.tokens, self.vals, self.keys, self._ended, self.src, self.parent,
                                     self.hparent, self.done, self.end_step, self.pool_tokens, self.pool_keys, self.pool_vals, self.pool_len,
                                     self.pool_n, self.n_img, b, first, self.early_stopping, write_pos, t, step_index, self.eos_index,
                                     self.len_w, first_col=self.first_col, first_pos=self.first_pos)
            elif self.num_beam_groups > 1:
                # diverse groups: the rank of every group on its own rows' keys less what the groups before it took at this position
                # (the keys as below; a table of ones without a length penalty)
                if first:
                    self.first_col = write_pos
                hip.beam_select_groups(self.pick_idx, self.pick_val, self.tokens, self.vals, self.keys, self._ended, self.src,
                                       self.parent, self.hparent, self.done, self.end_step, self.n_img, b, first, True, write_pos, t,
                                       step_index, self.eos_index, self.len_w, first_col=self.first_col, first_pos=self.first_pos,
                                       n_groups=self.num_beam_groups, diversity_penalty=self.diversity_penalty)
            elif self.length_penalty != 0.0:
                # the rank on key = score * len_w[L]; L counts from the image's first generated column: the dense first step's
                # write_pos, or a prompted session's first_pos (also behind its longest prompt, where the steps are dense again)
                if first:
                    self.first_col = write_pos
                hip.beam_select_best_norm(self.pick_idx, self.pick_val, self.tokens, self.vals, self.keys, self._ended, self.src,
                                          self.parent, self.hparent, self.done, self.end_step, self.n_img, b, first, True, write_pos, t,
                                          step_index, self.eos_index, self.len_w, first_col=self.first_col, first_pos=self.first_pos)
            else:
                hip.beam_select_best(self.pick_idx, self.pick_val, self.tokens, self.vals, self._ended, self.src, self.parent, self.hparent,
                                     self.done, self.end_step, self.n_img, b, first, True, write_pos, t, step_index, self.eos_index,
                                     first_pos=first_pos)
            if self.logprobs:
                hip.beam_record_logprobs(self.tokens, self.parent, self.done, self.end_step, self.pick_idx, self.pick_lp, self.n_img, b,
                                         first, write_pos, step_index, self.lp_w, self.par_w, first_pos=first_pos)
            return
        noise = self._noise("row", step_index, (rows, v), logits.stride(0))       # (None in a prompted session: Philox only)
        draw = (self.seed, self.img0, step_index, self.pick_idx, self.pick_val, self.err)
        if self.top_p < 1.0:              # the nucleus of the survivors: one entry point for the three routes below
            hip.beam_row_sample_nucleus(logits, v, rows, rpi, b, self.top_k, self.top_p, self.temperature, self.unk_index, noise, *draw,
                                        seed_ptr=self.seed_tensor, exact=self.exact, group_max=gm, first_pos=first_pos)
        elif prompted:
            hip.beam_row_sample_prompted(logits, v, rows, b, self.top_k, self.temperature, self.unk_index, noise, self.seed, self.img0,
                                         step_index, first_pos, self.pick_idx, self.pick_val, self.err, seed_ptr=self.seed_tensor,
                                         exact=self.exact, group_max=gm)
        elif gm is not None:
            # bf16 path: the vocabulary GEMM left per-row maxima of every 64-column group (dh_vocab_logits)
            hip.beam_row_sample_groups(logits, v, gm, rows, rpi, b, self.top_k, self.temperature, self.unk_index, noise, *draw,
                                       seed_ptr=self.seed_tensor)
        else:
            hip.beam_row_sample(logits, v, rows, rpi, b, self.top_k, self.temperature, self.unk_index, noise, *draw,
                                seed_ptr=self.seed_tensor, exact=self.exact)
        if self.logprobs:
            # return_logprobs: one more sweep of the rows (L2-resident by now) for log_softmax(x / T) at the picks -- behind the edits and
            # the bans, in front of the samplers' own filtering -- while `ended` still holds the flags of the rows the picks came from
            hip.beam_pick_logprobs(logits, v, rows, rpi, b, self.temperature, step_index, self._ended, self.pick_idx, self.pick_val,
                                   self.pick_lp, first_pos=first_pos)
        state = (self.pick_idx, self.pick_val, self.tokens, self.vals, self._ended, self.src, self.parent, self.hparent, self.done,
                 self.end_step, self.n_img, b)
        if prompted:
            hip.beam_select_prompted(*state, first_pos, first_sets_ended, write_pos, t, step_index, self.temperature, self.eos_index,
                                     None, self.seed, self.img0, seed_ptr=self.seed_tensor)
        else:
            noise = None if first else self._noise("cand", step_index, (self.n_img, b ** 2))
            hip.beam_select(*state, first, first_sets_ended, write_pos, t, step_index, self.temperature, self.eos_index, noise,
                            self.seed, self.img0, seed_ptr=self.seed_tensor)
        if self.logprobs:                 # slab `step_index`: every row's parent and the log-probability of the token it just got
            hip.beam_record_logprobs(self.tokens, self.parent, self.done, self.end_step, self.pick_idx, self.pick_lp, self.n_img, b, first,
                                     write_pos, step_index, self.lp_w, self.par_w, first_pos=first_pos)

    def finalize(self, len_bias_done, full_len, pad_index=0, defer_check=False, first_beam=False, beams=False, pos=0, attn_w=None):
        """Final draw among the beams and output copy; returns a ``SessionResult`` whose ``captions`` are ``(tokens int64 [n_img,
        max_len], lengths)``.  ``defer_check``: skip the host read of the device error word (hipGraph capture) -- the result carries
        ``self.err`` for the caller to check after replay.  ``first_beam``: no draw, beam 0 -- what the reference's final
        ``sample_k_indices(sample_val, k=1)`` degenerates to when ``sample_val`` is still the ``[beam, 1]`` column of the
        first step (rnn_models.py:93, 140-141: no decode step ran because the prefix already fills ``max_len - 1``).
        ``beams=True``: one launch of ``dh_beam_finalize_beams`` instead -- the same draw, and every beam kept: the ``captions`` are a
        ``BeamCaptions``.  ``pos``: the first generated column of a dense session (the
        prefix length), from where a beam's own ``<eos>`` is looked for; a prompted session's comes from ``self.first_pos``.
        ``attn_w`` (``return_attention``; fp32 ``[n_pos, rows, S]``, slab ``c`` = the maps position ``c`` wrote at its logical rows):
        always the ``beams`` launch, and one launch of ``dh_beam_gather_attention`` behind it leaves every kept beam's maps -- read
        through ``self.src``, for the columns below the beam's own length, zero elsewhere -- in the result's ``attention``, fp32
        ``[n_img, beam, max_len, S]``; its ``captions`` are those of ``beams=True``.
        ``search="beam"``: no draw and no noise -- always the ``beams`` launch, whose slot 0 is the beam with the largest score (equal
        scores: the lower engine index); ``drawn`` is 0 for every image and the plain pair is slot 0's row and ``row_lengths``.
        ``return_logprobs`` (``set_logprobs``): always the ``beams`` launch too, and one launch of ``dh_beam_gather_logprobs`` behind it
        walks every kept beam's back-pointers (``par_w``) once and leaves the log-probabilities of its own columns -- from the image's
        first generated column up to the beam's own length, zero elsewhere -- in the result's ``logprobs``, fp32 ``[n_img, beam,
        max_len]``; its ``captions`` are those of ``beams=True``.
        ``early_stopping`` (``set_early_stopping``): ONE launch of ``dh_beam_finalize_pool`` and never the ``beams`` launch -- the pool's
        entries and, for an image that is not done, its live slots offered through the select's insertion rule; always a
        ``BeamCaptions`` inside (the plain pair is ``(tokens[:, 0], lengths[:, 0])``): ``lengths`` each hypothesis' own with its
        ``<eos>`` included, ``scores`` the keys, ``beam_index`` the live slot or -1 for an entry of the pool, ``drawn`` 0.
        ``len_bias_done`` is NOT applied there: that convention cuts the last ``<eos>`` of a finished Transformer image, and here every
        hypothesis knows its own length."""
        best = self.search == "beam"
        if best:
            noise = None
        elif first_beam:                 # the kernel's race p / noise with an infinite handicap on every beam but the first
            noise = torch.full((self.n_img, self.beam_size), float("inf"), dtype=torch.float32, device=self.device)
            noise[:, 0] = 1.0
        else:
            noise = self._noise("final", 0, (self.n_img, self.beam_size))
        logprobs = None
        n, b, dev = self.n_img, self.beam_size, self.device

        def beam_outputs():               # what a launch that keeps every beam writes: tokens, four int32 pieces of one buffer, scores
            out = torch.empty((n, b, self.max_len), dtype=torch.int32, device=dev)
            ints = torch.empty((2 * n * b + 2 * n,), dtype=torch.int32, device=dev)
            return (out, ints[:n * b].view(n, b), ints[n * b:2 * n * b].view(n, b), ints[2 * n * b:2 * n * b + n], ints[2 * n * b + n:],
                    torch.empty((n, b), dtype=torch.float32, device=dev))
        if self.early_stopping is not None:
            # ``early_stopping``: ONE launch of ``dh_beam_finalize_pool``, never the ``beams`` launch -- the pool's entries and, for an
            # image that is not done, its live slots, the best ``beam_size`` by key.  Every hypothesis knows its own length (``<eos>``
            # included), so ``len_bias_done`` -- the convention that cuts a finished Transformer image's last ``<eos>`` -- is NOT applied.
            if attn_w is not None:
                raise NotImplementedError("early_stopping with return_attention: a hypothesis in the pool has no live engine row to gather from")
            out, o_len, o_idx, o_drawn, o_row, o_score = beam_outputs()
            hip.beam_finalize_pool(self.tokens, self.keys, self._ended, self.done, self.pool_tokens, self.pool_keys, self.pool_len,
                                   self.pool_n, out, o_len, o_score, o_idx, o_drawn, o_row, n, b, full_len, pad_index)
            attention = None
            captions = BeamCaptions(out.long(), o_len.long(), o_score, o_idx.long(), o_drawn.long(), o_row.long())
            if not beams:
                captions = (captions.tokens[:, 0], captions.row_lengths)
        elif beams or attn_w is not None or best or self.logprobs:
            out, o_len, o_idx, o_drawn, o_row, o_score = beam_outputs()
            hip.beam_finalize_beams(self.tokens, self.vals if self.keys is None else self.keys, self.done, self.end_step, out, o_len, o_score, o_idx, o_drawn, o_row, n, b,
                                    len_bias_done, full_len, pad_index, self.eos_index, pos, self.first_pos,
                                    self.temperature, noise, self.seed, self.img0, seed_ptr=self.seed_tensor)
            attention = None
            if attn_w is not None:
                attention = torch.empty((n, b, self.max_len, attn_w.shape[2]), dtype=torch.float32, device=dev)
                hip.beam_gather_attention(attn_w, self.src, o_idx, o_len, attention)
            if self.logprobs:
                logprobs = torch.empty((n, b, self.max_len), dtype=torch.float32, device=dev)
                hip.beam_gather_logprobs(self.lp_w, self.par_w, o_idx, o_len, logprobs, pos=pos, first_pos=self.first_pos)
            if best:
                o_drawn.zero_()           # (the kernel's draw among the beams is not this search's: slot 0, the best score, is returned)
            captions = BeamCaptions(out.long(), o_len.long(), o_score, o_idx.long(), o_drawn.long(), o_row.long())
            if best and not beams and attn_w is None and not self.logprobs:
                captions = (captions.tokens[:, 0], captions.row_lengths)
        else:
            attention = None
            out = torch.empty((self.n_img, self.max_len), dtype=torch.int32, device=self.device)
            out_len = torch.empty((self.n_img,), dtype=torch.int32, device=self.device)
            hip.beam_finalize(self.tokens, self.vals, self.done, self.end_step, out, out_len, self.n_img, self.beam_size,
                              len_bias_done, full_len, pad_index, self.temperature, noise, self.seed, self.img0,
                              seed_ptr=self.seed_tensor)
            captions = (out.long(), out_len.long())
        if defer_check:
            return SessionResult(captions, self.err, attention, logprobs)
        self.check()
        return SessionResult(captions, None, attention, logprobs)

    def check(self):
        """Raises like the reference does when every logit of a row was filtered (beam.py:46)."""
        self.raise_for(int(self.err.item()), self.top_p if self.exact else 1.0)

    @staticmethod
    def raise_for(code, top_p=1.0):
        """``top_p < 1``: the word of a session that already ran ``exact=True`` with a nucleus -- its overflow has no further
        fall-back."""
        if code == 0:
            return
        if code & hip.ERR_NONFINITE:
            # torch.multinomial's message for a probability row holding NaN (softmax over logits with a NaN or +inf among them)
            raise RuntimeError("probability tensor contains either `inf`, `nan` or element < 0 (a row's logits hold NaN or +inf)")
        if code & hip.ERR_ALL_FILTERED:
            raise RuntimeError("probability tensor contains either `inf`, `nan` or element < 0 "
                               "(every logit of a row was filtered: <unk> was the only top-k token)")
        if code & hip.ERR_OVERFLOW and top_p < 1.0:
            raise BeamOverflow(f"more than 1024 logits of a row survive its top-k filter (DH_BEAM_MAX_SURVIVORS) and top_p={top_p} takes the "
                               "nucleus among at most that many: flat logits have no nucleus draw, exact=True included -- use top_p=1.0")
        if code & hip.ERR_OVERFLOW:
            raise BeamOverflow("more than 1024 logits of a row tie at its top-k threshold (DH_BEAM_MAX_SURVIVORS): repeat with exact=True")
        # hip.ERR_TOO_FEW (fewer positive-probability tokens than beams: top_k == beam_size with <unk> in the top-k, or
        # beam_size >= num_tokens) is NOT an error: torch.multinomial of the torch versions this was pinned against fills the
        # remaining slots with zero-probability tokens, the kernels with <pad> at score -inf -- a dead beam either way, which no
        # later draw can pick.  The randomised sweep (tools/fuzz_generate.py) reproduces the reference token for token in all such
        # cases.  (torch <= 1.x raised "invalid multinomial distribution" here.)  The bit stays readable in ``helper.err``.

    def all_ended(self):
        """Host-visible early-exit test (one sync; callers poll it sparsely, not per token).  Engine use: every image's beams
        have ended (`done`); method-surface use (beam.py:110-112): every flag of the caller-visible ``has_ended``."""
        if self.has_ended is not self._ended:
            return bool(self.has_ended.cpu().numpy().all())
        return bool(self.done.cpu().numpy().all())

    # ---- the reference's method surface (beam.py:32-108): same names, argument meaning, shapes, dtypes and in-place behaviour,
    # each method one HIP launch.  Host-driven like the reference's own loops (rnn_models.py:87-128, transformers.py:532-569):
    # sample_k_indices reads the device error word (one sync per draw) so that it raises where torch.multinomial raises.
    def _draw_noise(self, shape):
        """Exp(1) noise of one multinomial call: the ``noise_source`` hook (``("multinomial", call number, shape)``) or Philox."""
        self._draws += 1
        if self.noise_source is None:
            return None
        t = self.noise_source("multinomial", self._draws - 1, shape)
        return None if t is None else t.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()

    def _no_nucleus(self, what):
        if self._history_edits:
            raise NotImplementedError(f"{what} with no_repeat_ngram_size / repetition_penalty: the history edits live in the batched "
                                      "engine's row draw (step / step_prompted); the reference-style method surface has none")
        if self._constraints:
            raise NotImplementedError(f"{what} with min_len / bad_words_ids: the bans live in the batched engine's row draw (step / "
                                      "step_prompted); the reference-style method surface has none")
        if self.sequence_bias is not None:
            raise NotImplementedError(f"{what} with sequence_bias: the biases live in the batched engine's row draw (step / "
                                      "step_prompted); the reference-style method surface has none")
        if self.search == "beam":
            raise NotImplementedError(f'{what} with search="beam": the deterministic search lives in the batched engine\'s steps (step / '
                                      "step_prompted); the reference-style method surface draws")
        if self.top_p < 1.0:
            raise NotImplementedError(f"{what} with top_p < 1: the nucleus lives in the batched engine's row draw (step / step_prompted); "
                                      "the reference-style method surface has none")

    def filter_top_k(self, logits):
        """beam.py:32-37: IN PLACE -- entries strictly below the row's ``top_k``-th largest value and the ``unk`` column become
        ``-inf`` (ties at the threshold stay); returns its argument."""
        hip.beam_filter_top_k(logits, self.top_k, self.unk_index)
        return logits

    def sample_k_indices(self, logits, k=None):
        """beam.py:39-48: ``torch.multinomial(softmax(logits / temperature), k)`` (no replacement) as an Exp(1) race on the
        device; ``logits`` is ``[n, V]`` -> int64 ``[n, k]`` or 1-D ``[V]`` -> ``[k]`` (the candidate draws, rnn_models.py:120)."""
        self._no_nucleus("sample_k_indices")
        k = self.beam_size if k is None else int(k)
        x = logits if logits.dim() == 2 else logits.reshape(1, -1)
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            raise TypeError("sample_k_indices expects fp32 logits with unit column stride")
        out = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
        self.err.zero_()
        hip.beam_sample_k(x, k, self.temperature, self._draw_noise(tuple(x.shape)), self.seed, self.img0, self._draws, out, self.err,
                          seed_ptr=self.seed_tensor)
        code = int(self.err.item())
        self.raise_for(code)            # (fewer positive entries than k: the zero-probability ones follow in index order, as
                                        #  current torch.multinomial returns them in an unspecified order -- no error)
        return out if logits.dim() == 2 else out[0]

    @staticmethod
    def filter_by_indices(values, indices):
        """beam.py:50-53: ``torch.gather(values, 1, indices)``."""
        out = torch.empty(indices.shape, dtype=torch.float32, device=values.device)
        hip.beam_gather(values, indices.contiguous(), out)
        return out

    def process_logits(self, logits, sample_seq, sample_val):
        """beam.py:55-108.  ``logits [n, V]`` fp32 (filtered IN PLACE, as the reference does), ``sample_seq [n, L]`` int64,
        ``sample_val [n]`` or ``[n, 1]``, ``self.has_ended [n]`` -> ``(prev_seqs, prev_vals), (new_ind, new_val)`` over the
        ``n_cand = sum(1 if ended else beam_size)`` candidates; ``self.has_ended`` becomes the ``[n_cand]`` bool flags."""
        self._no_nucleus("process_logits")
        b = self.beam_size
        logits = self.filter_top_k(logits)
        new_ind = self.sample_k_indices(logits, k=b)
        gathered = self.filter_by_indices(logits, new_ind)
        ended = self.has_ended
        ended = ended.view(torch.uint8) if ended.dtype == torch.bool else ended.to(torch.uint8)
        ended = ended.to(logits.device).contiguous()
        n = ended.shape[0]
        if logits.shape[0] != n or sample_seq.shape[0] != n:
            raise IndexError(f"process_logits: {logits.shape[0]} logit rows / {sample_seq.shape[0]} sequences for {n} has_ended flags")
        n_cand = int(sum(1 if e else b for e in ended.cpu().tolist()))
        seqs = sample_seq.to(torch.int64).contiguous()
        vals = sample_val.to(torch.float32).contiguous()
        dev = logits.device
        prev_seqs = torch.empty((n_cand, seqs.shape[1]), dtype=torch.int64, device=dev)
        prev_vals = torch.empty((n_cand,) + tuple(vals.shape[1:]), dtype=torch.float32, device=dev)
        out_ind = torch.empty((n_cand,), dtype=torch.int64, device=dev)
        out_val = torch.empty((n_cand,), dtype=torch.float32, device=dev)
        out_ended = torch.empty((n_cand,), dtype=torch.uint8, device=dev)
        hip.beam_expand(new_ind, gathered, ended, seqs, vals, b, self.eos_index, prev_seqs, prev_vals, out_ind, out_val, out_ended)
        self.has_ended = out_ended.view(torch.bool)
        return (prev_seqs, prev_vals), (out_ind, out_val)


def make_noise_source(rng, seed, noise_source, lo, hi, img0, state0=None):
    """The noise source of one decode session (images ``[lo, hi)`` of the batch): the caller's hook, or the torch-generator replay
    of ``rng="torch"`` (``TorchRngNoise``); ``rng`` None / "philox" = the kernels' own counter-based generator."""
    if rng in (None, "philox"):
        return noise_source
    if rng != "torch":
        raise ValueError(f'rng must be None, "philox" or "torch", not {rng!r}')
    if noise_source is not None:
        raise ValueError('rng="torch" and noise_source are mutually exclusive')
    return TorchRngNoise(seed, hi - lo, img0 + lo, state0=state0)


def check_ids(ids, n, capturing_ok=True, lengths=None):
    """``nn.Embedding``'s ``IndexError`` for ids outside ``[0, n)`` (reference: every token / label lookup).  The kernels gather rows by
    these ids without a bounds test, so an id outside the table would read foreign memory (round 5: a GPU memory fault on a label of -3,
    silent garbage on a token of V + 100): checked on the host, two scalars per call.  Inside a hipGraph capture nothing can be read
    back: ``generate_batch_graphed`` checks its inputs before the replay instead.  ``lengths`` (``[rows]``, prompted batches): only
    ``ids[i, :lengths[i]]`` is looked at -- the rest of a row is padding that no kernel reads."""
    if ids is None or ids.numel() == 0:
        return
    if ids.is_cuda and capturing_ok and torch.cuda.is_current_stream_capturing():
        return
    if lengths is not None:
        used = torch.arange(ids.shape[1], device=ids.device)[None, :] < torch.as_tensor(lengths).to(ids.device)[:, None]
        ids = ids[used]
        if ids.numel() == 0:
            return
    lo, hi = torch.aminmax(ids)
    if int(lo) < 0 or int(hi) >= n:
        raise IndexError("index out of range in self")


def check_prompts(caption, caption_lengths, max_len, num_tokens):
    """Validation of a prompted batch (``generate_batch(..., caption=C, caption_lengths=L)``): ``C`` int64 ``[N, P]``, ``L`` int64 or
    int32 ``[N]`` with ``0 <= L[i] <= P``; image ``i``'s prompt is ``C[i, :L[i]]`` and must leave at least one decode step
    (``L[i] + 1 < max_len``: the reference's degenerate returns for a prompt that fills ``max_len - 1`` exist on the dense path only).
    Token ids are range-checked over the used part of every row only (``check_ids``).  Host work (one read of ``L`` if it lives on
    the device).  Returns ``L`` as an int64 CPU tensor, or ``None`` without ``caption_lengths``."""
    if caption_lengths is None:
        return None
    if caption is None:
        raise ValueError("caption_lengths without caption: pass the padded prompts as caption=[N, P]")
    if caption.dim() != 2:
        raise ValueError(f"caption must be [N, P] with caption_lengths, got shape {tuple(caption.shape)}")
    lens = torch.as_tensor(caption_lengths)
    if lens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"caption_lengths must be int64 or int32, not {lens.dtype}")
    if lens.dim() != 1 or lens.shape[0] != caption.shape[0]:
        raise ValueError(f"caption_lengths must have shape [{caption.shape[0]}] (one length per caption row), got {tuple(lens.shape)}")
    host = lens.detach().cpu().to(torch.int64)
    if host.numel():
        lo, hi, p = int(host.min()), int(host.max()), caption.shape[1]
        if lo < 0 or hi > p:
            raise ValueError(f"caption_lengths must lie in [0, {p}] (the width of caption), found {lo if lo < 0 else hi}")
        if hi + 1 >= max_len:
            raise ValueError(f"a prompt of {hi} tokens leaves no decode step at max_len={max_len}: caption_lengths[i] + 1 < max_len "
                             "is required (use the dense caption=[N, p] call for the reference's behaviour in that case)")
    check_ids(caption, num_tokens, capturing_ok=False, lengths=host)
    return host


def prompts_need_philox(rng, noise_source):
    """A prompted batch draws with the kernels' Philox generator only."""
    if rng == "torch" or noise_source is not None:
        raise ValueError('caption_lengths needs the Philox generator: rng="torch" and noise_source draw in per-image shapes that '
                         "differ by phase (dense caption=[N, p] calls, one per prompt length, support them)")


def prompt_session_inputs(caption, caption_lengths, max_len, num_tokens, device, rng=None, noise_source=None, no_host_read=False):
    """What the decoders' prompted sessions need, or ``None`` for a dense call: ``(caption [N, pw] on the device, first_pos int32
    [N] on the device, the lengths as a Python list or None)``.  ``pw = min(P, max_len - 2)``: no valid prompt is longer.
    ``no_host_read`` (``defer_check`` / hipGraph capture) with device-resident lengths: nothing is read back -- the caller has
    validated them (``generate_batch_graphed`` does, before every replay) and the session treats ``0 .. pw`` as the mixed range."""
    if caption_lengths is None:
        return None
    prompts_need_philox(rng, noise_source)
    lens = torch.as_tensor(caption_lengths)
    host = None
    if not (lens.is_cuda and (no_host_read or torch.cuda.is_current_stream_capturing())):
        host = check_prompts(caption, lens, max_len, num_tokens).tolist()
    elif caption is None:
        raise ValueError("caption_lengths without caption: pass the padded prompts as caption=[N, P]")
    pw = max(0, min(caption.shape[1], max_len - 2))
    first_pos = lens.to(device=device, dtype=torch.int32).contiguous()
    return caption[:, :pw].to(device), first_pos, host


def session_inputs(settings, caption, caption_lengths, max_len, num_embeddings, device, seed, rng, noise_source, defer_check):
    """What both decoders' sessions settle before their first launch: ``(prompts, rng, noise_source, rng_seed, seed, rng_state0)``.
    ``search="beam"`` draws nothing, so no generator is read and no noise source is asked; ``prompts``: ``prompt_session_inputs``' triple
    or ``None`` for a dense call, whose ``caption`` ids are range-checked here; ``rng_seed``: the caller's seed, which
    ``rng="torch"`` replays generators from (``TorchRngNoise``), while ``seed`` is the Philox key (``resolve_seed``); ``rng_state0``:
    the default generator's state under ``rng="torch"`` with no seed, snapshotted once per call so that a repeated session
    (``BeamOverflow`` retry) replays the same draws."""
    if settings.search == "beam":
        rng, noise_source, seed = None, None, 0
    prompts = prompt_session_inputs(caption, caption_lengths, max_len, num_embeddings, device, rng, noise_source, no_host_read=defer_check)
    if prompts is None:
        check_ids(caption, num_embeddings)
    rng_seed = seed
    seed = 0 if rng == "torch" else resolve_seed(seed, noise_source)
    rng_state0 = torch.get_rng_state() if (rng == "torch" and rng_seed is None) else None
    return prompts, rng, noise_source, rng_seed, seed, rng_state0


def check_lengths(lengths, steps):
    """``pack_padded_sequence``'s errors for the teacher-forced LSTM forward (reference rnn_models.py:39)."""
    if int(lengths.min()) <= 0:
        raise RuntimeError("Length of all samples has to be greater than 0, but found an element in 'lengths' that is <= 0")
    if int(lengths.max()) > steps:
        raise RuntimeError(f"Expected sequence length to be larger than or equal to the maximum of lengths, but got sequence length {steps} and max length {int(lengths.max())}")


def classifier_must_be_finite(plan):
    """A NaN or inf in the classifier's weight or bias is in every row's logits: the reference's ``torch.multinomial`` raises on the
    first draw (beam.py:46).  The full-row samplers see such a logit (it sorts above everything) and flag ERR_NONFINITE; the
    group-maximum pre-filter of the 16-bit paths would not (``max`` drops NaN), so generate checks the operands once per plan."""
    ok = plan.get("_cls_finite")
    if ok is None:
        ok = plan["_cls_finite"] = bool(torch.isfinite(plan["cls_w"]).all()) and bool(torch.isfinite(plan["cls_b"]).all())
    if not ok:
        raise RuntimeError("probability tensor contains either `inf`, `nan` or element < 0 (the classifier's weight or bias holds NaN or inf)")


def call_logits_hook(hook, pos, logits, helper):
    """``logits_hook(pos, logits)`` before the beam step of position ``pos``; a hook whose attribute ``with_tokens`` is true is called
    ``hook(pos, logits, tokens)`` with the engine's int32 ``[rows, max_len]`` token table (row r's own history in columns < pos):
    what a checker needs to re-run a row teacher-forced (tests/test_fullsize_gpu.py)."""
    if getattr(hook, "with_tokens", False):
        hook(pos, logits, helper.tokens)
    else:
        hook(pos, logits)


_overflow_warned = False


def warn_overflow_retry():
    """One warning per process when a batch is decoded a second time through the general sampler (``BeamOverflow``): user hooks
    (``logits_hook``, ``noise_source``) then fire once more for the same steps."""
    global _overflow_warned
    if not _overflow_warned:
        _overflow_warned = True
        import warnings
        warnings.warn("deephumor_amd: a row had more logits tied at its top-k threshold than the pre-filtered samplers hold (flat "
                      "logits); the batch is decoded again with exact=True -- logits_hook / noise_source callbacks run a second time",
                      RuntimeWarning, stacklevel=3)


def resolve_seed(seed, noise_source=None):
    """``seed=None`` (the default of every ``generate``): a fresh 62-bit Philox key drawn from torch's default CPU
    generator -- the generator the reference's ``torch.multinomial`` calls consume (beam.py:46) -- so ``torch.manual_seed``
    controls ``generate`` and successive calls give different captions, as with the reference.  An int is used as is.
    With caller-supplied noise (RNG-replay parity tests) the Philox key is unused and nothing is drawn."""
    if seed is None and noise_source is not None:
        return 0
    if seed is None:
        return int(torch.randint(0, 1 << 62, (), dtype=torch.int64).item())
    return int(seed)


class SessionResult(NamedTuple):
    """What a decode session returns (``BeamSearchHelper.finalize``): ``captions`` -- the ``(tokens, lengths)`` pair or a
    ``BeamCaptions`` --, ``err`` -- the device error word of a ``defer_check`` session, else ``None`` --, and ``attention`` -- the kept
    beams' maps fp32 ``[n, B, T, S]`` of a ``return_attention`` session (whose ``captions`` are a ``BeamCaptions``), else ``None`` --,
    and ``logprobs`` -- the kept beams' per-token log-probabilities fp32 ``[n, B, T]`` of a ``return_logprobs`` session (whose
    ``captions`` are a ``BeamCaptions`` too), else ``None``."""
    captions: object
    err: object = None
    attention: object = None
    logprobs: object = None

    def record_stream(self, stream):
        for t in (*self.captions, self.err, self.attention, self.logprobs):
            if t is not None:
                t.record_stream(stream)

    @staticmethod
    def cat(parts):
        """The images of several sessions, in order; the error word is the OR of theirs."""
        first = parts[0]
        caps = [p.captions for p in parts]
        caps = BeamCaptions.cat(caps) if isinstance(first.captions, BeamCaptions) else tuple(torch.cat(ts, 0) for ts in zip(*caps))
        err = None
        if first.err is not None:
            err = first.err.clone()
            for p in parts[1:]:
                err |= p.err
        return SessionResult(caps, err, None if first.attention is None else torch.cat([p.attention for p in parts], 0),
                             None if first.logprobs is None else torch.cat([p.logprobs for p in parts], 0))

    def public(self, return_beams=False):
        """What ``generate_batch`` returns: the pair or the ``BeamCaptions``; behind it ``attention`` -- ``[N, B, T, S]`` for
        ``return_beams``, else the drawn slot's maps ``[N, T, S]`` behind ``best()``, the plain pair bit for bit --; behind that
        ``logprobs`` -- ``[N, B, T]``, or the drawn slot's ``[N, T]`` in the same way --; last the error word of a ``defer_check``
        call.  One element alone is returned as it is."""
        caps, att, lp = self.captions, self.attention, self.logprobs
        if (att is not None or lp is not None) and not return_beams:
            rows = torch.arange(caps.drawn.shape[0], device=caps.drawn.device)
            att = None if att is None else att[rows, caps.drawn]
            lp = None if lp is None else lp[rows, caps.drawn]
            caps = caps.best()
        out = (caps,) if isinstance(caps, BeamCaptions) else tuple(caps)
        out += tuple(t for t in (att, lp, self.err) if t is not None)
        return out[0] if len(out) == 1 else out


class DecodeSession:
    """What every decode session of both decoders sets up around its position loop: the ``helper`` (``settings.new_helper``), the
    fp32 ``logits [rows, V]`` and -- where the classifier fills them (16-bit paths, f32x planes) -- the 64-column ``group_max``, both
    padded to whole 256-column chunks (vocab_wreg; rows are 16-byte aligned for vector stores); the teacher-forced beginning
    (``set_prefix`` / ``set_prompts``: ``pos`` the dense prefix length, ``pmin`` / ``pmax`` the shortest and longest prompt); and the
    ``early_stop_every`` test.  ``plan=None``: no buffers (the re-forward decoder's logits are the classifier's own output)."""

    def __init__(self, helper, plan=None, num_tokens=0, early_stop_every=0, pad_index=0):
        self.helper, self.early_stop_every, self.pad_index = helper, early_stop_every, pad_index
        self.pos = self.pmin = self.pmax = 0
        self.logits = self.group_max = None
        if pad_index != 0:
            helper.tokens.fill_(pad_index)
        if plan is not None:
            rows, chunks, dev = helper.n_img * helper.beam_size, (num_tokens + 255) // 256, helper.device
            self.logits = torch.empty((rows, 256 * chunks), device=dev)[:, :num_tokens]
            if plan["dtype"] in hip.HALF_DTYPES or plan.get("f32_planes"):
                self.group_max = torch.empty((rows, 4 * chunks), device=dev)[:, :hip.n_groups(num_tokens)]

    def set_prefix(self, caption, lo, hi):
        """The dense prefix ``caption[lo:hi]`` (``None``: none) -> ``pos``, the first generated column."""
        if caption is not None:
            self.pos = self.pmin = self.pmax = caption.shape[1]
            self.helper.set_prefix(caption[lo:hi])
        return self.pos

    def set_prompts(self, prompts, lo, hi):
        """``prompts``: ``prompt_session_inputs``' triple.  Without host lengths (nothing may be read back) every position the
        prompts span counts as mixed."""
        cap, first_pos, host = prompts
        self.pmin, self.pmax = (min(host[lo:hi]), max(host[lo:hi])) if host is not None else (0, cap.shape[1])
        self.helper.set_prompts(cap[lo:hi], first_pos[lo:hi], self.pad_index)

    def all_done(self, i):
        """The reference's ``all_ended()`` break, tested every ``early_stop_every`` positions behind the last forced one (one host
        sync per test): finished images are frozen by ``dh_beam_select``, so nothing is left to do."""
        every = self.early_stop_every
        return bool(every and i > self.pmax and (i - self.pmax) % every == 0 and bool(self.helper.done.all()))


def decode_with_overflow_retry(run, exact, rng_state0=None):
    """``run(exact)``; flat logits -- more ties at a row's top-k threshold than the fast samplers hold (``BeamOverflow``) -- once more
    with ``exact=True``: every row draw through the general sampler (same seed: same captions where nothing overflowed), torch's
    default generator put back to ``rng_state0`` first where one is given.  With ``exact`` already on the overflow is the caller's."""
    try:
        return run(bool(exact))
    except BeamOverflow:
        if exact:
            raise
        warn_overflow_retry()
        if rng_state0 is not None:
            torch.set_rng_state(rng_state0)
        return run(True)


_STREAMS = {}


def run_interleaved(make_session, n_img, n_streams):
    """Runs ``make_session(lo, hi)`` -- a generator that decodes images ``[lo, hi)`` and yields after every
    position, returning a ``SessionResult`` -- either once, or as ``n_streams`` image sub-batches advanced
    round-robin on separate HIP streams.  Decode positions are chains of small, latency-bound kernels
    (a 640-row GEMM fills a fraction of the 256 CUs); two independent chains in flight fill the gaps.
    Captions are unchanged: every image's noise is keyed by its global index (``img0 + lo``)."""
    n_streams = max(1, min(n_streams, n_img))
    if n_streams == 1:
        gen = make_session(0, n_img)
        while True:
            try:
                next(gen)
            except StopIteration as e:
                return e.value
    main = torch.cuda.current_stream()
    dev = main.device
    pool = _STREAMS.setdefault(dev, [])
    while len(pool) < n_streams:
        pool.append(torch.cuda.Stream(device=dev))
    base, extra = divmod(n_img, n_streams)
    bounds, lo = [], 0
    for i in range(n_streams):
        hi = lo + base + (1 if i < extra else 0)
        bounds.append((lo, hi))
        lo = hi
    gens, results, alive = [], [None] * n_streams, set(range(n_streams))
    for (lo, hi), st in zip(bounds, pool):
        st.wait_stream(main)
        gens.append(make_session(lo, hi))
    while alive:
        for i in sorted(alive):
            with torch.cuda.stream(pool[i]):
                try:
                    next(gens[i])
                except StopIteration as e:
                    results[i] = e.value
                    alive.discard(i)
    for st in pool[:n_streams]:
        main.wait_stream(st)
    for r in results:
        r.record_stream(main)
    return SessionResult.cat(results)
