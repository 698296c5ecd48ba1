"""The cases of golden G24 (``tests/golden/g24_decode_trace_<kind>.npz``): what the Python decode layer launches and returns on
every route it has -- written once here, run by the recorder (``tools/make_decode_trace_golden.py``) and by the replay
(``tests/test_decode_trace_gpu.py``).

Only public calls: ``generate_batch`` / ``generate`` / ``generate_batch_graphed``, ``CaptionPipeline``, and a wrapper around
``hip._launch`` that notes the entry-point name.  Three images, beam 3, ``top_k`` 10, ``max_len`` 8, seed 1: compact and full
rows, positions with and without a ban launch (``min_len`` 3), and prompt lengths 0 / 2 / 4 for all three prompted phases in one
batch.  A case is keyed ``"<dtype>/<case>"`` and stores every tensor its call returns; the traced ones also store ``launches``,
the ordered entry-point names of the SECOND call (the first builds the plans):

    a        defaults                                                   launches + outputs
    b        every control on (``CONTROLS``)                            launches + outputs
    c        ``return_beams=True``                                      launches + outputs
    d        ``return_attention=True`` (Transformer only)               launches + outputs
    e        b behind a dense ``[3, 2]`` prefix                         launches + outputs
    f        b behind prompts ``[3, 4]`` of lengths 0 / 2 / 4           launches + outputs
    g        b on two streams                                           launches + outputs
    h        b with ``exact=True``                                      launches + outputs
    i_a i_b  a and b on a Transformer with ``pad_index=1`` (re-forward) launches + outputs
    j_a j_b  a and b through ``generate_batch_graphed``                 the second replay's outputs
    k_b k_b_beams  ``CaptionPipeline``, two batches of 3, b / b + beams outputs
    l        single-image ``generate``, b                               outputs

Golden G25 (``tests/golden/g25_decode_trace_search_<kind>.npz``, ``search_cases``) holds the settings behind ``search`` the same way --
``BEAM`` is ``search="beam"``, ``GROUPS`` that with ``beam_size=4, num_beam_groups=2, diversity_penalty=0.5``:

    beam beams_logprobs length      ``BEAM``; + ``return_beams`` and ``return_logprobs``; + ``length_penalty=1.0``   launches + outputs
    stop_true stop_false            ``BEAM`` + ``early_stopping``                                                   launches + outputs
    stop_pool stop_full             ``stop_true`` + ``return_beams`` and a bias towards ``<eos>``: some / only pool entries  launches + outputs
    groups groups_length groups_beams  ``GROUPS``; + ``length_penalty=1.0``; + ``return_beams``                      launches + outputs
    bias_logprobs                   ``search="sample"``, ``sequence_bias``, ``return_logprobs``                     launches + outputs
    bias_prompts                    b + ``sequence_bias`` behind the 0 / 2 / 4 prompts                              launches + outputs
    graphed_length                  ``BEAM`` + ``length_penalty=1.0`` through ``generate_batch_graphed``            the second replay's outputs
    pipe_groups pipe_groups_beams   ``CaptionPipeline``, ``GROUPS`` / + ``return_beams``                            outputs
    one                             single-image ``generate``, ``BEAM``                                             outputs
"""
import functools

import numpy as np
import torch

from helpers import synthetic_sd, synth_images

KINDS = ("CaptioningLSTM", "CaptioningTransformer")
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
KW = dict(beam_size=3, top_k=10, max_len=8, seed=1)
CONTROLS = dict(top_p=0.8, no_repeat_ngram_size=2, repetition_penalty=1.3, min_len=3, bad_words_ids=[[17], [230, 45]])
PREFIX = torch.tensor([[17, 230], [8, 9], [300, 301]])
PROMPTS = torch.tensor([[17, 230, 45, 7], [8, 9, 8, 11], [300, 301, 302, 303]])
PROMPT_LENGTHS = torch.tensor([0, 2, 4])


BEAM = dict(search="beam")
GROUPS = dict(search="beam", beam_size=4, num_beam_groups=2, diversity_penalty=0.5)
BIAS = {(17,): -2.0, (230, 45): 3.0, (8,): 1.5, (300, 8): -1.0}
EOS_BIAS = {(3,): 6.0}               # towards <eos>: the finished-hypothesis pool takes entries
EOS_FIRST = {(3,): 12.0}             # every row's best candidate is <eos>: behind ``min_len`` the pool is full within two positions


def fixture_name(kind):
    return f"g24_decode_trace_{kind}.npz"


def search_fixture_name(kind):
    return f"g25_decode_trace_search_{kind}.npz"


@functools.lru_cache(maxsize=2)
def build(kind, tag, pad_index=0):
    """The synthetic model of ``kind`` in dtype ``tag`` on the GPU (kept while its cases run: a graph cache lives on it)."""
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**(dict(hp, pad_index=pad_index) if pad_index else hp)).eval()
    model.load_state_dict(sd)
    return model.cuda().to(DTYPES[tag])


def fields(res):
    """Any public result as ``{name: tensor}``: a caption alone, a ``BeamCaptions``, or a tuple that begins with either (or with the
    ``tokens`` of the plain pair) and goes on with ``lengths``, ``attention`` (one dimension more than ``tokens``) and ``logprobs``."""
    if torch.is_tensor(res):                           # generate: the caption
        return {"tokens": res}
    if hasattr(res, "_fields"):                        # a BeamCaptions
        return dict(zip(res._fields, res))
    out = fields(res[0])
    for t in res[1:]:
        name = "lengths" if not t.is_floating_point() else "attention" if t.dim() > out["tokens"].dim() else "logprobs"
        assert name not in out, (name, [tuple(x.shape) for x in res[1:]])
        out[name] = t
    return out


def to_numpy(res):
    return {k: t.detach().cpu().numpy().copy() for k, t in fields(res).items()}


class Launches:
    """``with Launches() as names``: every ``hip._launch`` inside appends its entry-point name."""

    def __enter__(self):
        from deephumor_amd import hip
        self.hip, self.real, names = hip, hip._launch, []

        def noting(name, *a, **k):
            names.append(name)
            return self.real(name, *a, **k)
        hip._launch = noting
        return names

    def __exit__(self, *exc):
        self.hip._launch = self.real


def traced(call):
    """``call()`` twice; the second call's launches and outputs."""
    with torch.no_grad():
        call()
        with Launches() as names:
            out = to_numpy(call())
    out["launches"] = np.array(names)
    return out


def second(call):
    """``call()`` twice; the second call's outputs."""
    with torch.no_grad():
        call()
        return to_numpy(call())


def pipeline(model, images, controls=CONTROLS, **extra):
    """Two batches of three host images through ``CaptionPipeline``, seeds 1 and 2; every field of both results."""
    from deephumor_amd.pipeline import CaptionPipeline
    kw = {k: v for k, v in {**KW, **controls, **extra}.items() if k != "seed"}
    pipe = CaptionPipeline(model, **kw)
    out = {}
    for i, res in enumerate(pipe.run([(images[:3],), (images[1:],)], seeds=[1, 2])):
        out.update((f"batch{i}_{k}", v) for k, v in to_numpy(res).items())
    return out


@functools.lru_cache(maxsize=1)
def _images():
    return synth_images(4, seed=0)


def _cases(kind, tag, search=False):
    """Thunks only: nothing touches the GPU (or builds an image) until one is called."""
    three = lambda: _images()[:3].cuda()
    model = lambda pad_index=0: build(kind, tag, pad_index)

    def batch(pad_index=0, caption=None, **kw):
        def call():
            cap = {} if caption is None else {"caption": caption.cuda()}
            return model(pad_index).generate_batch(three(), **{**KW, **cap, **kw})
        return lambda: traced(call)
    if search:
        return _search_cases(model, three, batch)
    out = {"a": batch(), "b": batch(**CONTROLS), "c": batch(return_beams=True)}
    if kind == "CaptioningTransformer":
        out["d"] = batch(return_attention=True)
    out["e"] = batch(caption=PREFIX, **CONTROLS)
    out["f"] = batch(caption=PROMPTS, caption_lengths=PROMPT_LENGTHS, **CONTROLS)
    out["g"] = batch(streams=2, **CONTROLS)
    out["h"] = batch(exact=True, **CONTROLS)
    out["j_a"] = lambda: second(lambda: model().generate_batch_graphed(three(), **KW))
    out["j_b"] = lambda: second(lambda: model().generate_batch_graphed(three(), **KW, **CONTROLS))
    out["k_b"] = lambda: pipeline(model(), _images())
    out["k_b_beams"] = lambda: pipeline(model(), _images(), return_beams=True)
    out["l"] = lambda: second(lambda: model().generate(_images()[:1].cuda(), **KW, **CONTROLS))
    if kind == "CaptioningTransformer":
        out["i_a"], out["i_b"] = batch(pad_index=1), batch(pad_index=1, **CONTROLS)
    return out


def _search_cases(model, three, batch):
    """The second table (golden G25): the settings behind ``search``."""
    out = {"beam": batch(**BEAM),
           "beams_logprobs": batch(**BEAM, return_beams=True, return_logprobs=True),
           "length": batch(**BEAM, length_penalty=1.0),
           "stop_true": batch(**BEAM, early_stopping=True),
           "stop_false": batch(**BEAM, early_stopping=False),
           "stop_pool": batch(**BEAM, early_stopping=True, return_beams=True, sequence_bias=EOS_BIAS),
           "stop_full": batch(**BEAM, early_stopping=True, return_beams=True, sequence_bias=EOS_FIRST, min_len=3),
           "groups": batch(**GROUPS),
           "groups_length": batch(**GROUPS, length_penalty=1.0),
           "groups_beams": batch(**GROUPS, return_beams=True),
           "bias_logprobs": batch(search="sample", sequence_bias=BIAS, return_logprobs=True),
           "bias_prompts": batch(caption=PROMPTS, caption_lengths=PROMPT_LENGTHS, **CONTROLS, sequence_bias=BIAS)}
    out["graphed_length"] = lambda: second(lambda: model().generate_batch_graphed(three(), **KW, **BEAM, length_penalty=1.0))
    out["pipe_groups"] = lambda: pipeline(model(), _images(), controls=GROUPS)
    out["pipe_groups_beams"] = lambda: pipeline(model(), _images(), controls=GROUPS, return_beams=True)
    out["one"] = lambda: second(lambda: model().generate(_images()[:1].cuda(), **KW, **BEAM))
    return out


def cases(kind):
    """``{"<dtype>/<case>": thunk}`` in running order; ``thunk()`` runs the case on the GPU and returns ``{field: numpy array}``."""
    return {f"{tag}/{name}": thunk for tag in DTYPES for name, thunk in _cases(kind, tag).items()}


def search_cases(kind):
    """``cases`` for golden G25."""
    return {f"{tag}/{name}": thunk for tag in DTYPES for name, thunk in _cases(kind, tag, search=True).items()}
