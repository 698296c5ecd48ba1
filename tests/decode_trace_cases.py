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


def fixture_name(kind):
    return f"g24_decode_trace_{kind}.npz"


@functools.lru_cache(maxsize=2)
def build(kind, tag, pad_index=0):
    """The synthetic model of ``kind`` in dtype ``tag`` on the GPU (kept while its cases run: a graph cache lives on it)."""
    import deephumor_amd.models as M
    sd, hp = synthetic_sd(kind)
    model = getattr(M, kind)(**(dict(hp, pad_index=pad_index) if pad_index else hp)).eval()
    model.load_state_dict(sd)
    return model.cuda().to(DTYPES[tag])


def fields(res):
    """Any public result as ``{name: tensor}``."""
    if torch.is_tensor(res):                           # generate: the caption
        return {"tokens": res}
    if hasattr(res, "_fields"):                        # a BeamCaptions
        return dict(zip(res._fields, res))
    if hasattr(res[0], "_fields"):                     # (BeamCaptions, attention)
        return dict(fields(res[0]), attention=res[1])
    if len(res) == 3:
        return dict(zip(("tokens", "lengths", "attention"), res))
    if res[1].is_floating_point():                     # generate with return_attention: (caption, its map)
        return dict(zip(("tokens", "attention"), res))
    return dict(zip(("tokens", "lengths"), res))


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


def pipeline(model, images, **extra):
    """Two batches of three host images through ``CaptionPipeline``, seeds 1 and 2; every field of both results."""
    from deephumor_amd.pipeline import CaptionPipeline
    kw = {k: v for k, v in KW.items() if k != "seed"}
    pipe = CaptionPipeline(model, **kw, **CONTROLS, **extra)
    out = {}
    for i, res in enumerate(pipe.run([(images[:3],), (images[1:],)], seeds=[1, 2])):
        out.update((f"batch{i}_{k}", v) for k, v in to_numpy(res).items())
    return out


@functools.lru_cache(maxsize=1)
def _images():
    return synth_images(4, seed=0)


def _cases(kind, tag):
    """Thunks only: nothing touches the GPU (or builds an image) until one is called."""
    three = lambda: _images()[:3].cuda()
    model = lambda pad_index=0: build(kind, tag, pad_index)

    def batch(pad_index=0, caption=None, **kw):
        def call():
            cap = {} if caption is None else {"caption": caption.cuda()}
            return model(pad_index).generate_batch(three(), **KW, **cap, **kw)
        return lambda: traced(call)
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


def cases(kind):
    """``{"<dtype>/<case>": thunk}`` in running order; ``thunk()`` runs the case on the GPU and returns ``{field: numpy array}``."""
    return {f"{tag}/{name}": thunk for tag in DTYPES for name, thunk in _cases(kind, tag).items()}
