"""Prints what ``tests/text_occlusion_ref.WORST`` / ``WORST_16`` record, on the GPU: ``|text_occlusion - want|`` of (base, drop, token_drop)
per kind, level, fill and type, ``want`` = golden G29 or the fp32 restatement of ``tests/text_occlusion_ref.py`` on the model's own
weights; then the fp32 worst over both settings of ``f32_split`` as ``WORST`` entries and the 16-bit values against G29.  Its output is
``profiles/text_occlusion/errors.txt``.  Information, not a gate: the tests gate, and print the same figures under ``-s``.

    python tools/text_occlusion_errors.py > profiles/text_occlusion/errors.txt
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import explain_ref as E, text_occlusion_ref as T
import test_text_occlusion_gpu as G
from deephumor_amd import hip
from helpers import synth_images
hip.load()
data = tuple(t.cuda() for t in T.inputs(synth_images(E.N_TEMPLATES, seed=0)))
worst = {}
def note(key, got, want):
    e = tuple(float(np.abs(a.double().cpu().numpy() - np.asarray(b)).max()) for a, b in zip(got, want))
    worst[key] = tuple(max(x, y) for x, y in zip(e, worst.get(key, (0, 0, 0))))
    return e
for kind in E.KINDS:
    g = T.golden(kind)
    for tag, dt, opts in G.SETTINGS:
        model = G.build(kind, dt)
        with hip.option_scope(**opts):
            for name, fill in (("pad", "pad"), ("unk", 1)):
                got = G.occl(model, kind, data, dt, fill=fill, return_tokens=True)
                k = (kind, "history", name)
                e1 = note(k + ("g29", tag), got, (g["base"], g[f"hist_{name}_drop"], g[f"hist_{name}_tokens"]))
                e2 = note(k + ("restatement", tag), got, G.restated(kind)[("history", name)])
                print(tag, k, "g29", e1, "restatement", e2, flush=True)
            if kind in T.LABEL_KINDS:
                got = G.occl(model, kind, data, dt, level="label", fill=1, return_tokens=True)
                k = (kind, "label", "unk")
                e1 = note(k + ("g29", tag), got, (g["label_base"], g["label_drop"], g["label_tokens"]))
                e2 = note(k + ("restatement", tag), got, G.restated(kind)[("label", "unk")])
                print(tag, k, "g29", e1, "restatement", e2, flush=True)
print("==== WORST (fp32, both settings)")
keys = sorted({k[:4] for k in worst})
for k in keys:
    v = tuple(max(worst[k + ("f32_split",)][i], worst[k + ("f32_exact",)][i]) for i in range(3))
    print(f'    ("{k[0]}", "{k[1]}", "{k[2]}", "{k[3]}"): ({v[0]:.3e}, {v[1]:.3e}, {v[2]:.3e}),')
print("==== 16-bit against G29")
for k in keys:
    if k[3] == "g29":
        print(k[:3], {t: tuple(f"{x:.3e}" for x in worst[k + (t,)]) for t in ("f16", "bf16")})
