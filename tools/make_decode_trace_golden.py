"""Records golden G24 (``tests/golden/g24_decode_trace_<kind>.npz``): the ordered ``hip._launch`` entry-point names and every returned
tensor, bit for bit, of the decode layer's routes -- ``generate_batch`` with and without every control, prefix, prompts, streams,
``exact``, the re-forward decoder, ``generate_batch_graphed``, ``CaptionPipeline`` and single-image ``generate``, in bf16 and fp32
(the cases: ``tests/decode_trace_cases.py``, which ``tests/test_decode_trace_gpu.py`` replays).

Needs the GPU, not the reference: the fixture is what THIS tree does, recorded in front of a change to the Python decode layer that
must move no launch and no bit.  Every case is run twice here and must repeat itself before it is written.

    python tools/make_decode_trace_golden.py [--search] [kind ...]

``--search``: golden G25 (``g25_decode_trace_search_<kind>.npz``, ``decode_trace_cases.search_cases``) -- the settings behind
``search``: beam search, log-probabilities, the length penalty, the pool, the groups and the biases.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decode_trace_cases as dt                                            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    args = [a for a in sys.argv[1:] if a != "--search"]
    table, fixture = (dt.search_cases, dt.search_fixture_name) if "--search" in sys.argv else (dt.cases, dt.fixture_name)
    for kind in (args or dt.KINDS):
        fix = {}
        for key, thunk in table(kind).items():
            got, again = thunk(), thunk()
            assert got.keys() == again.keys(), key
            for name, arr in got.items():
                assert arr.dtype == again[name].dtype and np.array_equal(arr, again[name], equal_nan=arr.dtype.kind == "f"), (key, name)
                fix[f"{key}/{name}"] = arr
            print(kind, key, {k: tuple(v.shape) for k, v in got.items()}, flush=True)
        path = os.path.join(OUT, fixture(kind))
        np.savez_compressed(path, **fix)
        print(path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
