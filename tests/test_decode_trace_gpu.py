"""Golden G24 replayed on a real MI355X: every route of the Python decode layer (``decode_trace_cases``) makes the launches, in the
order, and returns the tensors, bit for bit, that ``tools/make_decode_trace_golden.py`` recorded.  No tolerances.  Golden G25
(``search_cases``: the settings behind ``search``) is replayed the same way."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_trace_cases as dt  # noqa: E402
from helpers import golden  # noqa: E402

CASES = [(kind, key) for kind in dt.KINDS for key in dt.cases(kind)]


@pytest.fixture(scope="module")
def thunks():
    return {kind: dt.cases(kind) for kind in dt.KINDS}


def test_the_fixture_holds_exactly_these_cases():
    for kind in dt.KINDS:
        recorded = {k.rsplit("/", 1)[0] for k in golden(dt.fixture_name(kind)).files}
        assert recorded == set(dt.cases(kind)), kind


def _replay(table, fixture, kind, key):
    g = golden(fixture(kind))
    want = {k[len(key) + 1:]: g[k] for k in g.files if k.rsplit("/", 1)[0] == key}
    got = table(kind)[key]()
    assert got.keys() == want.keys(), (kind, key)
    if "launches" in want:
        assert got.pop("launches").tolist() == want.pop("launches").tolist(), (kind, key)
    for name, arr in want.items():
        assert got[name].dtype == arr.dtype and got[name].shape == arr.shape, (kind, key, name)
        assert torch.equal(torch.from_numpy(got[name]), torch.from_numpy(arr)), (kind, key, name)


SEARCH_CASES = [(kind, key) for kind in dt.KINDS for key in dt.search_cases(kind)]


def test_the_search_fixture_holds_exactly_these_cases():
    for kind in dt.KINDS:
        recorded = {k.rsplit("/", 1)[0] for k in golden(dt.search_fixture_name(kind)).files}
        assert recorded == set(dt.search_cases(kind)), kind


@pytest.mark.parametrize("kind,key", SEARCH_CASES, ids=[f"{kind}-search-{key}" for kind, key in SEARCH_CASES])
def test_search_route_replays_its_recording(kind, key):
    """Golden G25: the settings behind ``search`` -- launches by name and order, every returned tensor bit for bit."""
    _replay(dt.search_cases, dt.search_fixture_name, kind, key)


@pytest.mark.parametrize("kind,key", CASES, ids=[f"{kind}-{key}" for kind, key in CASES])
def test_route_replays_its_recording(kind, key, thunks):
    g = golden(dt.fixture_name(kind))
    want = {k[len(key) + 1:]: g[k] for k in g.files if k.rsplit("/", 1)[0] == key}
    got = thunks[kind][key]()
    assert got.keys() == want.keys(), (kind, key)
    if "launches" in want:
        assert got.pop("launches").tolist() == want.pop("launches").tolist(), (kind, key)
    for name, arr in want.items():
        assert got[name].dtype == arr.dtype and got[name].shape == arr.shape, (kind, key, name)
        assert torch.equal(torch.from_numpy(got[name]), torch.from_numpy(arr)), (kind, key, name)
