"""The sampled beam step on a real MI355X, every row-draw route: ``dh_beam_row_sample`` / ``_exact`` / ``_groups``, their prompted
twins and the nucleus entry against the fp64 restatement of ``tests/row_draw_ref.py`` with supplied noise AND with the restated
Philox noise; the sampled ``dh_beam_select`` bit for bit; the final draw of ``dh_beam_finalize_beams``.

Every launch reads a PADDED logits buffer (row stride = V rounded up to 256, plus 8; the pad columns hold +1e30 or NaN, the noise
table 0.0 there) and writes into pick tables pre-filled with a sentinel, two rows longer than the launch.  Picks are compared for
equality, so a row enters a case only if its race margin in the restatement is >= 1e-4 (``row_draw_ref.MARGIN``); a row below it is
redrawn from the next seed, never skipped.  Values: ``|got - want| <= 2e-6 + 2^-23 |want|``.  The tables and input builders of this
module need no GPU: ``tests/test_row_draw_ref_cpu.py`` checks routes, boundaries and margins of all of them."""
import collections
import functools
import time

import numpy as np
import pytest
import torch

import row_draw_ref as R
from beam_search_ref import State

pytestmark = pytest.mark.gpu

ROWS, UNK, EOS = 6, 1, 3
SENT_I, SENT_V = -7, -7.0
TOP_PS = (0.3, 0.8, 0.97)
FIRST_POS, STEPS = (0, 2), (0, 2, 3)
NINF = float("-inf")
PADS = (1e30, float("nan"))
T0 = time.time()
WORST = collections.defaultdict(float)        # route -> worst |value error| seen by this module's tests

# ---- B1: (V, top_k, beam, temperature) -- V on both sides of every dispatch boundary, fewer columns than threads, V = 3;
#      top_k in {1, 50, 256, 257}, beam in {1, 5, 64}, temperature in {0.7, 1.0, 1.3}
CASES = [(3, 3, 2, 1.0), (71, 50, 5, 1.3), (4096, 50, 5, 1.0), (4096, 257, 5, 0.7), (4097, 256, 64, 0.7), (16384, 256, 5, 1.3),
         (16384, 257, 64, 1.0), (16385, 50, 5, 0.7), (36864, 1, 1, 1.3), (36864, 50, 5, 1.0), (36865, 50, 5, 1.0), (65536, 256, 64, 1.3),
         (65536, 50, 1, 0.7), (65537, 50, 5, 0.7), (65537, 256, 5, 1.0)]
# one case per route for the tests that need a route, not a boundary: route -> (case, entry)
ROUTE_CASE = {"f8": ((4096, 50, 5, 1.0), "plain"), "f16": ((16384, 256, 5, 1.3), "plain"), "f36": ((16385, 50, 5, 0.7), "plain"),
              "f64": ((36865, 50, 5, 1.0), "plain"), "general": ((65537, 50, 5, 0.7), "plain"), "groups": ((36864, 50, 5, 1.0), "groups")}
# ---- B2: (route, V, top_k, hot threads / groups): rows whose cheap bound is loose while the true threshold is sharp
HOT_OVER = [("f8", 4096, 256, 255), ("f16", 16384, 256, 255), ("f36", 36864, 50, 49), ("f64", 65536, 50, 49), ("groups", 16384, 50, 40)]
HOT_MID = [("f8", 4096, 128, 80), ("f16", 16384, 50, 40), ("f36", 36864, 50, 18), ("f64", 65536, 50, 10), ("groups", 16384, 50, 10)]
# ---- B3 / B5: route -> (V, entry)
ROUTE_V = {"f8": (4096, "plain"), "f16": (16384, "plain"), "f36": (36864, "plain"), "f64": (65536, "plain"), "general": (65537, "plain"),
           "exact": (16384, "exact"), "groups": (16384, "groups")}


def entries(v, top_k):
    return ("plain", "exact") + (("groups",) if R.groups_allowed(v, top_k) else ())


def route_of(v, top_k, entry):
    return R.route(v, top_k, exact=entry == "exact", groups=entry == "groups")


# ---- inputs (CPU only) ------------------------------------------------------------------------------------------------------------
def _admit(make, check):
    """The first of 64 seeds whose row passes ``check`` (-> margin): a row is redrawn, never skipped."""
    for attempt in range(64):
        row = make(attempt)
        if check(*row) >= R.MARGIN:
            return row
    raise AssertionError("no seed of 64 gives this row a margin")


def _stack(rows):
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def _margin(x, nz, temp, beam, top_k, top_ps=()):
    return min(min(R.row_draw(x[None], nz[None], temp, beam, top_k, UNK, tp)[3]) for tp in (None,) + tuple(top_ps))


@functools.lru_cache(maxsize=None)
def case_inputs(v, top_k, beam, temp):
    """``(logits [ROWS, V], noise [ROWS, V], {None | top_p: row_draw's result})``: random rows; row 0 with <unk> as its arg-max, row 2
    with ``top_k + 3`` equal logits straddling the threshold (and one above them).  Every row has its margin for the plain draw and for each top_p."""
    def make(r):
        def one(attempt):
            g = torch.Generator().manual_seed(1000003 * v + 7919 * top_k + 131 * beam + 17 * r + 100003 * attempt)
            x = torch.randn(v, generator=g) * 2.5
            if r == 0 and top_k > 2:
                x[UNK] = 50.0
            if r == 2 and top_k > 2 and v >= top_k + 16:
                x[10:10 + top_k + 3] = 30.0
                x[5] = 31.0 + 0.125 * attempt               # (one above them: no prefix of equal p is a round number like top_p)
            return x, torch.empty(v).exponential_(1, generator=g)
        return one
    logits, noise = _stack([_admit(make(r), lambda x, nz: _margin(x, nz, temp, beam, top_k, TOP_PS)) for r in range(ROWS)])
    return logits, noise, {tp: R.row_draw(logits, noise, temp, beam, top_k, UNK, tp) for tp in (None,) + TOP_PS}


@functools.lru_cache(maxsize=None)
def hot_inputs(rt, v, top_k, hot, beam=5, temp=1.0):
    """Rows whose ``hot`` threads (columns ``i % NT < hot``) or whole 64-column groups (5 .. 5 + hot) hold only large, distinct values."""
    cols = torch.arange(v)
    mask = (cols // 64 >= 5) & (cols // 64 < 5 + hot) if rt == "groups" else cols % R.FAST[rt][1] < hot

    def make(r):
        def one(attempt):
            g = torch.Generator().manual_seed(2000003 * v + 7919 * top_k + 131 * hot + 17 * r + 100003 * attempt)
            x = torch.randn(v, generator=g) * 2.5
            big = 30.0 + torch.randn(v, generator=g) * 2.5
            x[mask] = big[mask]
            return x, torch.empty(v).exponential_(1, generator=g)
        return one

    def check(x, nz):
        return _margin(x, nz, temp, beam, top_k) if len(torch.unique(x[mask])) == int(mask.sum()) else 0.0
    logits, noise = _stack([_admit(make(r), check) for r in range(ROWS)])
    return logits, noise, R.row_draw(logits, noise, temp, beam, top_k, UNK)


@functools.lru_cache(maxsize=None)
def tied_inputs(v, n_tied, top_k=50, beam=5, temp=1.0):
    """Rows with ``n_tied`` logits tied at the top (9.0 over values clamped to +-7.5) and <unk> far below."""
    def make(r):
        def one(attempt):
            g = torch.Generator().manual_seed(3000003 * v + 7919 * n_tied + 17 * r + 100003 * attempt)
            x = torch.randn(v, generator=g).clamp(-3, 3) * 2.5
            at = torch.randperm(v - 2, generator=g)[:n_tied] + 2
            x[at] = 9.0
            x[UNK] = -40.0
            return x, torch.empty(v).exponential_(1, generator=g)
        return one
    logits, noise = _stack([_admit(make(r), lambda x, nz: _margin(x, nz, temp, beam, top_k)) for r in range(ROWS)])
    return logits, noise, R.row_draw(logits, noise, temp, beam, top_k, UNK)


@functools.lru_cache(maxsize=None)
def sparse_inputs(v, n_finite, top_k, beam, temp=1.0):
    """Rows with ``n_finite`` finite logits (never <unk>), the rest -inf: what min_len / bad_words_ids leave of a small vocabulary."""
    def make(r):
        def one(attempt):
            g = torch.Generator().manual_seed(4000003 * v + 7919 * n_finite + 17 * r + 100003 * attempt)
            x = torch.full((v,), NINF)
            at = torch.randperm(v - 2, generator=g)[:n_finite] + 2
            x[at] = torch.randn(n_finite, generator=g) * 2.5
            return x, torch.empty(v).exponential_(1, generator=g)
        return one
    logits, noise = _stack([_admit(make(r), lambda x, nz: _margin(x, nz, temp, beam, top_k)) for r in range(ROWS)])
    return logits, noise, R.row_draw(logits, noise, temp, beam, top_k, UNK)


def f32_bits(bits):
    return torch.tensor([bits - (1 << 32) if bits >= 1 << 31 else bits], dtype=torch.int32).view(torch.float32)[0]


BAD = {"+inf": float("inf"), "+nan": f32_bits(0x7FC00000), "-nan": f32_bits(0xFFC00000)}


@functools.lru_cache(maxsize=None)
def nonfinite_inputs(rt, bad):
    """The route's case with one value of row 1 -- the neighbour of its arg-max, in the same 64-column group -- replaced."""
    (v, top_k, beam, temp), entry = ROUTE_CASE[rt] if rt in ROUTE_CASE else ((16384, 50, 5, 1.0), "exact")
    logits, noise, _ = case_inputs(v, top_k, beam, temp)
    logits = logits.clone()
    at = int(logits[1].argmax()) ^ 1
    assert at != UNK
    logits[1, at] = BAD[bad]
    return logits, noise, R.row_draw(logits, noise, temp, beam, top_k, UNK), (v, top_k, beam, temp), entry


def tile(t, rows):
    return t[torch.arange(rows) % t.shape[0]]


def prompted_rows(beam, step):
    """The rows a prompted launch draws at ``step``: an image past its prompt all of them, an image at its first position row 0."""
    rows = []
    for img, fp in enumerate(FIRST_POS):
        rows += list(range(img * beam, (img + 1) * beam)) if step > fp else [img * beam] if step == fp else []
    return rows


@functools.lru_cache(maxsize=None)
def philox_inputs(v, top_k, beam, temp, top_p, prompted_step, seed0, img0, step, rpi):
    """The case's logits under restated Philox noise: the first seed (of 64 from ``seed0``) at which every drawn row has its margin."""
    logits = case_inputs(v, top_k, beam, temp)[0]
    rows, drawn = ROWS, list(range(ROWS))
    if prompted_step is not None:
        rows, rpi, step, drawn = len(FIRST_POS) * beam, beam, prompted_step, prompted_rows(beam, prompted_step)
        logits = tile(logits, rows)
    for seed in range(seed0, seed0 + 64):
        noise = R.row_noise(seed, img0, step, rows, rpi, v)
        want = R.row_draw(logits, noise, temp, beam, top_k, UNK, top_p)
        if min(want[3][r] for r in drawn) >= R.MARGIN:
            return seed, logits, want, drawn, rpi, step
    raise AssertionError("no seed of 64 gives these rows a margin")


@functools.lru_cache(maxsize=None)
def flat_inputs(seed, seed_ptr, img0, step, rpi):
    """B6: the expected picks of flat rows (V = 65, beam = top_k = 64, <unk> = 1) -- the survivors in ascending order of the restated
    noise -- and the smallest relative gap between consecutive sorted noise values."""
    nz = R.row_noise(seed ^ seed_ptr, img0, step, ROWS, rpi, 65)
    nz[:, UNK] = np.inf
    order = np.argsort(nz, axis=1, kind="stable")[:, :64]
    s = np.sort(nz, axis=1)[:, :64]
    return order, float(((s[:, 1:] - s[:, :-1]) / s[:, 1:]).min())


FLAT_VARIANTS = {"base": (11, 0, 5, 2, 3), "seed_lo": (12, 0, 5, 2, 3), "seed_hi": (11 + (7 << 32), 0, 5, 2, 3),
                 "seed_ptr": (11, 0x5A5A00000123, 5, 2, 3), "img0": (11, 0, 6, 2, 3), "step": (11, 0, 5, 3, 3), "rows_per_img": (11, 0, 5, 2, 2)}


def flat_variant(name):
    """(seed, seed_ptr, img0, step, rows_per_img) of a variant, its seed advanced until the noise gaps are >= 1e-5."""
    seed, sp, img0, step, rpi = FLAT_VARIANTS[name]
    for k in range(64):
        if flat_inputs(seed + 1000 * k, sp, img0, step, rpi)[1] >= 1e-5:
            return seed + 1000 * k, sp, img0, step, rpi
    raise AssertionError(name)


def select_state(n_img, beam, tok_ld, with_src, seed):
    """``test_beam_search_gpu.random_state``'s kind of state: ended beams, dead (-inf) beams, a finished image (2), an image whose
    beams have all ended (1: it finishes in this step), <eos> and -inf among the picks -- and one live candidate per image."""
    g = torch.Generator().manual_seed(seed)
    r = n_img * beam
    st = State(n_img, beam, tok_ld, src_len=tok_ld + 1 if with_src else 0)
    st.tokens = torch.randint(4, 50, (r, tok_ld), generator=g, dtype=torch.int32)
    st.vals = torch.randint(-12, 0, (r,), generator=g).float() * 0.25
    st.ended = (torch.rand(r, generator=g) < 0.3).to(torch.uint8)
    st.vals[torch.rand(r, generator=g) < 0.15] = NINF
    if with_src:
        st.src = (torch.randint(0, beam, (r, tok_ld + 1), generator=g, dtype=torch.int32)
                  + (torch.arange(r, dtype=torch.int32) // beam * beam)[:, None])
    st.parent = torch.full((r,), -5, dtype=torch.int32)
    st.hparent = torch.full((r,), -5, dtype=torch.int32)
    if n_img > 2:
        st.done[2], st.end_step[2] = 1, 1
    if n_img > 1:
        st.ended[beam:2 * beam] = 1
    pick_idx = torch.randint(0, 50, (r, beam), generator=g, dtype=torch.int32)
    pick_idx[torch.rand(r, beam, generator=g) < 0.2] = EOS
    pick_val = torch.sort(torch.randint(-8, 0, (r, beam), generator=g).float() * 0.25, dim=1, descending=True).values
    pick_val[torch.rand(r, beam, generator=g) < 0.1] = NINF
    st.vals[::beam] = -0.75                              # (an image whose candidates are all -inf has no softmax)
    pick_val[::beam, 0] = -0.25
    return st, pick_idx, pick_val


# (first, write_pos, first_pos): dense first / later steps, the step that writes no token, the prompted phases
SELECT_STEPS = [(True, 0, None), (False, 3, None), (False, 6, None), (False, 3, (5, 3, 1)), (False, 3, (3, 0, 4))]
SEL_T, SEL_TOK_LD, SEL_STEP, SEL_TEMP = 3, 6, 3, 0.7


@functools.lru_cache(maxsize=None)
def select_inputs(beam, with_src, case, philox):
    """``(state before, pick_idx, pick_val, noise fp32 or None, seed, want state, margins)``: the first state seed (of 64) whose
    candidate races all have their margin."""
    first, write_pos, first_pos = SELECT_STEPS[case]
    for attempt in range(64):
        sd = 29 * beam + 7 * case + 3 * int(with_src) + int(philox) + 1009 * attempt
        st, pick_idx, pick_val = select_state(3, beam, SEL_TOK_LD, with_src, sd)
        if first:
            st.vals.zero_()
            st.ended.zero_()
            st.done.zero_()
        if philox:
            noise32, nz = None, R.select_noise(sd, 4, SEL_STEP, 3, beam)
        else:
            noise32 = torch.empty(3, beam * beam).exponential_(1, generator=torch.Generator().manual_seed(sd + 1))
            nz = noise32.double().numpy()
        want = State.of(st.tokens, st.vals, st.ended, st.done, st.end_step, beam, st.src, st.parent, st.hparent)
        margins = R.select_sampled(want, pick_idx, pick_val, nz, SEL_TEMP, first, write_pos, SEL_T, SEL_STEP, EOS, first_pos=first_pos)
        if min(margins) >= R.MARGIN:
            return st, pick_idx, pick_val, noise32, sd, want, margins
    raise AssertionError("no seed of 64 gives this select a margin")


@functools.lru_cache(maxsize=None)
def final_inputs(beam, philox):
    n_img = 4
    for attempt in range(64):
        sd = 31 * beam + int(philox) + 1009 * attempt
        g = torch.Generator().manual_seed(sd)
        vals = torch.randint(-12, 0, (n_img, beam), generator=g).float() * 0.25
        vals[torch.rand(n_img, beam, generator=g) < 0.2] = NINF
        vals[:, beam // 2] = -1.0
        noise32 = None if philox else torch.empty(n_img, beam).exponential_(1, generator=g)
        nz = R.final_noise(sd, 4, n_img, beam) if philox else noise32.double().numpy()
        drawn, margins = R.final_draw(vals, nz, SEL_TEMP)
        if min(margins) >= R.MARGIN:
            return vals, noise32, sd, drawn, margins
    raise AssertionError("no seed of 64 gives this draw a margin")


# ---- the device side ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    return h


def ldl_of(v):
    return (v + 255) // 256 * 256 + 8


class Dev:
    """A case's padded device buffers: logits ``[rows, ldl]`` (pads set by ``pad``), noise of the same stride with 0.0 in its pads,
    group maxima over the REAL columns (fmax: a NaN is no maximum)."""

    def __init__(self, logits, noise=None, rows=None):
        self.v = logits.shape[1]
        idx = None if rows is None else (torch.arange(rows) % logits.shape[0]).cuda()
        x = logits.cuda() if idx is None else logits.cuda()[idx]
        self.rows, ldl = x.shape[0], ldl_of(self.v)
        self.x = torch.empty(self.rows, ldl, device="cuda")
        self.x[:, :self.v] = x
        self.nz = None
        if noise is not None:
            nz = torch.as_tensor(noise).float().cuda()
            self.nz = torch.zeros(self.rows, ldl, device="cuda")
            self.nz[:, :self.v] = nz if idx is None else nz[idx]
        ng = R.n_groups(self.v)
        full = torch.full((self.rows, ng * 64), NINF, device="cuda")
        full[:, :self.v] = torch.nan_to_num(x, nan=NINF, posinf=float("inf"), neginf=NINF)
        self.gm = full.view(self.rows, ng, 64).max(-1).values.contiguous()
        self.pad(PADS[0])

    def pad(self, value):
        self.x[:, self.v:] = value
        return self


def run(h, d, entry, beam, top_k, temp, top_p=None, first_pos=None, step=0, noise=True, seed=0, img0=0, rpi=3, seed_ptr=None):
    """One launch over the case's rows into sentinel-filled pick tables two rows longer: ``(picks int64, values, err)``."""
    rows, v = d.rows, d.v
    pi = torch.full((rows + 2, beam), SENT_I, dtype=torch.int32, device="cuda")
    pv = torch.full((rows + 2, beam), SENT_V, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nz = d.nz if noise else None
    gm = d.gm if entry == "groups" else None
    fp = None if first_pos is None else torch.tensor(first_pos, dtype=torch.int32, device="cuda")
    sp = None if seed_ptr is None else torch.tensor([seed_ptr], dtype=torch.int64, device="cuda")
    x = d.x                                            # (the wrappers take the row stride from the tensor)
    if top_p is not None:
        h.beam_row_sample_nucleus(x, v, rows, beam if fp is not None else rpi, beam, top_k, top_p, temp, UNK, nz, seed, img0, step, pi, pv, err,
                                  seed_ptr=sp, exact=entry == "exact", group_max=gm, first_pos=fp)
    elif fp is not None:
        h.beam_row_sample_prompted(x, v, rows, beam, top_k, temp, UNK, nz, seed, img0, step, fp, pi, pv, err, seed_ptr=sp,
                                   exact=entry == "exact", group_max=gm)
    elif entry == "groups":
        h.beam_row_sample_groups(x, v, gm, rows, rpi, beam, top_k, temp, UNK, nz, seed, img0, step, pi, pv, err, seed_ptr=sp)
    else:
        h.beam_row_sample(x, v, rows, rpi, beam, top_k, temp, UNK, nz, seed, img0, step, pi, pv, err, seed_ptr=sp, exact=entry == "exact")
    torch.cuda.synchronize()
    pi, pv = pi.cpu(), pv.cpu()
    assert bool((pi[rows:] == SENT_I).all()) and bool((pv[rows:] == SENT_V).all()), "rows past the launch were written"
    return pi[:rows].long(), pv[:rows], int(err.item())


def same(got, want, rt, rows=None, what=""):
    """Picks equal (the live ones; a dead slot holds -inf), values inside the bound, for ``rows`` (all by default); every other row of
    the launch still holds the sentinel.  Returns the worst value error, which also goes to WORST[route]."""
    pi, pv, _ = got
    picks, vals, _, _ = want
    n = pi.shape[0]
    rows = list(range(n)) if rows is None else rows
    worst = 0.0
    for r in range(n):
        tag = (what, rt, "row", r)
        if r not in rows:
            assert bool((pi[r] == SENT_I).all()) and bool((pv[r] == SENT_V).all()), tag + ("an idle row was written",)
            continue
        live = picks[r % picks.shape[0]] >= 0
        w_i, w_v = picks[r % picks.shape[0]], vals[r % picks.shape[0]]
        assert pi[r][live].tolist() == w_i[live].tolist(), tag + (pi[r].tolist(), w_i.tolist())
        assert bool((pv[r][~live] == NINF).all()), tag
        e = (pv[r][live].double() - w_v[live]).abs()
        assert bool((e <= 2e-6 + 2.0 ** -23 * w_v[live].abs()).all()), tag + (float(e.max()),)
        worst = max(worst, float(e.max()) if e.numel() else 0.0)
    WORST[rt] = max(WORST[rt], worst)
    return worst


def flags_of(want, rows=None):
    out = 0
    for r, f in enumerate(want[2]):
        out |= f if rows is None or r in rows else 0
    return out


# ---- B1: the route matrix, supplied noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,top_k,beam,temp", CASES, ids=lambda x: str(x))
def test_route_matrix_supplied_noise(hip, v, top_k, beam, temp):
    """Plain, exact and groups entry points; the plain draw, the nucleus entry at three top_p and the prompted entry at three steps;
    both pad flavours: picks equal, values inside the bound, err == 0, idle rows and rows past the launch untouched."""
    logits, noise, want = case_inputs(v, top_k, beam, temp)
    assert all(f == 0 for w in want.values() for f in w[2]) and min(min(w[3]) for w in want.values()) >= R.MARGIN
    d = Dev(logits, noise)
    dp = Dev(logits, noise, rows=len(FIRST_POS) * beam)
    for pad in PADS:
        d.pad(pad), dp.pad(pad)
        for entry in entries(v, top_k):
            rt = route_of(v, top_k, entry)
            got = run(hip, d, entry, beam, top_k, temp)
            assert got[2] == 0, (entry, got[2])
            worst = same(got, want[None], rt, what=entry)
            for tp in TOP_PS:
                got = run(hip, d, entry, beam, top_k, temp, top_p=tp)
                assert got[2] == 0, (entry, tp, got[2])
                worst = max(worst, same(got, want[tp], rt, what=(entry, tp)))
            for step in STEPS:
                got = run(hip, dp, entry, beam, top_k, temp, first_pos=FIRST_POS, step=step)
                assert got[2] == 0, (entry, step, got[2])
                worst = max(worst, same(got, want[None], rt, rows=prompted_rows(beam, step), what=(entry, "prompted", step)))
            got = run(hip, dp, entry, beam, top_k, temp, top_p=0.8, first_pos=FIRST_POS, step=2)
            assert got[2] == 0, (entry, "nucleus prompted", got[2])
            worst = max(worst, same(got, want[0.8], rt, rows=prompted_rows(beam, 2), what=(entry, "nucleus prompted")))
            print(f"V {v} top_k {top_k} beam {beam} T {temp} pad {pad} {entry} -> {rt}: worst value error {worst:.3e}")


# ---- B2: where the large values stand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt,v,top_k,hot", HOT_OVER + HOT_MID, ids=lambda x: str(x))
def test_loose_bound_sharp_threshold(hip, rt, v, top_k, hot):
    """HOT_OVER: more than 1,024 candidates pass the cheap bound while exactly top_k survive -- the in-kernel exact re-derivation
    (radix_row_candidates) must give the reference's picks with no flag.  HOT_MID: ~650 candidates, the rank search of row_tail."""
    logits, noise, want = hot_inputs(rt, v, top_k, hot)
    entry = "groups" if rt == "groups" else "plain"
    assert route_of(v, top_k, entry) == rt and flags_of(want) == 0
    d = Dev(logits, noise)
    for pad in PADS:
        got = run(hip, d.pad(pad), entry, 5, top_k, 1.0)
        assert got[2] == 0, got[2]
        print(f"{rt} V {v} top_k {top_k} hot {hot} pad {pad}: worst value error {same(got, want, rt):.3e}")


# ---- B3: ties and the 1,024-survivor limit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", list(ROUTE_V))
def test_ties_at_the_survivor_limit(hip, rt):
    """1,024 logits tied at the threshold: every route draws, no flag.  1,025: the single-pass and groups kernels flag OVERFLOW, the
    general kernel draws over the row (the reference's picks, no flag); the nucleus entry flags OVERFLOW on every route."""
    v, entry = ROUTE_V[rt]
    kernel = route_of(v, 50, entry)
    assert kernel == ("general" if rt == "exact" else rt)
    logits, noise, want = tied_inputs(v, 1024)
    got = run(hip, Dev(logits, noise).pad(PADS[1]), entry, 5, 50, 1.0)
    assert got[2] == 0 and flags_of(want) == 0, got[2]
    same(got, want, kernel, what="1024 tied")
    logits, noise, want = tied_inputs(v, 1025)
    d = Dev(logits, noise).pad(PADS[1])
    got = run(hip, d, entry, 5, 50, 1.0)
    if kernel == "general":
        assert got[2] == 0 and flags_of(want) == 0, got[2]
        same(got, want, kernel, what="1025 tied")
    else:
        assert got[2] & R.ERR_OVERFLOW, got[2]
    assert run(hip, d, entry, 5, 50, 1.0, top_p=0.8)[2] & R.ERR_OVERFLOW


# ---- B4: sparse rows --------------------------------------------------------------------------------------------------------------
def test_sparse_rows_small_vocabulary(hip):
    """V = 71 with 10 finite logits, top_k 50: the threshold is -inf; every route draws among the finite ones, no flag."""
    logits, noise, want = sparse_inputs(71, 10, 50, 5)
    assert flags_of(want) == 0
    d = Dev(logits, noise).pad(PADS[1])
    for entry in ("plain", "exact"):
        got = run(hip, d, entry, 5, 50, 1.0)
        assert got[2] == 0, (entry, got[2])
        same(got, want, route_of(71, 50, entry), what=entry)


def test_sparse_rows_overflow_to_exact(hip):
    """V = 5,000 with 10 finite logits: 4,989 survivors tie at -inf -- OVERFLOW on the single-pass and groups routes, the reference's
    picks from the general kernel."""
    logits, noise, want = sparse_inputs(5000, 10, 50, 5)
    assert flags_of(want) == 0
    d = Dev(logits, noise).pad(PADS[0])
    assert run(hip, d, "plain", 5, 50, 1.0)[2] & R.ERR_OVERFLOW
    assert run(hip, d, "groups", 5, 50, 1.0)[2] & R.ERR_OVERFLOW
    got = run(hip, d, "exact", 5, 50, 1.0)
    assert got[2] == 0, got[2]
    same(got, want, "general", what="exact")


@pytest.mark.parametrize("entry", ("plain", "exact"))
def test_fewer_finite_logits_than_beams(hip, entry):
    """Three finite logits, five beams: TOO_FEW, the live picks are the reference's, the dead picks have value -inf.  Also the classic
    form: top_k == beam with <unk> inside the top-k."""
    logits, noise, want = sparse_inputs(71, 3, 50, 5)
    assert flags_of(want) == R.ERR_TOO_FEW and bool((want[0][:, 3:] == -1).all()) and bool((want[0][:, :3] >= 0).all())
    got = run(hip, Dev(logits, noise).pad(PADS[1]), entry, 5, 50, 1.0)
    same(got, want, route_of(71, 50, entry), what="3 finite")
    assert got[2] == R.ERR_TOO_FEW, got[2]
    logits, noise, _ = case_inputs(4096, 50, 5, 1.0)
    want = R.row_draw(logits, noise, 1.0, 5, 5, UNK)              # row 0: <unk> is the arg-max, 4 survivors for 5 beams
    assert want[2] == [R.ERR_TOO_FEW, 0, 0, 0, 0, 0] and min(want[3]) >= R.MARGIN
    got = run(hip, Dev(logits, noise), entry, 5, 5, 1.0)
    same(got, want, route_of(4096, 5, entry), what="unk in the top-k")
    assert got[2] == R.ERR_TOO_FEW and got[0][0, 4] == 0, got[2]


@pytest.mark.parametrize("entry", ("plain", "exact", "groups"))
def test_only_unk_in_the_top_1(hip, entry):
    logits, noise, _ = case_inputs(4096, 50, 5, 1.0)
    want = R.row_draw(logits, noise, 1.0, 1, 1, UNK)
    assert want[2] == [R.ERR_ALL_FILTERED, 0, 0, 0, 0, 0] and min(want[3]) >= R.MARGIN
    got = run(hip, Dev(logits, noise), entry, 1, 1, 1.0)
    assert got[2] == R.ERR_ALL_FILTERED, got[2]
    same(got, want, route_of(4096, 1, entry))


# ---- B5: non-finite rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("rt", list(ROUTE_CASE) + ["exact"])
def test_nonfinite_rows(hip, rt, bad):
    """+inf, a NaN with a clear sign bit and a NaN with its sign bit SET in row 1: NONFINITE on every route (the reference's
    torch.multinomial raises: torch.topk ranks a NaN of either sign above everything), row 1 hands on the finite dummy (0, 0.0),
    the other rows are drawn as ever."""
    logits, noise, want, (v, top_k, beam, temp), entry = nonfinite_inputs(rt, bad)
    assert want[2] == [0, R.ERR_NONFINITE, 0, 0, 0, 0] and want[0][1].tolist() == [0] * beam and want[1][1].tolist() == [0.0] * beam
    d = Dev(logits, noise)
    for pad in PADS:
        got = run(hip, d.pad(pad), entry, beam, top_k, temp)
        assert got[2] == R.ERR_NONFINITE, (pad, got[2])
        same(got, want, route_of(v, top_k, entry), what=bad)
    got = run(hip, d, entry, beam, top_k, temp, top_p=0.8)
    assert got[2] == R.ERR_NONFINITE and got[0][1].tolist() == [0] * beam and got[1][1].tolist() == [0.0] * beam, got[2]


# ---- B6: the Philox counters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FLAT_VARIANTS))
def test_philox_counters_on_flat_rows(hip, name):
    """64 equal-probability survivors: the picks are the tokens in ascending order of their noise, so the restated philox_exp1 must
    reproduce all 64 in order -- for the base arguments and with one of them changed at a time (which must change the picks)."""
    seed, sp, img0, step, rpi = flat_variant(name)
    order, gap = flat_inputs(seed, sp, img0, step, rpi)
    assert gap >= 1e-5
    d = Dev(torch.full((ROWS, 65), 0.5)).pad(PADS[1])
    pi, pv, err = run(hip, d, "plain", 64, 64, 1.0, noise=False, seed=seed, img0=img0, step=step, rpi=rpi, seed_ptr=sp if sp else None)
    assert err == 0 and pi.tolist() == order.tolist()
    assert float((pv.double() + np.log(64.0)).abs().max()) <= 2e-6 + 2.0 ** -23 * np.log(64.0)
    if name != "base":
        base = flat_inputs(*flat_variant("base"))[0]
        assert (order != base).any(axis=1).sum() >= (3 if name == "rows_per_img" else ROWS)     # rows 0, 1 share (image, row) at 2 and 3


@pytest.mark.parametrize("rt", list(ROUTE_CASE))
def test_philox_draw_is_the_restated_noise(hip, rt):
    """noise=None: the kernel equals row_draw fed the restated Philox table -- the plain, nucleus and prompted forms of one case per
    route."""
    (v, top_k, beam, temp), entry = ROUTE_CASE[rt]
    assert route_of(v, top_k, entry) == rt
    logits = case_inputs(v, top_k, beam, temp)[0]
    d, dp = Dev(logits).pad(PADS[1]), Dev(logits, rows=len(FIRST_POS) * beam).pad(PADS[1])
    sp = 0x1234500000077
    for top_p, pstep in ((None, None), (0.8, None), (None, 0), (None, 2), (None, 3), (0.8, 2)):
        seed, _, want, drawn, rpi, step = philox_inputs(v, top_k, beam, temp, top_p, pstep, 900, 3, 4, 3)
        got = run(hip, d if pstep is None else dp, entry, beam, top_k, temp, top_p=top_p, first_pos=None if pstep is None else FIRST_POS,
                  step=step, noise=False, seed=seed ^ sp, seed_ptr=sp, img0=3, rpi=rpi)
        assert got[2] == 0, (top_p, pstep, got[2])
        same(got, want, rt, rows=drawn, what=("philox", top_p, pstep))


# ---- B7: the sampled select and the final draw ------------------------------------------------------------------------------------
def run_select(h, st, pick_idx, pick_val, noise32, seed, first, write_pos, first_pos):
    dev = {k: None if v is None else v.clone().cuda() for k, v in st.fields().items()}
    nz = None if noise32 is None else noise32.cuda()
    sp = torch.tensor([0x77000000005], dtype=torch.int64, device="cuda")
    args = (pick_idx.cuda(), pick_val.cuda(), dev["tokens"], dev["vals"], dev["ended"], dev["src"], dev["parent"], dev["hparent"],
            dev["done"], dev["end_step"], st.n_img, st.beam)
    if first_pos is None:
        h.beam_select(*args, first, True, write_pos, SEL_T, SEL_STEP, SEL_TEMP, EOS, nz, seed ^ 0x77000000005, 4, seed_ptr=sp)
    else:
        h.beam_select_prompted(*args, torch.tensor(first_pos, dtype=torch.int32, device="cuda"), True, write_pos, SEL_T, SEL_STEP,
                               SEL_TEMP, EOS, nz, seed ^ 0x77000000005, 4, seed_ptr=sp)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu() for k, v in dev.items()}


@pytest.mark.parametrize("philox", (False, True), ids=("noise", "philox"))
@pytest.mark.parametrize("with_src", (False, True), ids=("lstm", "src"))
@pytest.mark.parametrize("beam", (1, 3, 5, 17, 64))
def test_sampled_select_is_the_restatement_bit_for_bit(hip, beam, with_src, philox):
    """Every state field equals select_sampled's (vals bitwise): dense first / later steps, the step that writes no token and the
    prompted phases; ended and dead beams, a finished image, an image finishing in this step; both select instantiations (MB 16 / 64)."""
    for case, (first, write_pos, first_pos) in enumerate(SELECT_STEPS):
        st, pick_idx, pick_val, noise32, seed, want, margins = select_inputs(beam, with_src, case, philox)
        assert min(margins) >= R.MARGIN
        got = run_select(hip, st, pick_idx, pick_val, noise32, seed, first, write_pos, first_pos)
        for k, w in want.fields().items():
            if w is None:
                continue
            if k == "vals":
                assert torch.equal(got[k].view(torch.int32), w.view(torch.int32)), (case, k, got[k].tolist(), w.tolist())
            else:
                assert torch.equal(got[k], w), (case, k, got[k].tolist(), w.tolist())


@pytest.mark.parametrize("philox", (False, True), ids=("noise", "philox"))
@pytest.mark.parametrize("beam", (1, 5, 64))
def test_final_draw(hip, beam, philox):
    """dh_beam_finalize_beams' out_drawn names (through out_index) the beam final_draw picks."""
    vals, noise32, seed, drawn, margins = final_inputs(beam, philox)
    n_img, t = vals.shape[0], 6
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    tokens = torch.randint(4, 50, (n_img * beam, t), generator=torch.Generator().manual_seed(beam), dtype=torch.int32).cuda()
    out_tokens, out_len, out_score = i32(n_img, beam, t), i32(n_img, beam), torch.zeros(n_img, beam, device="cuda")
    out_index, out_drawn, out_row_len = i32(n_img, beam), i32(n_img), i32(n_img)
    sp = torch.tensor([0x3300000009], dtype=torch.int64, device="cuda")
    hip.beam_finalize_beams(tokens, vals.reshape(-1).cuda(), torch.zeros(n_img, dtype=torch.uint8, device="cuda"), i32(n_img), out_tokens,
                            out_len, out_score, out_index, out_drawn, out_row_len, n_img, beam, 1, t, 0, EOS, 0, None, SEL_TEMP,
                            None if noise32 is None else noise32.cuda(), seed ^ 0x3300000009, 4, seed_ptr=sp)
    torch.cuda.synchronize()
    got = out_index.cpu().gather(1, out_drawn.cpu().long()[:, None])[:, 0].tolist()
    assert got == drawn, (got, drawn, margins)


def test_zz_report():
    """(runs last in the module) the module's wall time and the worst value error per route."""
    print(f"row-draw routes: {time.time() - T0:.1f} s wall; worst |value error| per route: "
          + ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST.items())))
