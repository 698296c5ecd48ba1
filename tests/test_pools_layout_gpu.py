"""The pooling, layout and preprocessing kernels between the encoder's GEMMs -- the pools and layout kernels of conv.hip,
dh_normalize_pack_u8 and dh_round16_keep_nonzero of preproc.hip, the three fp32 channels-last helpers of gemm_f32x.hip --
against the references of rowops_ref.py, exact but for avgpool_rows:

  max pools          F.max_pool2d(x, 3, 2, 1) on all-negative inputs (a padding cell read as 0 would win), non-square H x W
  avgpool_nhwc(_f32) both kernels sum the positions in index order: the sequential fp32 sum, one division, one rounding, bit for bit
  avgpool_rows       a wave tree: fp64, gated at YARD_MULT = 4 x the CPU fp32 mean's error (ROWS_YARD, recomputed by
                     tests/test_rowops_ref_cpu.py)
  layouts            permute / zero-padded channels / the one-rounding cast
  normalisations     ((x / 255) - mean) / std in fp32, all 256 byte values; the fused pack equals pack(normalize(x))
  wrap cases         one shape per capped launcher, less than 10 % past its cap: the second trip of the grid-stride loop.
                     Left out: nchw_to_nhwc_f32 and maxpool3x3s2_nhwc_f32, whose 16,777,216-thread caps need 0.3 - 1 GB operands.

Every test prints what it covered; the wrappers here own their outputs, so there is no sentinel buffer to check."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_ref as R  # noqa: E402
from rowops_ref import DT16, DT16_IDS, F32, NAME  # noqa: E402
from test_rowops_routes_gpu import Worst, right_or_refused  # noqa: E402

# max(worst CPU fp32 x.mean() error against fp64, half an fp32 ulp of the result) over the rows of each HW
ROWS_YARD = {1: 1.192e-07, 49: 7.785e-08, 63: 5.156e-08, 64: 4.284e-08, 65: 6.052e-08, 200: 6.571e-08}


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print(f"[test_pools_layout_gpu] module wall time {time.time() - t0:.1f} s")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


# ---- max pools ------------------------------------------------------------------------------------------------------------------
def test_maxpool_nchw_is_exact(hip):
    n_cases = 0
    for h, w in R.POOL_HW:
        for c in R.POOL_C:
            for n in R.POOL_N:
                x = R.negative(n, c, h, w, seed=h * 16 + w + c + n)
                assert torch.equal(hip.maxpool3x3s2(x.cuda()).cpu(), R.maxpool_ref(x)), (n, c, h, w)
                n_cases += 1
    print(f"[maxpool3x3s2] f32: {n_cases} cases exact")


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_maxpool_nhwc_is_exact(hip, dt):
    n_cases = 0
    for h, w in R.POOL_HW:
        for c in R.POOL_C:
            for n in R.POOL_N:
                x = R.negative(n, c, h, w, seed=h * 16 + w + c + n).to(dt)
                got = hip.maxpool3x3s2_nhwc(nhwc(x).cuda())
                assert got.dtype == dt and torch.equal(nchw(got.cpu()).float(), R.maxpool_ref(x.float())), (NAME[dt], n, c, h, w)
                n_cases += 1
    print(f"[maxpool3x3s2_nhwc] {NAME[dt]}: {n_cases} cases exact")


def test_maxpool_nhwc_f32_is_exact(hip):
    n_cases = 0
    for h, w in R.POOL_HW:
        for c in R.POOL_C_F32:
            for n in R.POOL_N:
                x = R.negative(n, c, h, w, seed=h * 16 + w + c + n)
                assert torch.equal(nchw(hip.maxpool3x3s2_nhwc_f32(nhwc(x).cuda()).cpu()), R.maxpool_ref(x)), (n, c, h, w)
                n_cases += 1
    print(f"[maxpool3x3s2_nhwc_f32] f32: {n_cases} cases exact")


# ---- average pools --------------------------------------------------------------------------------------------------------------
def avg_cases(dt, channels):
    for hw in R.AVG_HW:
        for c in channels:
            for n in R.POOL_N:
                h = 7 if hw == 49 else 1
                yield (R.randn(n, h, hw // h, c, seed=hw + c + n) + 0.25).to(dt)


@pytest.mark.parametrize("dt", DT16, ids=DT16_IDS)
def test_avgpool_nhwc_is_bit_exact(hip, dt):
    """"Same summation order as the plain loop": HW below, at and above the eight-position round."""
    n_cases = 0
    for x in avg_cases(dt, R.AVG_C):
        n, h, w, c = x.shape
        got = hip.avgpool_nhwc(x.cuda())
        assert got.dtype == dt and torch.equal(got.cpu(), R.avgpool_seq_ref(x.view(n, h * w, c))), (NAME[dt], tuple(x.shape))
        n_cases += 1
    print(f"[avgpool_nhwc] {NAME[dt]}: {n_cases} cases bit exact")


def test_avgpool_nhwc_f32_is_bit_exact(hip):
    """avgpool_nhwc_f32_kernel sums the positions in index order too."""
    n_cases = 0
    for x in avg_cases(F32, R.AVG_C + (3,)):
        n, h, w, c = x.shape
        assert torch.equal(hip.avgpool_nhwc_f32(x.cuda()).cpu(), R.avgpool_seq_ref(x.view(n, h * w, c))), tuple(x.shape)
        n_cases += 1
    print(f"[avgpool_nhwc_f32] f32: {n_cases} cases bit exact")


def test_avgpool_rows_against_fp64(hip):
    worst = Worst("avgpool_rows", "abs")
    for hw in R.ROWS_HW:
        for n, c in R.ROWS_NC:
            x = R.avgpool_rows_case(n, c, hw)
            got = hip.avgpool_rows(x.cuda())
            assert got.shape == (n, c)
            worst.add(hw, R.abs_err(got, x.double().mean(dim=(2, 3))), f"HW={hw} rows={n * c}")
    worst.check(lambda key: R.YARD_MULT * ROWS_YARD[key])


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def test_layouts_are_exact(hip):
    n_cases = 0
    for c in R.LAYOUT_DIMS:
        for hw in R.LAYOUT_DIMS:
            for n in R.POOL_N:
                x = R.randn(n, c, hw, 1, seed=c * 101 + hw + n)
                got = hip.nchw_to_rows(x.cuda())
                assert got.shape == (n, hw, c) and torch.equal(got.cpu(), x.view(n, c, hw).permute(0, 2, 1)), ("nchw_to_rows", n, c, hw)
                n_cases += 1
    for c in (1, 3, 4):
        for cp in (4, 8):
            x = R.randn(2, c, 5, 7, seed=c + cp)
            got = hip.nchw_to_nhwc_f32(x.cuda(), cp=cp).cpu()
            assert torch.equal(got, R.nhwc_pad_ref(x, cp)) and bool((got[..., c:] == 0).all()), ("nchw_to_nhwc_f32", c, cp)
            n_cases += 1
    for dt in DT16:
        for c in (1, 3, 4, 5, 8):
            for h, w in ((1, 1), (5, 7), (3, 9)):
                x = R.randn(2, c, h, w, seed=c + h + w)
                got = hip.pack_nchw_to_nhwc8(x.cuda(), out_dtype=dt).cpu()
                assert got.dtype == dt and torch.equal(got.view(torch.int16), R.pack_nhwc8_ref(x, dt).view(torch.int16)), ("pack", NAME[dt], c, h, w)
                n_cases += 1
    print(f"[nchw_to_rows / nchw_to_nhwc_f32 / pack_nchw_to_nhwc8] {n_cases} cases exact")


# ---- normalisations -------------------------------------------------------------------------------------------------------------
def test_normalisations_are_bit_exact(hip):
    for c in (1, 3, 4):
        x = R.bytes_image(2, 17, 19, c, seed=c)
        assert all(len(torch.unique(x[..., ch])) == 256 for ch in range(c))
        mean, std = R.NORM_MEAN[:c], R.NORM_STD[:c]
        want = R.normalize_ref(x, mean, std)
        got = hip.normalize_u8_hwc(x.cuda(), mean.cuda(), std.cuda())
        assert torch.equal(got.cpu(), want), ("normalize_u8_hwc", c)
        for dt in DT16:
            fused = hip.normalize_pack_u8(x.cuda(), mean.cuda(), std.cuda(), out_dtype=dt)
            assert torch.equal(fused, hip.pack_nchw_to_nhwc8(got, out_dtype=dt)), ("normalize_pack_u8 vs pack", NAME[dt], c)
            assert torch.equal(fused.cpu().view(torch.int16), R.pack_nhwc8_ref(want, dt).view(torch.int16)), ("normalize_pack_u8", NAME[dt], c)
    print("[normalize_u8_hwc / normalize_pack_u8] C = 1, 3, 4, all byte values: bit exact")


# ---- wrap cases: the second trip of each capped grid-stride loop ---------------------------------------------------------------
def test_wrap_maxpool_nchw(hip):
    shape = R.WRAP["maxpool3x3s2"][1]["shape"]
    assert R.wraps("maxpool3x3s2", shape)
    x = -(torch.randint(1, 200, shape, generator=R.gen(1), dtype=torch.uint8).float())
    assert torch.equal(hip.maxpool3x3s2(x.cuda()).cpu(), R.maxpool_ref(x))
    print(f"[maxpool3x3s2] wrap {shape}: exact")


def test_wrap_maxpool_nhwc(hip):
    """Small negative integers, exact in both 16-bit types: one fp32 reference serves both."""
    shape = R.WRAP["maxpool3x3s2_nhwc"][1]["shape"]
    assert R.wraps("maxpool3x3s2_nhwc", shape)
    x = -(torch.randint(1, 200, shape, generator=R.gen(2), dtype=torch.uint8).float())
    want = nhwc(R.maxpool_ref(nchw(x)))
    for dt in DT16:
        got = hip.maxpool3x3s2_nhwc(x.to(dt).cuda())
        assert torch.equal(got.cpu().float(), want), NAME[dt]
    print(f"[maxpool3x3s2_nhwc] wrap {shape}: exact in bf16 and fp16")


def test_wrap_normalise_and_pack(hip):
    """normalize_u8_hwc, normalize_pack_u8 and pack_nchw_to_nhwc8 on one image just past 8,388,608 pixels."""
    shape = R.WRAP["normalize_u8_hwc"][1]["shape"]
    assert all(R.wraps(k, R.WRAP[k][1]["shape"]) for k in ("normalize_u8_hwc", "normalize_pack_u8", "pack_nchw_to_nhwc8"))
    assert R.WRAP["normalize_pack_u8"][1]["shape"] == shape and R.WRAP["pack_nchw_to_nhwc8"][1]["shape"] == (shape[0], shape[3]) + shape[1:3]
    x = torch.randint(0, 256, shape, generator=R.gen(3), dtype=torch.uint8)
    mean, std = R.NORM_MEAN[:3], R.NORM_STD[:3]
    want = R.normalize_ref(x, mean, std)
    got = hip.normalize_u8_hwc(x.cuda(), mean.cuda(), std.cuda())
    assert torch.equal(got.cpu(), want)
    for dt in DT16:
        want16 = want.permute(0, 2, 3, 1).to(dt).view(torch.int16)
        for name, out in (("normalize_pack_u8", hip.normalize_pack_u8(x.cuda(), mean.cuda(), std.cuda(), out_dtype=dt)),
                          ("pack_nchw_to_nhwc8", hip.pack_nchw_to_nhwc8(got, out_dtype=dt))):
            out = out.cpu().view(torch.int16)
            assert torch.equal(out[..., :3], want16) and bool((out[..., 3:] == 0).all()), (name, NAME[dt])
    print(f"[normalize_u8_hwc / normalize_pack_u8 / pack_nchw_to_nhwc8] wrap {shape}: bit exact")


def test_wrap_round16_keep_nonzero(hip):
    shape = R.WRAP["round16_keep_nonzero"][1]["shape"]
    assert R.wraps("round16_keep_nonzero", shape)
    x = R.randn(*shape, seed=4)
    x[::7] *= 1e-9
    x[::11] *= 1e-30
    x[::13] = 0.0
    x[5::13] = -0.0
    for dt in DT16:
        got = hip.round16_keep_nonzero(x.cuda(), dt)
        assert torch.equal(got.cpu().view(torch.int16), R.round16_keep_nonzero_ref(x, dt).view(torch.int16)), NAME[dt]
    print(f"[round16_keep_nonzero] wrap {shape}: bit exact in bf16 and fp16")


# ---- what the C entry points reject before any launch, and the wrapper contracts -----------------------------------------------
def test_sixteen_bit_pools_reject_fp32(hip):
    x = torch.zeros(1, 3, 3, 8, device="cuda")
    for fn in (hip.maxpool3x3s2_nhwc, hip.avgpool_nhwc):
        with pytest.raises(RuntimeError, match="dh_"):
            fn(x)


def test_pool_wrappers_refuse_or_answer(hip):
    """A view of a wider buffer (every stride but the last doubled): the right answer or an AssertionError, never silence."""
    wide = lambda t: torch.cat([t, t - 1], -1).cuda()[..., :t.shape[-1]]      # noqa: E731
    res = {}
    x = R.negative(2, 8, 5, 6, seed=1)
    res["maxpool3x3s2"] = right_or_refused(lambda: hip.maxpool3x3s2(wide(x)), R.maxpool_ref(x))
    res["avgpool_rows"] = right_or_refused(lambda: hip.avgpool_rows(wide(x)), x.mean(dim=(2, 3)))
    res["nchw_to_rows"] = right_or_refused(lambda: hip.nchw_to_rows(wide(x)), x.view(2, 8, 30).permute(0, 2, 1))
    res["nchw_to_nhwc_f32"] = right_or_refused(lambda: hip.nchw_to_nhwc_f32(wide(x[:, :3]), cp=4), R.nhwc_pad_ref(x[:, :3], 4))
    xl = nhwc(x)
    res["maxpool3x3s2_nhwc_f32"] = right_or_refused(lambda: hip.maxpool3x3s2_nhwc_f32(wide(xl)), nhwc(R.maxpool_ref(x)))
    res["avgpool_nhwc_f32"] = right_or_refused(lambda: hip.avgpool_nhwc_f32(wide(xl)), R.avgpool_seq_ref(xl.view(2, 30, 8)))
    for dt in DT16:
        x16 = xl.to(dt)
        res[f"maxpool3x3s2_nhwc {NAME[dt]}"] = right_or_refused(lambda: hip.maxpool3x3s2_nhwc(wide(x16)), nhwc(R.maxpool_ref(nchw(x16.float()))).to(dt))
        res[f"avgpool_nhwc {NAME[dt]}"] = right_or_refused(lambda: hip.avgpool_nhwc(wide(x16)), R.avgpool_seq_ref(x16.view(2, 30, 8)))
    print(f"[wrappers] {res}")
