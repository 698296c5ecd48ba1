"""The 16-bit encoder's kernel schedule (``encoders._schedule``), pinned.  Every specialised trunk kernel is bit-identical to the
implicit-GEMM tile kernel, so no result test notices a bottleneck routed to a slower one: these rows say which kernel runs each
convolution.  They are the launches of one forward in a kernel trace (rocprofv3 --kernel-trace) of the encoder before the schedule
existed, at the same shapes and levels."""
import pytest
import torch

import deephumor_amd.models as M
from deephumor_amd.models.encoders import Step, _schedule

T, WREG, S4, DIRECT = "conv2d_nhwc_bn_act", "conv1x1_wreg_nhwc", "conv3x3_s4_nhwc", "conv3x3_direct_nhwc"
DUAL, DUALW = "conv1x1_dual_nhwc", "conv1x1_dual_wreg_nhwc"
RING, S1, S2, S3 = "bottleneck_tail_nhwc", "bottleneck_tail_s1_nhwc", "bottleneck_tail_s2_nhwc", "bottleneck_tail_s3_nhwc"
STEM = "stem_conv7_bn_relu_maxpool"


def tail(name, conv1=T, fuse=False):
    return Step(conv1, name, name, fuse)


# (N, H, W, encoder_generic) -> (stem, [Step] of layer1.0 .. layer4.2)
CASES = {
    (256, 224, 224, 0): (STEM, [Step(T, DIRECT, DUALW, True), tail(S1, None, True), tail(RING, None),
                                Step(WREG, T, DUALW, False), tail(S2, WREG, True), tail(S2, None, True), tail(S2, None),
                                Step(WREG, T, DUALW, False)] + [tail(S3, WREG)] * 5
                         + [Step(WREG, T, DUAL, False)] + [Step(T, S4, WREG, False)] * 2),
    (256, 224, 224, 1): (STEM, [Step(T, DIRECT, DUAL, False)] + [tail(RING)] * 2 + [Step(T, T, DUAL, False)] + [tail(RING)] * 3
                         + [Step(T, T, DUAL, False)] + [tail(S3)] * 5 + [Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 2),
    (256, 224, 224, 2): (STEM, ([Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 2) + ([Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 3)
                         + ([Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 5) + ([Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 2)),
    (4, 224, 224, 0): (STEM, [Step(T, DIRECT, DUALW, True), tail(S1, None, True), tail(RING, None),
                              Step(WREG, T, DUAL, False), tail(S2, T, True), tail(S2, None, True), tail(S2, None),
                              Step(T, T, DUAL, False)] + [tail(S3)] * 5 + [Step(T, T, DUAL, False)] + [Step(T, S4, T, False)] * 2),
    # stages at 40 x 56 / 20 x 28 / 10 x 14 / 5 x 7: no register-streamed tail, the ring tail in stages 1 and 2
    (3, 160, 224, 0): (STEM, [Step(T, DIRECT, DUAL, False)] + [tail(RING)] * 2 + [Step(T, T, DUAL, False)] + [tail(RING)] * 3
                       + [Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 5 + [Step(T, T, DUAL, False)] + [Step(T, T, T, False)] * 2),
}
# level 3: level 2's bottlenecks behind the implicit-GEMM stem (+ max-pool)
CASES[(256, 224, 224, 3)] = (T, CASES[(256, 224, 224, 2)][1])


@pytest.fixture(scope="module")
def encoder():
    return M.ImageEncoder(256, spatial_features=True).eval().bfloat16()


@pytest.mark.parametrize("n,h,w,level", sorted(CASES))
def test_encoder_16bit_schedule(encoder, n, h, w, level):
    stem, steps = _schedule(encoder._bottlenecks(), (n, 3, h, w), False, level)
    want_stem, want_steps = CASES[(n, h, w, level)]
    assert stem == want_stem
    assert len(steps) == len(want_steps) == 16
    for i, (got, want) in enumerate(zip(steps, want_steps)):
        assert got == want, (i, got, want)
    # the packed input layout ([N, H, W, 8]) reads the same size
    assert _schedule(encoder._bottlenecks(), (n, h, w, 8), True, level) == (stem, steps)


def test_encoder_16bit_on_cpu_tensors_still_refused(encoder):
    with pytest.raises(RuntimeError, match="need CUDA"):
        encoder.features(torch.zeros(1, 3, 64, 64))
