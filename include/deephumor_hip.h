/*
 * deephumor_hip.h -- C-ABI of the MI355X (gfx950) image->caption hot path.
 *
 * The reference (ilya16/deephumor) is pure Python on torch ops; it has no FFI of its own.  Each
 * entry point below replaces the torch call sites named in its comment (file:line under the
 * reference tree) and is what a maintainer would bind from the modules under deephumor/models through ctypes
 * (see INTEGRATION.md).  Conventions, all entry points:
 *   - plain device pointers + explicit sizes; no torch types; no allocation, no host sync and no
 *     stream sync inside; workspace is supplied by the caller; re-entrant across streams;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - returns DH_OK (0) or a DH_ERR_* code; dh_error_string() names it;
 *   - `dtype` is the storage type of activations and weights: DH_F32 (the parity path, bit-exact
 *     greedy ids vs the reference) or DH_BF16 / DH_F16 (the throughput paths: 16-bit storage in HBM, 16-bit MFMA
 *     operands, fp32 accumulation; bias/scale/shift/LayerNorm vectors stay fp32; wherever a comment below says
 *     "bf16" or "DH_BF16 only" the entry point takes DH_F16 as well).  An entry point that lacks a
 *     dtype returns DH_ERR_UNSUPPORTED for it.
 *   - row-major everywhere; images NCHW; "rows" are (image, beam) pairs, image-major.
 */
#ifndef DEEPHUMOR_HIP_H
#define DEEPHUMOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_ABI_VERSION 35

enum { DH_OK = 0, DH_ERR_BAD_ARG = 1, DH_ERR_UNSUPPORTED = 2, DH_ERR_LAUNCH = 3 };
enum { DH_F32 = 0, DH_BF16 = 1,          /* storage type of activations and weights */
       DH_BF16_OUT_F32 = 2,              /* dh_linear only: bf16 operands, fp32 output (logits) */
       DH_F16 = 3,                       /* IEEE half storage / v_mfma_f32_16x16x32_f16 operands (BASELINE config 5) */
       DH_F16_OUT_F32 = 4,               /* dh_linear only: fp16 operands, fp32 output */
       DH_F32_OUT_PLANES = 5 };          /* dh_attn_self_decode / dh_attn_cross_decode only: fp32 operands, `out` = the fp16 planes
                                            [2][rows][D] (hi = fp16(x), lo = fp16((x - hi) * 2^11)) of the split-operand GEMM that
                                            consumes the result (option "f32_split": dh_linear_f32xp_wreg) */

/* device-side error bits OR-ed into the `err` word of the beam kernels */
enum { DH_BEAM_ERR_ALL_FILTERED = 1,   /* every logit filtered (-inf): reference raises RuntimeError, beam.py:46 */
       DH_BEAM_ERR_OVERFLOW = 2,       /* more than DH_BEAM_MAX_SURVIVORS logits at a row's top-k threshold in a pre-filtered kernel: repeat
                                          the step / batch with dh_beam_row_sample_exact (the models do) */
       DH_BEAM_ERR_TOO_FEW = 4,        /* informational: fewer positive-probability tokens than beams (dead beams, as torch's
                                          zero-probability picks) */
       DH_BEAM_ERR_NONFINITE = 8 };    /* a row's top-k survivors hold NaN or +inf: softmax is NaN, the reference's torch.multinomial raises
                                          RuntimeError (beam.py:46); the kernels hand on a finite dummy pick (token 0) */
#define DH_BEAM_MAX_SURVIVORS 1024
#define DH_BEAM_MAX_BEAMS 64
#define DH_BEAM_MAX_HISTORY 1024     /* longest row history dh_beam_history_logits looks at (token columns < pos) */
#define DH_BEAM_MAX_BAD_WORDS 4096   /* most phrases of one dh_beam_constrain_logits list */
#define DH_BEAM_MAX_BAD_LEN 32       /* most token ids of one phrase */

int dh_abi_version(void);
const char* dh_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * Encoder (deephumor/models/encoders.py:46-70, torchvision resnet50 trunk at :34-38,56)
 * ------------------------------------------------------------------------------------------- */

/* y = act( conv2d(x, w) * scale[co] + shift[co] (+ residual) ).  Replaces Conv2d(bias=False) +
 * eval-mode BatchNorm2d (+ residual add) (+ ReLU) of one trunk layer.  scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale, precomputed by the caller.  x [N,Cin,H,W], w [Cout,Cin,KH,KW],
 * residual/y [N,Cout,Ho,Wo], Ho = (H+2*pad-KH)/stride+1.  KH==KW in {1,3,7}. residual may be NULL. */
int dh_conv2d_bn_act(const void* x, const void* w, const float* scale, const float* shift,
                     const void* residual, void* y, int N, int Cin, int H, int W, int Cout,
                     int KH, int KW, int stride, int pad, int relu, int dtype, void* stream);

/* Channels-last (NHWC) bf16 convolution on the matrix cores, same fused epilogue.  x [N,H,W,Cin],
 * w [Cout,KS,KS,Cin] (repacked once from the checkpoint's [Cout,Cin,KS,KS]), residual/y [N,Ho,Wo,Cout].
 * Implicit GEMM: rows = output pixels, k = (kh,kw,ci); Cin % 8 == 0.  DH_BF16 only. */
int dh_conv2d_nhwc_bn_act(const void* x, const void* w, const float* scale, const float* shift,
                          const void* residual, void* y, int N, int H, int W, int Cin, int Cout,
                          int KS, int stride, int pad, int relu, int dtype, void* stream);

/* The ResNet stem in one launch (16-bit dtypes): conv + BatchNorm + ReLU + MaxPool2d(3, 2, 1) -- torchvision resnet children
 * conv1, bn1, relu, maxpool (encoders.py:37-38).  A workgroup computes the 15 x 15 patch of convolution pixels under a 7 x 7
 * block of pooled pixels and pools it in LDS: the 4x larger un-pooled activation (411 MB at 256 images) is neither written nor
 * read back.  x NHWC [N,H,W,Cin] (Cin % 8 == 0: the packed image), w [Cout,KS,KS,Cin], y NHWC [N,Ho/2,Wo/2,Cout]; conv output
 * Ho, Wo even; Cout <= 64.  Bit-identical to dh_conv2d_nhwc_bn_act + dh_maxpool3x3s2_nhwc (rounding is monotonic). */
int dh_conv2d_nhwc_bn_relu_maxpool(const void* x, const void* w, const float* scale, const float* shift, void* y, int N,
                                   int H, int W, int Cin, int Cout, int KS, int stride, int pad, int dtype, void* stream);

/* The ResNet-50 stem as a DIRECT convolution on the matrix cores (16-bit dtypes): conv 7x7 / stride 2 / pad 3, 3 -> 64
 * channels, + BatchNorm + ReLU + MaxPool2d(3, 2, 1) -- torchvision resnet children conv1, bn1, relu, maxpool
 * (encoders.py:37-38) -- reading the caller's image as it is: x_fmt 0 = fp32 NCHW [N,3,H,W] (no packing launch in front),
 * x_fmt 1 = 16-bit channels-last [N,H,W,8] (dh_normalize_pack_u8 / dh_pack_nchw_to_nhwc8; channels 0..2 used).  A workgroup
 * loads the 35 x 36 input pixels under a 15 x 15 patch of convolution outputs once into LDS and forms the MFMA operands at
 * ds_read time (one MFMA = one kernel row: K = 8 kw slots x 4 channels), so neither an im2col matrix nor the un-pooled
 * activation ever exists.  w [64][7 kh][8 kw slots][4 channels] 16-bit (slot 7 and channel 3 zero; repacked once by the
 * caller from the checkpoint's [64,3,7,7]), scale/shift fp32 [64], y channels-last [N, Ho/2, Wo/2, 64]; conv output Ho, Wo even. */
int dh_stem_conv7_bn_relu_maxpool(const void* x, int x_fmt, const void* w, const float* scale, const float* shift, void* y,
                                  int N, int H, int W, int dtype, void* stream);

/* 3x3 / stride 1 / pad 1 convolution + BatchNorm + ReLU as a DIRECT convolution on the matrix cores (16-bit dtypes,
 * channels-last): the conv2 of the ResNet-50 bottlenecks of stages 1 and 2 (torchvision Bottleneck.conv2 / bn2 / relu).  A
 * workgroup brings the (4 + 2) x (W + 2) input pixels under four output rows into LDS once and serves all nine taps from
 * them; only the [Cout][64 k] weight slabs stream -- 3.5x less L2 -> LDS traffic per output pixel than the implicit GEMM of
 * dh_conv2d_nhwc_bn_act, same contract: x [N,H,W,Cin], w [Cout,3,3,Cin], y [N,H,W,Cout], relu must be 1.  Supported shapes
 * (dh_conv3x3_direct_supported != 0): H % 4 == 0 and (Cin = Cout = 64, W = 56) or (Cin = Cout = 128, W = 28); anything else
 * returns DH_ERR_BAD_ARG and belongs to dh_conv2d_nhwc_bn_act. */
int dh_conv3x3_direct_supported(int H, int W, int Cin, int Cout);
int dh_conv3x3_direct_nhwc(const void* x, const void* w, const float* scale, const float* shift, void* y, int N, int H,
                           int W, int Cin, int Cout, int relu, int dtype, void* stream);

/* The tail of a ResNet bottleneck in ONE launch (16-bit dtypes, channels-last): out = relu(bn3(conv3(relu(bn2(conv2(y1))))) +
 * residual), conv2 3x3 / stride 1 / pad 1 (C -> C), conv3 1x1 (C -> 4C) -- torchvision Bottleneck.forward from conv2 on
 * (encoders.py:37-38,56).  conv2 runs as in dh_conv3x3_direct_nhwc; its output tile never leaves LDS: it is the activation
 * operand of the 1x1 expansion, whose weights stream through the same LDS ring.  Bit-identical to dh_conv3x3_direct_nhwc
 * followed by dh_conv2d_nhwc_bn_act(1x1, residual, relu).  Shapes as dh_conv3x3_direct_supported(H, W, C, C).
 * y1 [N,H,W,C], w2 [C,3,3,C], w3 [4C,C], residual / out [N,H,W,4C], scale / shift fp32 per output channel. */
int dh_bottleneck_tail_nhwc(const void* y1, const void* w2, const float* scale2, const float* shift2, const void* w3,
                            const float* scale3, const float* shift3, const void* residual, void* out, int N, int H,
                            int W, int C, int dtype, void* stream);

/* The same bottleneck tail for STAGE 3 (H = W = 14, C = 256 -> 1024; torchvision layer3.1 .. layer3.5, reference encoders.py:37-38,56):
 * one image per workgroup, patch-resident 3x3, the weights streamed from L2 straight into registers in MFMA fragment order --
 * w2_packed / w3_packed = dh_pack_mfma_fragments of w2 viewed as [C][9 C] and of w3 [4C][C] (packed once per weight version).
 * w3_packed == NULL (and residual == NULL): only conv2 + bn2 + relu, out = [N,14,14,C].  Bit-identical to the unfused pair of
 * dh_conv2d_nhwc_bn_act launches. */
int dh_bottleneck_tail_s3_supported(int H, int W, int C);
int dh_bottleneck_tail_s3_nhwc(const void* y1, const void* w2_packed, const float* scale2, const float* shift2,
                               const void* w3_packed, const float* scale3, const float* shift3, const void* residual,
                               void* out, int N, int H, int W, int C, int dtype, void* stream);

/* The stage-1 form (56 x 56 x 64 -> 256; layer1.1-layer1.2), optionally with the NEXT bottleneck's conv1 + bn1 + relu (256 -> N1 = 64)
 * behind it in the same launch: the output tile is the operand of that conv1 straight from LDS, the 411 MB tensor is not read back
 * (csrc/conv_s1.hip).  w1_packed = dh_pack_mfma_fragments(w1' [N1][256]) or NULL.  Bit-identical to dh_bottleneck_tail_nhwc followed by
 * dh_conv2d_nhwc_bn_act (1x1). */
int dh_bottleneck_tail_s1_supported(int H, int W, int C, int N1);
int dh_bottleneck_tail_s1_nhwc(const void* y1, const void* w2_packed, const float* scale2, const float* shift2,
                               const void* w3_packed, const float* scale3, const float* shift3, const void* residual, void* out,
                               const void* w1_packed, const float* scale1, const float* shift1, void* y1_next, int N1, int N,
                               int H, int W, int C, int dtype, void* stream);

/* The stage-2 form of dh_bottleneck_tail_s3_nhwc (28 x 28 x 128 -> 512; layer2.1-layer2.3): four output rows of one image per
 * workgroup, three workgroups per CU, weights from L2 into registers, no barrier in the loops (csrc/conv_s2.hip).
 * w2_packed = dh_pack_mfma_fragments(w2 [128][3*3*128]), w3_packed = dh_pack_mfma_fragments(w3 [512][128]).
 * Bit-identical to dh_bottleneck_tail_nhwc. */
int dh_bottleneck_tail_s2_supported(int H, int W, int C);
int dh_bottleneck_tail_s2_nhwc(const void* y1, const void* w2_packed, const float* scale2, const float* shift2,
                               const void* w3_packed, const float* scale3, const float* shift3, const void* residual, void* out,
                               const void* w1_packed /* or NULL: + the NEXT bottleneck's conv1 + bn1 + relu (512 -> N1 = 128) on the output
                               chunks while they are in LDS; dh_pack_mfma_fragments(w1' [128][512]) */,
                               const float* scale1, const float* shift1, void* y1_next /* [N,28,28,N1] */, int N1,
                               int N, int H, int W, int C, int dtype, void* stream);

/* conv2 (3x3, stride 1) + bn2 + relu of the STAGE-4 bottlenecks without downsample (7 x 7 x 512; torchvision Bottleneck.conv2 / bn2 /
 * relu of layer4.1-2, encoders.py:37-38): a workgroup = (two images, half of the output channels), pixels resident in LDS without a
 * halo, weights from L2 into registers in fragment order (csrc/conv_s4.hip).  w_packed = dh_pack_mfma_fragments(w [512][3*3*512]).
 * Bit-identical to dh_conv2d_nhwc_bn_act (KS 3, stride 1, pad 1, relu). */
int dh_conv3x3_s4_supported(int H, int W, int C);
int dh_conv3x3_s4_nhwc(const void* x, const void* w_packed, const float* scale, const float* shift, void* y, int N, int H, int W, int C,
                       int dtype, void* stream);

/* 16-bit weight matrix w [R][K] row-major -> MFMA operand fragments: out[((k / 32) * (R / 16) + r / 16) * 64 + lane] (16 bytes) = the 8
 * values k = 32 s + 8 (lane >> 4) .. + 7 of row 16 rt + (lane & 15); R % 16 == 0, K % 32 == 0; out has R * K elements. */
int dh_pack_mfma_fragments(const void* w, void* out, int R, int K, void* stream);

/* 1x1 stride-1 convolution + BatchNorm (+ ReLU), no residual, channels-last rows, with the weights stationary in registers and the
 * pixels streamed through two LDS buffers (csrc/conv1x1_wreg.hip; torchvision Bottleneck.conv1 / bn1 / relu of the K >= 512 stages,
 * encoders.py:37-38): y [M, Cout] = relu?((x [M, Cin] w^T) * scale + shift), w_packed = dh_pack_mfma_fragments(w [Cout, Cin]).
 * Cin 256, 512 or 1,024, Cout / 128 in {1, 2, 4, 8, 16}, M >= 8,192 (_supported).  Bit-identical to dh_conv2d_nhwc_bn_act(KS = 1). */
int dh_conv1x1_wreg_supported(long long M, int Cin, int Cout);
int dh_conv1x1_wreg_nhwc(const void* x, const void* w_packed, const float* scale, const float* shift, const void* residual /* or NULL; Cin = 512 */,
                         void* y, long long M, int Cin, int Cout, int relu, int dtype, void* stream);

/* The dual form (dh_conv1x1_dual_nhwc: relu(bn3(conv3(y)) + bn_d(downsample(x))) of a stage's first bottleneck, encoders.py:37-38 /
 * torchvision Bottleneck.forward with `downsample`) in the same streaming structure, for the instances C1 + C2 = 128, 384 or 768,
 * Cout a multiple of 256 (_supported).  w_packed = dh_pack_mfma_fragments(w [Cout, C1 + C2]).  Bit-identical to dh_conv1x1_dual_nhwc. */
int dh_conv1x1_dual_wreg_supported(int N, int Ho, int Wo, int H, int W, int C1, int C2, int Cout);
int dh_conv1x1_dual_wreg_nhwc(const void* y, const void* x, const void* w_packed, const float* shift, void* out, int N, int Ho, int Wo,
                              int C1, int H, int W, int C2, int stride, int Cout, int relu,
                              const void* w1_packed /* or NULL: + the NEXT bottleneck's conv1 + bn1 + relu (Cout = 256 -> N1 = 64, C1 + C2 = 128) on the
                              block's outputs while they are in LDS; dh_pack_mfma_fragments(w1' [64][256]) */,
                              const float* scale1, const float* shift1, void* y1_next /* [N,Ho,Wo,N1] */, int N1, int dtype, void* stream);

/* Stem of the bf16 path: conv 7x7/2 (or 3x3) + BN + ReLU reading the caller's NCHW fp32 image (fp32
 * weights [Cout,Cin,KS,KS]) on the vector ALUs and writing channels-last bf16 y [N,Ho,Wo,Cout]. */
int dh_stem_conv_nhwc(const float* x, const float* w, const float* scale, const float* shift, void* y,
                      int N, int Cin, int H, int W, int Cout, int KS, int stride, int pad, int relu,
                      int dtype, void* stream);

/* relu(conv3(y) + downsample(x) + shift) as ONE launch: the end of a ResNet stage's first bottleneck (torchvision
 * Bottleneck.forward: out = relu(bn3(conv3(out)) + downsample(x))).  w = [W3 * bn3_scale | Wd * bnd_scale]
 * [Cout, C1 + C2] bf16 (the BatchNorm scales folded into the weights), shift = bn3_shift + bnd_shift.
 * y NHWC [N,Ho,Wo,C1], x NHWC [N,H,W,C2] read at pixel (oh*stride, ow*stride); C1, C2 % 64 == 0.  DH_BF16 only. */
int dh_conv1x1_dual_nhwc(const void* y, const void* x, const void* w, const float* shift, void* out, int N, int Ho, int Wo,
                         int C1, int H, int W, int C2, int stride, int Cout, int relu, int dtype, void* stream);

/* Input packing for a matrix-core stem: NCHW fp32 image [N,C,H,W] (C <= 8) -> channels-last bf16 [N,H,W,8] with
 * channels C..7 zero, so the 7x7 stem is a dh_conv2d_nhwc_bn_act with Cin = 8 (weights zero-padded likewise). */
int dh_pack_nchw_to_nhwc8(const float* x, void* y, int N, int C, int H, int W, int dtype, void* stream);

/* Image preprocessing on device: u8 [N,H,W,C] -> fp32 NCHW (x / 255 - mean[c]) / std[c], bit-identical to
 * torchvision ToTensor + Normalize (deephumor_demo.ipynb:566-567; the resize in front of it: dh_resize_u8_hwc). */
int dh_normalize_u8_hwc(const uint8_t* x, const float* mean, const float* stdv, float* y, int N, int H, int W, int C,
                        void* stream);

/* fp32 -> 16-bit (round to nearest even) that never turns a non-zero value into zero: a value that underflows in the storage type
 * becomes the smallest subnormal of its sign.  ImageEncoder's spatial features on the fp16 path go through it, because
 * TransformerDecoder reads an encoder row with any exactly-zero element as padding (reference transformers.py:480) and fp16
 * underflows below 3e-8 where fp32 / bf16 do not. */
int dh_round16_keep_nonzero(const float* x, void* y, long long n, int dtype, void* stream);

/* transforms.Resize((Hout, Wout)) of the notebook's pipeline (deephumor_demo.ipynb:565) for decoded 8-bit images on device:
 * Pillow's antialiased BILINEAR resample, bit-exact (horizontal pass into the 8-bit intermediate `tmp` [N,Hin,Wout,C], then
 * vertical -- except for images more than 100 x taller than wide whose height shrinks, which PIL/Image.py resizes vertically
 * first: intermediate [N,Hout,Win,C]; `tmp` must hold N * max(Hin * Wout, Hout * Win) * C bytes; 22-bit fixed-point weights,
 * accumulator 2^21 + sum, result clip8(acc >> 22)).  bounds_* [n_out][2] = (first
 * source index, count) and k* [n_out][ksize_*] int32 weights come from the host (Pillow's precompute_coeffs in double
 * precision: deephumor_amd.experiments.inference.resize_coefficients); a pass whose sizes agree is skipped.  C <= 8. */
int dh_resize_u8_hwc(const uint8_t* src, uint8_t* tmp, uint8_t* dst, const int32_t* bounds_x, const int32_t* kx, int ksize_x,
                     const int32_t* bounds_y, const int32_t* ky, int ksize_y, int N, int Hin, int Win, int Hout, int Wout,
                     int C, void* stream);

/* ToTensor + Normalize fused with the stem's input packing (16-bit paths): u8 [N,H,W,C] -> normalised bf16 / fp16
 * channels-last [N,H,W,8] (channels C..7 zero), bit-identical to dh_pack_nchw_to_nhwc8(dh_normalize_u8_hwc(x)) -- the
 * matrix-core stem convolution reads it directly, no fp32 NCHW tensor in front of conv1. */
int dh_normalize_pack_u8(const uint8_t* x, const float* mean, const float* stdv, void* y, int N, int H, int W, int C,
                         int dtype, void* stream);

/* Teacher-forced (prefill) forms of the decoder row kernels -- forward() over all positions at once (transformers.py
 * DecoderLayer.forward with the causal + pad mask of :471-478).  Rows are sequence-major: row n*n_pos + t.
 *   dh_embed_prefill      x = (t == 0 ? start_emb[n] : tok_emb[tokens[n, t-1]]) / scale + pos_emb[t]; start_emb == NULL:
 *                         x = tok_emb[tokens[n, t]] / scale + pos_emb[t] (forward without an image slot, transformers.py:432)
 *   dh_attn_self_prefill  causal self-attention over qkv [rows, 3D] of ONE projection GEMM (no KV cache); head dim 64,
 *                         n_pos <= 56 (bf16) / 40 (fp32); key j >= 1 masked where tokens[n, j-1] == pad_index
 *   dh_attn_cross_prefill every position of image n against that image's S patch keys kv [n_img*S, 2D] */
int dh_embed_prefill(const void* tok_emb, const void* pos_emb, const void* start_emb, const int32_t* tokens, int tok_ld,
                     void* x, int n_seq, int n_pos, int D, float scale, int dtype, void* stream);
int dh_attn_self_prefill(const void* qkv, const int32_t* tokens, int tok_ld, void* out, int n_seq, int n_pos, int D,
                         int n_heads, float scale, int pad_index, int dtype, void* stream);
int dh_attn_cross_prefill(const void* q, int ldq, const void* kv, const uint8_t* keymask, void* out, int n_img, int n_pos,
                          int S, int D, int n_heads, float scale, int dtype, void* stream);

/* Channels-last bf16 pools of the bf16 path: MaxPool2d(3,2,1) x [N,H,W,C] -> [N,Ho,Wo,C];
 * AdaptiveAvgPool2d(1) x [N,HW,C] -> y [N,C].  C % 8 == 0.  DH_BF16 only. */
int dh_maxpool3x3s2_nhwc(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
int dh_avgpool_nhwc(const void* x, void* y, int N, int HW, int C, int dtype, void* stream);

/* MaxPool2d(kernel 3, stride 2, padding 1) -- trunk index 3.  x [N,C,H,W] -> y [N,C,Ho,Wo]. */
int dh_maxpool3x3s2(const void* x, void* y, int N, int C, int H, int W, int dtype, void* stream);

/* AdaptiveAvgPool2d(1): x [rows, HW] -> y [rows] (rows = N*C).  encoders.py:60. */
int dh_avgpool_rows(const void* x, void* y, int rows, int HW, int dtype, void* stream);

/* features.reshape(bs, C, HW).transpose(2, 1): x [N,C,HW] -> y [N,HW,C].  encoders.py:65-66. */
int dh_nchw_to_rows(const void* x, void* y, int N, int C, int HW, int dtype, void* stream);

/* LabelEncoder: out[n, 0..E) = mean over the L label positions of emb[labels[n,j], :] (pads
 * included, encoders.py:104).  labels int64 [N, L]; out row stride ld_out (>= E). */
int dh_label_mean(const void* emb, const int64_t* labels, void* out, int ld_out, int N, int L, int E,
                  int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layers: nn.Linear call sites (encoders.py:61,67,142; rnn_models.py:44,81,109 classifier;
 * nn.LSTM gate products; transformers.py:97,127,162-163,488)
 * ------------------------------------------------------------------------------------------- */

/* C[m,n] = act( (sum_k A[m,k]*W[n,k] + bias[n]) * scale[n] + shift[n] + residual[m,n] ), fp32 accumulate
 * on the matrix cores (fp32: v_mfma_f32_32x32x2_f32, exact; bf16: v_mfma_f32_32x32x16_bf16).
 * A [M,K] lda, W [N,K] ldw (nn.Linear layout), C [M,N] ldc, residual [M,N] ldres (same type as C's
 * operands).  bias/scale/shift/residual may be NULL (scale/shift: eval-mode BatchNorm1d folded behind
 * the Linear, encoders.py:61).  K % 4 == 0 (fp32) / K % 8 == 0 (bf16). */
int dh_linear(const void* A, int lda, const void* W, int ldw, const float* bias,
              const float* scale, const float* shift, const void* residual, int ldres,
              void* C, int ldc, int M, int N, int K, int relu, int dtype, void* stream);

/* dh_linear with DEFERRED LayerNorm (16-bit dtypes): the post-LN decoder layer x = LN(x + sublayer(x))
 * (transformers.py:356-375) without a LayerNorm launch.  Rows travel PRE-LayerNorm together with per-(row, 64-column tile)
 * partial statistics {mean, M2 = sum of squared deviations from that mean}, [rows][D/64][2] fp32, written by the GEMM
 * that produced the rows (o_stats); a row's mean / rstd is the fixed-order combination of its tiles (deterministic).
 *   a_stats != NULL: the A rows are pre-LN.  The caller folded gamma into the weight (W'[n,k] = W[n,k] * gamma[k]) and
 *       beta into the bias (bias'[n] = bias[n] + sum_k beta[k] W[n,k]); a_colsum[n] = sum_k W'[n,k].  Then
 *       C = act( rstd[m] * (A W'^T - mu[m] * a_colsum) + bias' ) == act( LN(A) W^T + bias ).     a_tiles = K / 64 <= 8.
 *   r_stats != NULL: the residual rows are pre-LN: residual' = (residual - mu) * rstd * r_gamma[n] + r_beta[n].  r_tiles = N / 64.
 *   o_stats != NULL: partial statistics of the (rounded) output rows are written to o_stats[m][N / 64] (N % 64 == 0).
 * All of a_stats / r_stats / o_stats may be NULL (then this is dh_linear with bias + residual). */
typedef struct dh_ln_fold {
    const float* a_stats; int a_tiles; float a_eps; const float* a_colsum;
    const float* r_stats; int r_tiles; float r_eps; const float* r_gamma; const float* r_beta;
    float* o_stats;
} dh_ln_fold_t;
int dh_linear_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual, int ldres,
                 void* C, int ldc, int M, int N, int K, int relu, const dh_ln_fold_t* ln, int dtype, void* stream);

/* dh_linear_ln for the decode shapes with the weights stationary in registers (csrc/linear_wreg.hip; transformers.py:97,127,
 * 162-163 applied to the rows of one position): w_packed = dh_pack_mfma_fragments(W [N, K]) replaces (W, ldw).  Two forms:
 *   residual == NULL: optional ln->a_stats (deferred LayerNorm of the A rows), optional ReLU; K == 512, N % 64 == 0;
 *   residual != NULL: ln->o_stats required, ln->r_stats optional; K == 512 or 2,048, N % 64 == 0.
 * Results are bit-identical to dh_linear_ln on the unpacked weights.  _supported: 1 when (N, K, form) is taken. */
int dh_linear_ln_wreg_supported(int N, int K, int with_residual_stats);
/* 0.0 = shape not taken; else the fraction of resident workgroup slots the launch keeps busy over its residency rounds (1.0: one round):
 * the decode driver uses the register-stationary kernel at >= 0.85 and the tile kernels otherwise. */
double dh_linear_ln_wreg_occupancy(int M, int N, int K, int with_residual_stats);
int dh_linear_ln_wreg(const void* A, int lda, const void* w_packed, const float* bias, const void* residual, int ldres,
                      void* C, int ldc, int M, int N, int K, int relu, const dh_ln_fold_t* ln, int dtype, void* stream);
/* Vocabulary projection feeding beam search (bf16 operands): logits [M,V] fp32 = A*W^T + bias, and
 * group_max[m, g] = max(logits[m, 64g .. 64g+63]) for g < 2*ceil(V/128) (row stride gm_ld) -- the pre-filter
 * dh_beam_row_sample_groups uses to read only the ~top_k column groups that can hold a top-k logit.
 * logits == NULL: only the group maxima are produced (K % 64 == 0, K >= 128) (teacher-forced scoring, probes).
 * The padding of a logits row is SCRATCH: with ldl >= 128 * ceil(V / 128) the 256-row kernel stores whole 128-column panels, i.e.
 * it writes columns V .. 128 * ceil(V / 128) - 1 of every row too (finite values, never read); nothing outside [M, ldl] is touched. */
int dh_vocab_logits(const void* A, int lda, const void* W, int ldw, const float* bias, float* logits, int ldl,
                    float* group_max, int gm_ld, int M, int V, int K, int dtype, void* stream);

/* dh_vocab_logits with the weights streamed from L2 into registers in MFMA fragment order and the activation rows resident in LDS
 * (csrc/vocab_wreg.hip; the classifier of a beam-search step, rnn_models.py:45 / transformers.py:489 inside generate()).
 * w_packed = dh_pack_mfma_fragments(W padded to Vpad = ceil(V / 256) * 256 rows with copies of row V - 1) re-ordered chunk-major
 * ([16 k-steps][Vpad / 16 tiles][1 KB] -> [Vpad / 256 chunks][16 k-steps][16 tiles][1 KB]), bias_padded [Vpad] padded
 * likewise (NULL: no bias).  _supported: K = 512, M = 80 x {1, 2, 4, 8, 16, 32} or any M <= 640 (row blocks padded to a power of two
 * with idle workgroups, the last block's missing rows masked), ldl and gm_ld cover Vpad (ldl = 0: no logits).
 * Bit-identical to dh_vocab_logits on the columns [0, Vpad) and on the group maxima. */
int dh_vocab_logits_wreg_supported(int M, int V, int K, int ldl, int gm_ld);
int dh_vocab_logits_wreg(const void* A, int lda, const void* w_packed, const float* bias_padded, float* logits, int ldl,
                         float* group_max, int gm_ld, int M, int V, int K, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row addressing shared by the decoder kernels.  A decode step works on `rows` compact rows
 * rc = img*rows_per_img + w.  Persistent per-row state (tokens, KV cache, LSTM state) lives at
 * "logical" row rl = rc*row_mult of buffers sized for n_img*beam rows: before the first draw
 * every image has ONE row (rows_per_img=1, row_mult=beam), afterwards `beam` rows (row_mult=1).
 * ------------------------------------------------------------------------------------------- */

/* x[rc,:] = (pos==0 && start_emb ? start_emb[img,:] : tok_emb[token,:]) / scale + pos_emb[pos,:]
 * with token = tokens[rl*tok_ld + pos - (start_emb?1:0)].  transformers.py:455-469 / 697-718. */
int dh_embed_rows(const void* tok_emb, const void* pos_emb, const void* start_emb,
                  const int32_t* tokens, int tok_ld, void* x, int rows, int rows_per_img,
                  int row_mult, int pos, int D, float scale, int dtype, void* stream);

/* out = LayerNorm(x + y) * gamma + beta, eps as given (nn.LayerNorm default 1e-5), rows of D.
 * transformers.py:360,368,375.  out may alias x.  D % 4 == 0, D <= 4096. */
int dh_add_layernorm(const void* x, const void* y, const float* gamma, const float* beta,
                     void* out, int rows, int D, float eps, int dtype, void* stream);

/* Single-position masked multi-head self-attention over a KV cache (transformers.py:356 -> 97-127,
 * in the KV-cached form SURVEY.md 8(a) G-TR.4 shows equivalent).
 *   qkv   [rows, 3*D]  this position's q | k | v for every compact row (output of dh_linear)
 *   kcache/vcache [(pos_cap) * rows_total * D]  position-major cache of ONE layer; position t of
 *         logical row rl is written here by this call
 *   src   [rows_total, src_ld] int32: src[rl, j] = logical row whose cache slot holds position j of
 *         row rl's history (beam reordering is this indirection, never a copy), j < t
 *   tokens[rows_total, tok_ld]: key position j>=1 is masked iff tokens[rl, j-1] == pad_index
 *         (transformers.py:474-477); position 0 (image slot) never is.  pad_index < 0: no masking.
 *   out   [rows, D]
 * t = index of the current position (keys 0..t).  dynamic LDS = rows_per_img*(t+1+64)*4 bytes. */
int dh_attn_self_decode(const void* qkv, void* kcache, void* vcache, const int32_t* src, int src_ld,
                        const int32_t* tokens, int tok_ld, void* out, int n_img, int rows_per_img,
                        int row_mult, int rows_total, int t, int D, int n_heads, float scale,
                        int pad_index, int dtype, void* stream);

/* Single-position multi-head attention over the S image patches (transformers.py:364 -> 97-127).
 *   q [rows, ldq] (first D columns used), kv [n_img*S, 2*D] = fc_k | fc_v of enc_out (computed once
 *   per image), keymask [n_img*S] uint8 (1 = masked: some element of that enc_out row == 0,
 *   transformers.py:480-481), out [rows, D]. */
int dh_attn_cross_decode(const void* q, int ldq, const void* kv, const uint8_t* keymask, void* out,
                         int n_img, int rows_per_img, int S, int D, int n_heads, float scale,
                         int dtype, void* stream);

/* The attention WEIGHTS of that position, averaged over the heads (generate_batch(..., return_attention=True)): for the compact row
 * rc = img * rows_per_img + w,  out[rc * row_mult, j] = 1 / n_heads * sum_h softmax_j(q[rc, h] . k[img, j, h] / scale), j < S -- the
 * softmax of transformers.py:106-115 with masked keys at -1e8 (weight exactly 0 beside a live key; 1 / S when every key of the image
 * is masked).  q, kv (the K half is read) and keymask as for dh_attn_cross_decode, in DH_F32 / DH_BF16 / DH_F16; out fp32, row
 * stride S, written at the rows' LOGICAL slots (row_mult as in dh_attn_self_decode).  Scores, softmax and the head sum are fp32 with
 * the exact division and expf for every storage type; one wave per head, the waves' sums added in wave order through LDS (a fixed
 * order, no atomics).
 * q and kv 16-byte aligned, ldq % 8 == 0; DH_ERR_UNSUPPORTED beyond S = 8192. */
int dh_attn_cross_weights(const void* q, int ldq, const void* kv, const uint8_t* keymask, float* out, int n_img,
                          int rows_per_img, int row_mult, int S, int D, int n_heads, float scale, int dtype, void* stream);

/* The same attention on the matrix cores (16-bit dtypes, head dim 64, S <= 64, rows_per_img <= 16).  dh_attn_cross_pack
 * re-lays kv out ONCE per batch and layer as kp [n_img][n_heads][64 keys][64] and vt [n_img][n_heads][64][64 key slots]
 * (V transposed, key slots permuted into MFMA operand order, keys >= S zero) -- 16 KB per (image, head); dperm != 0
 * additionally permutes K's head-dim slots into the order of a 16 x 16 MFMA accumulator tile (the layout rounds 2-5's fused fc_q +
 * attention launch needed; kept as the product's default so that every 16-bit summation order -- and token -- stays what it was);
 * _decode_packed / _prefill_packed take the same flag and then read q in that slot order (prefill and decode agree bit for bit).  One wave then
 * handles one (image, head) straight from HBM: no LDS, no barrier, one memory round trip.  _prefill_packed: every
 * position of image n (rows n*n_pos + t) in ONE launch, 16 positions per row block of the grid; n_pos is any row count an image serves. */
int dh_attn_cross_pack(const void* kv, void* kp, void* vt, int n_img, int S, int D, int n_heads, int dperm, int dtype, void* stream);

int dh_attn_cross_decode_packed(const void* q, int ldq, const void* kp, const void* vt, const uint8_t* keymask, void* out,
                                int n_img, int rows_per_img, int S, int D, int n_heads, float scale, int dperm, int dtype, void* stream);
int dh_attn_cross_prefill_packed(const void* q, int ldq, const void* kp, const void* vt, const uint8_t* keymask, void* out,
                                 int n_img, int n_pos, int S, int D, int n_heads, float scale, int dperm, int dtype, void* stream);

/* keymask[r] = any(enc_out[r, :] == 0)  (transformers.py:480-481).  enc_out [rows, D]. */
int dh_enc_key_mask(const void* enc_out, uint8_t* keymask, int rows, int D, int dtype, void* stream);

/* Module-level API of the reference's transformer building blocks (the captioning models never call these directly;
 * they exist so that MultiHeadAttentionLayer.forward / DecoderLayer.forward / get_pad_mask / get_autoregressive_mask
 * keep working for callers of deephumor.models):
 *   dh_pad_mask             mask[b,q,k] = (key[b,k] == pad_index), uint8 [bs,Lq,Lk]        transformers.py:12-26
 *   dh_autoregressive_mask  mask[b,q,k] = (k > q), uint8 [bs,L,L]                          transformers.py:29-40
 *   dh_mask_or              a |= b over n bytes (input_mask = pad | causal)                transformers.py:477
 *   dh_enc_nonzero_rows     out[r] = all(enc_out[r,:] != 0) as int64                       transformers.py:480
 *   dh_attn_masked          softmax(q k^T / scale masked_fill(mask, -1e8)) v, heads merged transformers.py:99-124
 *                           q/k/v [bs*L, ld*] projected rows, mask uint8 [bs,L,L] or NULL, out [bs*L, D] */
int dh_pad_mask(const int64_t* key, uint8_t* mask, int bs, int Lq, int Lk, long long pad_index, void* stream);
int dh_autoregressive_mask(uint8_t* mask, int bs, int L, void* stream);
int dh_mask_or(uint8_t* a, const uint8_t* b, long long n, void* stream);
int dh_enc_nonzero_rows(const void* enc_out, int64_t* out, int rows, int D, int dtype, void* stream);
int dh_attn_masked(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const uint8_t* mask,
                   void* out, int bs, int L, int D, int n_heads, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM cell (nn.LSTM single time step; rnn_models.py:80,108)
 * ------------------------------------------------------------------------------------------- */

/* Gathers one step's inputs.  For every compact row rc (logical rl = rc*row_mult):
 *   xcat0[rc] = [ x_in , h_prev[0][hp] ],  xcatl[l-1][rc][Hh:2Hh] = h_prev[l][hp] (l>=1),
 *   c_cur[l][rc] = c_prev[l][hp]
 * where x_in = emb[tokens[rl*tok_ld + tok_pos]] if tokens != NULL else img_emb[img], and
 * hp = hparent ? hparent[rl] : rl; hp < 0 or h_prev == NULL means zero state.
 * h_prev/c_prev [n_layers, rows_total, Hh]; xcat0 [rows, E+Hh]; xcatl [n_layers-1, rows, 2*Hh];
 * c_cur [n_layers, rows, Hh].  Embeddings / hidden states have the storage dtype; the cell state c
 * (c_prev, c_cur) is always fp32. */
int dh_lstm_prepare(const void* emb, const void* img_emb, const int32_t* tokens, int tok_ld, int tok_pos,
                    const int32_t* hparent, const void* h_prev, const float* c_prev,
                    void* xcat0, void* xcatl, float* c_cur, int rows, int rows_per_img, int row_mult,
                    int rows_total, int n_layers, int E, int Hh, int dtype, void* stream);

/* gates [rows, 4*Hh] fp32 in PyTorch order i,f,g,o (biases already added by dh_linear; with bf16
 * operands use DH_BF16_OUT_F32 there), c_cur / c_new fp32, h_new / h_out in the storage dtype:
 *   c' = sigmoid(f)*c_cur + sigmoid(i)*tanh(g);  h' = sigmoid(o)*tanh(c')
 * writes h_new[rl], c_new[rl] (state at logical rows) and h_out[rc*ld_out + 0..Hh) (next layer's
 * input slot or the classifier input). */
int dh_lstm_cell(const float* gates, const float* c_cur, void* h_new, float* c_new, void* h_out,
                 int ld_out, int rows, int row_mult, int Hh, int dtype, void* stream);
/* The same two row kernels for fp32 rows on the split-operand path with the gate GEMM's operand ALSO stored as fp16 planes (hi, lo * 2^11;
 * options "f32_split" + "f32_planes"): xcat0_planes [2][rows][E + Hh], xcatl_planes [n_layers - 1][2][rows][2 Hh]; dh_lstm_cell_f32x
 * stores the new hidden row into h_planes (hi at h_planes, lo `plane` elements further, row stride ld_planes). */
int dh_lstm_prepare_f32x(const float* emb, const float* img_emb, const int32_t* tokens, int tok_ld, int tok_pos,
                         const int32_t* hparent, const float* h_prev, const float* c_prev, float* xcat0, float* xcatl, float* c_cur,
                         void* xcat0_planes, void* xcatl_planes, int rows, int rows_per_img, int row_mult, int rows_total,
                         int n_layers, int E, int Hh, void* stream);
int dh_lstm_cell_f32x(const float* gates, const float* c_cur, float* h_new, float* c_new, float* h_out, int ld_out,
                      void* h_planes, long long plane, int ld_planes, int rows, int row_mult, int Hh, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Beam-search step (deephumor/models/beam.py:32-108; rnn_models.py:87-103,111-137;
 * transformers.py:532-545,552-573,576-577)
 * ------------------------------------------------------------------------------------------- */

/* Per row: top-k filter (threshold = k-th largest, strict '<', ties kept, unk always dropped),
 * p = softmax(filtered / temperature), draw `beam` tokens without replacement as the top-`beam`
 * of p / Exp(1)-noise (== torch.multinomial on CPU), gather, log_softmax over the picks.
 *   logits [rows, ldl] fp32 (read only); pick_idx/pick_val [rows, beam]
 *   noise: NULL -> counter-based Philox noise keyed by (seed ^ *seed_ptr, img0+img, step, row, token)
 *          (seed_ptr: optional device-resident word, so a captured hipGraph can be replayed with new seeds);
 *          else [rows, ldl] fp32 Exp(1) samples supplied by the caller (RNG-replay parity tests)
 *   err: int32 word, DH_BEAM_ERR_* bits are OR-ed in. */
int dh_beam_row_sample(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                       int top_k, float temperature, int unk_index, const float* noise,
                       uint64_t seed, const uint64_t* seed_ptr, int img0, int step, int32_t* pick_idx,
                       float* pick_val, int32_t* err, void* stream);

/* dh_beam_row_sample on the general kernel only: any top_k / V, and a row with more than DH_BEAM_MAX_SURVIVORS logits at its top-k
 * threshold (flat or constant logits: beam.py:34 keeps every tie) is drawn over the whole row instead of flagging
 * DH_BEAM_ERR_OVERFLOW.  Slower; the models repeat a batch through it when the pre-filtered kernels flagged that overflow. */
int dh_beam_row_sample_exact(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                             int top_k, float temperature, int unk_index, const float* noise,
                             uint64_t seed, const uint64_t* seed_ptr, int img0, int step, int32_t* pick_idx,
                             float* pick_val, int32_t* err, void* stream);

/* Teacher-forced scoring without materialising the logits (bf16): logp[m] = log_softmax(A[m,:] W^T + bias)[targets[m]]
 * (metrics.py:4-9 via F.cross_entropy).  group_max / group_sum [M, gm_ld >= 2*ceil(V/128)] and target_logit [M] are
 * scratch.  targets outside [0, V) give logp = 0.  K % 64 == 0, K >= 128.
 * dtype == DH_F32: A is fp32 [M, lda] (lda % 4 == 0, 16-byte aligned) and W holds the dh_split_f32x planes of the classifier weight,
 * [2][V][ldw] fp16 with ldw = Kp (a multiple of 32, >= K); bias fp32; everything else as above, K % 64 == 0 and K >= 128 too.  The
 * f32x tile (dh_linear_f32x) in a log-sum-exp mode: fp32-class values, no logits written, ONE kernel for every M -- a row's result
 * does not depend on M or on its place in the batch -- fixed reduction order, no float atomics.  An activation with |x| >= 65504
 * sets the stream's sticky overflow word (dh_f32x_take_overflow) like every other f32x kernel. */
int dh_vocab_logprob(const void* A, int lda, const void* W, int ldw, const float* bias, const int64_t* targets, float* logp,
                     float* group_max, float* group_sum, float* target_logit, int gm_ld, int M, int V, int K, int dtype,
                     void* stream);

/* Same contract as dh_beam_row_sample, guided by the column-group maxima of dh_vocab_logits: the k-th largest
 * group maximum bounds the k-th largest logit from below, so only groups whose maximum reaches it are read. */
int dh_beam_row_sample_groups(const float* logits, int ldl, int V, const float* group_max, int gm_ld,
                              int n_groups, int group_cols, int rows, int rows_per_img, int beam,
                              int top_k, float temperature, int unk_index, const float* noise,
                              uint64_t seed, const uint64_t* seed_ptr, int img0, int step, int32_t* pick_idx,
                              float* pick_val, int32_t* err, void* stream);

/* Per image: builds the candidate list (a live beam contributes `beam` candidates, an ended beam one
 * with token 0 / score +0), draws `beam` of them without replacement from softmax(cand_val/T),
 * and rewrites the image's beam state IN PLACE.
 *   first != 0: the image has one source row (its picks are row img of pick_*): every new beam's
 *               parent is beam 0; `ended` is set from eos only if first_sets_ended (LSTM yes,
 *               Transformer no -- transformers.py:540-545 never updates has_ended there).
 *   tokens [R, tok_ld]: the picked token is written at column write_pos if write_pos < tok_ld
 *               (the Transformer's last step writes nothing, transformers.py:557).
 *   vals [R], ended [R] uint8, src [R, src_ld] (NULL for LSTM): src[r', 0..t) follow the parent,
 *               src[r', t] = parent row;  parent [R] / hparent [R]: logical parent rows for the
 *               sequence and for the LSTM state (rnn_models.py:135-137 quirk: candidate index / beam).
 *   done [n_img] uint8, end_step [n_img] int32: set to 1 / `step_index` when every beam of the image
 *               has ended (break at rnn_models.py:131 / transformers.py:572); done images are frozen.
 *   noise: NULL -> Philox; else [n_img, beam*beam] Exp(1) samples. */
int dh_beam_select(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                   float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                   int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                   int first, int first_sets_ended, int write_pos, int t, int step_index,
                   float temperature, int eos_index, const float* noise, uint64_t seed,
                   const uint64_t* seed_ptr, int img0, void* stream);

/* ---- Prompted batches: every image brings a caption prompt of its own length (the reference's `caption` argument,
 * rnn_models.py:73-103 / transformers.py:517-545, one image per call there).  The *_prompted entry points take the arguments of their
 * namesakes with the launch-wide `first` flag replaced by first_pos [n_img] int32 (device): image img's prompt length.  `step` /
 * `step_index` is the launch's absolute position; rows_per_img must equal beam.  Per image:
 *   step <  first_pos[img]  forced: no draw, no error bits, no noise consumed, its logits rows are not read (NaN there is harmless);
 *                           tokens / vals / ended / done untouched; parent, hparent and src[., t] of its rows = its base row img*beam.
 *   step == first_pos[img]  first : what first != 0 does with logical row img*beam as the single source row (its picks are row
 *                           img*beam of pick_*; noise keyed with row index 0, as the dense first step).
 *   step >  first_pos[img]  normal: the first == 0 step, bit for bit. */
int dh_beam_row_sample_prompted(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                int top_k, float temperature, int unk_index, const float* noise,
                                uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                int32_t* pick_idx, float* pick_val, int32_t* err, void* stream);
int dh_beam_row_sample_exact_prompted(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam,
                                      int top_k, float temperature, int unk_index, const float* noise,
                                      uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                      int32_t* pick_idx, float* pick_val, int32_t* err, void* stream);
int dh_beam_row_sample_groups_prompted(const float* logits, int ldl, int V, const float* group_max, int gm_ld,
                                       int n_groups, int group_cols, int rows, int rows_per_img, int beam,
                                       int top_k, float temperature, int unk_index, const float* noise,
                                       uint64_t seed, const uint64_t* seed_ptr, int img0, int step, const int32_t* first_pos,
                                       int32_t* pick_idx, float* pick_val, int32_t* err, void* stream);
int dh_beam_select_prompted(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                            float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                            int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                            const int32_t* first_pos, int first_sets_ended, int write_pos, int t, int step_index,
                            float temperature, int eos_index, const float* noise, uint64_t seed,
                            const uint64_t* seed_ptr, int img0, void* stream);

/* ---- Nucleus (top-p) row draw: dh_beam_row_sample on the nucleus of the top-k survivors, every route through ONE entry point.
 * 0 < top_p < 1 (anything else, 1 included, is DH_ERR_BAD_ARG: without a nucleus the entry points above are the call).  Per row:
 *   1. survivors as dh_beam_row_sample: logits >= the top_k-th largest, ties kept, unk dropped; p = softmax(survivors / temperature);
 *   2. survivors ordered by p descending, equal p by token index ascending;
 *   3. the survivor at sorted position j stays iff the exclusive prefix p[0] + ... + p[j-1] (fp32) is < top_p, or j < beam;
 *   4. the race of dh_beam_row_sample over those that stay: `beam` winners of p / Exp(1), ties to the lower index.  The noise is indexed
 *      by token id (Philox counter or noise[row, token]) as there; pick_val = log_softmax over the picks' untempered logits.
 * DH_BEAM_ERR_TOO_FEW keeps its meaning (fewer than `beam` survivors BEFORE the cut).  A row with more than DH_BEAM_MAX_SURVIVORS survivors
 * flags DH_BEAM_ERR_OVERFLOW on every route, exact included: there is no nucleus over a row in global memory.
 *   exact != 0       the general kernel (dh_beam_row_sample_exact's), group_max ignored;
 *   group_max != NULL (exact == 0) dh_beam_row_sample_groups' route: [rows, gm_ld] group maxima, n_groups groups of group_cols columns;
 *   otherwise        dh_beam_row_sample's choice of kernel by V and top_k (group_max, gm_ld, n_groups, group_cols unused);
 *   first_pos != NULL the prompted phases of the *_prompted entry points ([rows / beam] int32, rows_per_img == beam). */
int dh_beam_row_sample_nucleus(const float* logits, int ldl, int V, const float* group_max, int gm_ld, int n_groups,
                               int group_cols, int rows, int rows_per_img, int beam, int top_k, float top_p,
                               float temperature, int unk_index, const float* noise, uint64_t seed, const uint64_t* seed_ptr,
                               int img0, int step, const int32_t* first_pos, int exact, int32_t* pick_idx, float* pick_val,
                               int32_t* err, void* stream);

/* ---- Deterministic search (search="beam", not in the reference): the row step and the select step that keep the most likely
 * continuations instead of drawing.  No noise is generated or read, nothing is filtered by top_k, and two runs are bit-identical (no
 * float atomics; every reduction in a fixed order).
 * dh_beam_row_best, per row of fp32 logits [rows, ldl] as the samplers would see it (behind dh_beam_history_logits /
 * dh_beam_constrain_logits):
 *   lse      = logsumexp(x[0 .. V) / temperature) over every real column, unk_index included (mass the model assigns);
 *   pick_idx = the `beam` columns with the largest stored logit x, largest first; equal logits (-0.0 == +0.0) go to the lower column
 *              index; unk_index, -inf and columns >= V are never picked.  The order is on x itself: exact;
 *   pick_val = x[pick] / temperature - lse: the model's log-probability of the pick.
 * Picks go to pick_idx / pick_val [rows, beam] at row r, as dh_beam_row_sample leaves them.  err:
 *   DH_BEAM_ERR_NONFINITE     a NaN or +inf anywhere in the row's real columns (picks: token 0, value 0);
 *   DH_BEAM_ERR_ALL_FILTERED  no column but unk_index is > -inf (picks: token 0, value 0);
 *   DH_BEAM_ERR_TOO_FEW       fewer than `beam` such columns: the slots behind them hold token 0 at -inf (dead beams, informational);
 *   never DH_BEAM_ERR_OVERFLOW: a constant row has a defined answer, its `beam` lowest eligible columns.
 * group_max != NULL ([rows, gm_ld] maxima of n_groups <= 1024 groups of group_cols <= 64 columns, dh_beam_row_sample_groups' contract):
 * the second look at the row reads only the groups whose maximum reaches the bound the first sweep found; NULL: it reads the row again
 * (gm_ld, n_groups, group_cols are then not looked at).  Same picks either way.
 * rows_per_img = 1 for the dense first step (logits [n_img, V]), beam otherwise.  first_pos != NULL ([rows / beam] int32,
 * rows_per_img == beam): the prompted phases with `step` the absolute position -- a forced image's rows are neither read nor written,
 * an image at its first step uses its base row img * beam only.  beam <= DH_BEAM_MAX_BEAMS, 0 < temperature < inf, ldl >= V. */
int dh_beam_row_best(const float* logits, int ldl, int V, const float* group_max, int gm_ld, int n_groups, int group_cols,
                     int rows, int rows_per_img, int beam, float temperature, int unk_index, int step,
                     const int32_t* first_pos, int32_t* pick_idx, float* pick_val, int32_t* err, void* stream);

/* dh_beam_select / dh_beam_select_prompted without the draw: the candidate list is built exactly as there (a live beam: `beam`
 * candidates vals[b] + pick_val, one fp32 add; an ended beam: one candidate, token 0, its score unchanged) and the `beam` candidates
 * with the largest score stay, largest first; equal scores go to the lower candidate index, -inf ranks last.  Token rows, src, parent,
 * ended, done, end_step, write_pos and t are dh_beam_select's.  Two differences: hparent is the real parent row (base + parent beam),
 * not the dense-layout index; and the caller passes first_sets_ended = 1 for every decoder kind.
 * first_pos == NULL: a dense batch, `first` is the launch-wide flag; first_pos != NULL ([n_img] int32): the prompted phases of
 * dh_beam_select_prompted against step_index (`first` is not read). */
int dh_beam_select_best(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                        float* vals, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                        int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                        int first, const int32_t* first_pos, int first_sets_ended, int write_pos, int t, int step_index,
                        int eos_index, void* stream);

/* dh_beam_select_best with length normalisation (search="beam", length_penalty != 0): the same candidate list in the same order, ranked
 * by key = score * len_w[L] (ONE fp32 multiply of the fp32 score; -inf stays -inf) instead of the score.  len_w: fp32 [tok_ld + 1], the
 * caller's table (len_w[0] = 1, len_w[L] = L ** -length_penalty rounded once from fp64, every entry a positive normal number); no powf
 * runs on the device.  L = write_pos + 1 - first_col for every live candidate of an image -- first_col the image's first generated
 * column: the argument for a dense batch, first_pos[img] for a prompted one (first_col is then not read) -- clamped to [0, tok_ld].
 * An ended beam's candidate carries keys[its row], the key it was kept with, never recomputed at the current L.  The `beam` candidates
 * with the largest key stay, equal keys to the lower candidate index, -inf last; keys [rows] receives the kept candidates' keys and vals
 * their raw cumulative scores.  A first step ranks nothing and stores keys = pick_val * len_w[L] (L = 1 there).  A forced or a done image
 * leaves keys untouched.  ended, done, end_step, parent, hparent, src and the token rows are dh_beam_select_best's.
 * len_w, keys != NULL and first_col >= 0 are required. */
int dh_beam_select_best_norm(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                             float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                             int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                             int first, const int32_t* first_pos, int first_col, const float* len_w, int first_sets_ended,
                             int write_pos, int t, int step_index, int eos_index, void* stream);

/* dh_beam_select_best_norm with a finished-hypothesis pool (search="beam", early_stopping True / False).  Per image: pool_tokens int32
 * [beam, tok_ld], pool_keys / pool_vals fp32 [beam], pool_len int32 [beam], pool_n int32 -- physically sorted, slot 0 the largest key,
 * equal keys in order of arrival; the caller starts it with pool_n = 0 and pool_keys = -inf.  `ended` marks DEAD slots here (vals = keys =
 * -inf), which bring one candidate: token 0 at their score and key.  The candidates are built and ranked as dh_beam_select_best_norm
 * does (key = score * len_w[L]; len_w a table of ones without a length penalty; a first step keeps pick order).  Down the ranking: a
 * candidate whose token is eos_index never takes a slot -- with rank < beam and key > -inf it is offered to the pool: the parent's token
 * row with eos_index at write_pos, its key, its raw score, length write_pos + 1, inserted behind every entry whose key is >= its own;
 * entry `beam` falls off, so a full pool is entered only strictly above its worst key --; every other candidate with key > -inf takes
 * the next live slot until `beam` are taken, written as dh_beam_select_best_norm writes a kept candidate with ended = 0.  Slots left
 * over are dead: their own row with token 0 at write_pos, vals = keys = -inf, ended = 1, parent = hparent = src[.., t] = themselves
 * -- at an image's first step the image's base row instead, the only row with decoder state behind it (its token row holds the same
 * prefix).  The walk looks at the first 2 * beam ranks: a row's picks are distinct tokens, so at most `beam` candidates are eos_index.
 * done[img] = 1 and end_step[img] = step_index when the pool holds `beam` entries and stop_when_full is 1, or pool_keys[beam - 1] >=
 * keys of live slot 0 (-inf for a dead one).  Forced and done images: as dh_beam_select_best.  Plain vector stores in a fixed order, no
 * atomics.  Required: every pointer but src and first_pos, 0 <= write_pos < tok_ld, first_col >= 0, stop_when_full 0 or 1. */
int dh_beam_select_pool(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                        float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                        int32_t* hparent, uint8_t* done, int32_t* end_step, int32_t* pool_tokens, float* pool_keys,
                        float* pool_vals, int32_t* pool_len, int32_t* pool_n, int n_img, int beam,
                        int first, const int32_t* first_pos, int first_col, const float* len_w, int stop_when_full,
                        int write_pos, int t, int step_index, int eos_index, void* stream);

/* dh_beam_select_best_norm over diverse groups of beams (search="beam", num_beam_groups > 1; Vijayakumar et al. 2016).  The `beam` slots
 * of an image are n_groups groups of Bg = beam / n_groups: slots g * Bg .. g * Bg + Bg - 1 are group g at every step.  The candidate list
 * and the keys q = score * len_w[L] are dh_beam_select_best_norm's (len_w a table of ones without a length penalty); candidate c belongs to
 * group (its parent slot) / Bg, at an image's first step -- one source row -- to every group.  For g = 0 .. n_groups - 1 in order: `said`
 * holds the tokens the kept candidates of the groups before g took at this position; a candidate of a live row with a finite key gets
 * pen = fp32(q - fp32(diversity_penalty * fp32(times its token stands in said))) -- two separately rounded operations, no FMA --, an ended
 * beam's single candidate and a -inf candidate keep pen = q; the group's Bg candidates with the largest pen go to slots g * Bg + rank,
 * equal pen to the lower candidate index, -inf (and NaN) last; their tokens are appended to said (an ended beam's candidate and a
 * candidate at -inf add nothing).  What is stored is NOT penalised: vals gets the raw cumulative score, keys gets q.  ended, done,
 * end_step, parent, hparent, src, the token rows, forced and done images are dh_beam_select_best_norm's.  One wave per image does all its
 * groups; no atomics.  Required: what dh_beam_select_best_norm requires, n_groups >= 1 with beam % n_groups == 0, and a finite
 * diversity_penalty > 0. */
int dh_beam_select_groups(const int32_t* pick_idx, const float* pick_val, int32_t* tokens, int tok_ld,
                          float* vals, float* keys, uint8_t* ended, int32_t* src, int src_ld, int32_t* parent,
                          int32_t* hparent, uint8_t* done, int32_t* end_step, int n_img, int beam,
                          int first, const int32_t* first_pos, int first_col, const float* len_w, int first_sets_ended,
                          int write_pos, int t, int step_index, int eos_index, int n_groups, float diversity_penalty,
                          void* stream);

/* The result of a search with a pool, one launch, nothing written to the pool or the state: per image the pool's entries and -- unless
 * the image is done -- its live slots (ended == 0), offered in slot order through dh_beam_select_pool's insertion rule with the key
 * they were kept with and length min(full_len, tok_ld); the best `beam` stay.  Fewer than `beam`: the slots that were not offered follow
 * in slot order at score -inf with that length.  out_tokens [n_img, beam, out_ld]: every entry's row below its own length, pad_index
 * behind; out_len its length (<eos> included); out_score its key; out_index its live slot, -1 for an entry of the pool; out_drawn 0;
 * out_row_len = out_len[:, 0]. */
int dh_beam_finalize_pool(const int32_t* tokens, int tok_ld, const float* keys, const uint8_t* ended, const uint8_t* done,
                          const int32_t* pool_tokens, const float* pool_keys, const int32_t* pool_len, const int32_t* pool_n,
                          int32_t* out_tokens, int out_ld, int32_t* out_len, float* out_score, int32_t* out_index,
                          int32_t* out_drawn, int32_t* out_row_len, int n_img, int beam, int full_len, int pad_index,
                          void* stream);

/* ---- History-dependent logit edits in front of a row draw: no_repeat_ngram_size and repetition_penalty, IN PLACE on fp32 logits
 * [rows, ldl], one launch.  Logits row r reads its history h[0 .. pos) from tokens[r * tok_row_mult, 0 .. pos) (int32, row stride tok_ld):
 * tok_row_mult = beam for the dense first step (logits [n_img, V], image i's tokens at row i * beam), 1 otherwise.  Ids outside [0, V)
 * are never a column (they still take part in the n-gram comparison).  Per row, in this order:
 *   1. penalty != 1: for every DISTINCT token t of h, x = logits[t] becomes x < 0 ? x * penalty : x / penalty (fp32, correctly
 *      rounded division; once per token however often it occurs; -inf stays -inf);
 *   2. ngram = n >= 1 and pos >= n: for every j in [0, pos - n] with h[j .. j+n-2] == h[pos-n+1 .. pos-1], logits[h[j+n-1]] = -inf
 *      (n == 1: every token of h).  A banned column is -inf whatever the penalty did;
 *   3. group_max != NULL ([rows, gm_ld], n_groups groups of group_cols columns: dh_beam_row_sample_groups' contract): every group
 *      holding a column that step 1 or 2 stored to is recomputed as the exact fp32 maximum of the row's stored logits over the
 *      group's real columns (< V; pad columns a producer wrote are not looked at), -inf if they are all -inf.  Other groups,
 *      other logits are not written.  Pass group_max exactly when the sampler that follows reads it.
 * first_pos != NULL ([rows / rows_per_img] int32): the prompted phases with step = pos -- rows the *_prompted samplers do not
 * draw from (forced images; all but the base row of an image at its first step) are left untouched.
 * pos <= tok_ld and <= DH_BEAM_MAX_HISTORY, ngram >= 0 (0: off), penalty finite and > 0 (1: off); both off is DH_ERR_BAD_ARG: the
 * caller makes no launch then.  pos is a launch constant like `step`, so the call can be captured into a hipGraph. */
int dh_beam_history_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                           const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                           const int32_t* first_pos, int ngram, float penalty, void* stream);

/* ---- Bans in front of a row draw: min_len and a list of banned phrases, IN PLACE on fp32 logits [rows, ldl], one launch, on the row
 * geometry of dh_beam_history_logits (history h[0 .. pos) = tokens[r * tok_row_mult, 0 .. pos); first_pos: idle rows untouched).
 * The list is shared by all rows: phrase w is words[word_off[w] .. word_off[w+1]) (int32, device; word_off has n_words + 1
 * entries), 1 .. DH_BEAM_MAX_BAD_LEN ids each, n_words <= DH_BEAM_MAX_BAD_WORDS; a phrase of another length is skipped.  Per row:
 *   1. pos < min_len and 0 <= eos_index < V: logits[eos_index] = -inf;
 *   2. for every phrase w of l ids with l - 1 <= pos and h[pos-l+1 .. pos) == w[0 .. l-1): logits[w[l-1]] = -inf (l == 1: at
 *      every pos).  A last id outside [0, V) is never a column; prefix ids are compared as they are;
 *   3. group_max != NULL: as dh_beam_history_logits' step 3 -- every group holding a column that 1 or 2 stored to is recomputed as
 *      the exact fp32 maximum over its real columns (< V), -inf if they are all -inf; no other group, no other logit is written.
 *      Pass group_max exactly when the sampler that follows reads it.
 * Every store is -inf, so this launch and dh_beam_history_logits commute on the logits and compose on the maxima.
 * pos <= tok_ld (only the last DH_BEAM_MAX_BAD_LEN - 1 tokens are looked at), min_len >= 0; n_words == 0 with pos >= min_len is
 * DH_ERR_BAD_ARG: the caller makes no launch then.  pos is a launch constant, so the call can be captured into a hipGraph. */
int dh_beam_constrain_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                             const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                             const int32_t* first_pos, int eos_index, int min_len, const int32_t* words, const int32_t* word_off,
                             int n_words, void* stream);

/* ---- Biases in front of a row draw: sequence_bias, a finite number added to a token's logit when the token would complete a phrase,
 * IN PLACE on fp32 logits [rows, ldl], one launch, on the row geometry of dh_beam_constrain_logits (history h[0 .. pos) =
 * tokens[r * tok_row_mult, 0 .. pos); first_pos: idle rows untouched).  The list is shared by all rows and is STABLY SORTED BY LAST
 * ID by the caller: phrase w is words[word_off[w] .. word_off[w+1]) (int32, device; n_words + 1 offsets; 1 .. DH_BEAM_MAX_BAD_LEN
 * ids, n_words in 1 .. DH_BEAM_MAX_BAD_WORDS) with bias[w] (fp32, device); run q is the phrases run_off[q] .. run_off[q+1) (int32,
 * device; n_runs + 1 entries): all the phrases of one last id, in the caller's list order.  Per row:
 *   1. for every run, x = logits[last id]; for every phrase w of the run IN ORDER, of l ids with l - 1 <= pos and
 *      h[pos-l+1 .. pos) == w[0 .. l-1) (l == 1: at every pos): x = x + bias[w], each addition one round-to-nearest fp32 add; the
 *      column is stored once if any phrase fired (-inf stays -inf).  A last id outside [0, V) is never a column; prefix ids are
 *      compared as they are; a phrase whose last id is not its run's is skipped;
 *   2. group_max != NULL: as dh_beam_history_logits' step 3 -- every group holding a column that 1 stored to is recomputed as the
 *      exact fp32 maximum over its real columns (< V); no other group, no other logit is written.  Pass group_max exactly when the
 *      sampler that follows reads it.
 * Behind dh_beam_history_logits (the penalty scales the model's logit) and on either side of dh_beam_constrain_logits (-inf + b =
 * -inf).  pos <= tok_ld; an empty list is DH_ERR_BAD_ARG: the caller makes no launch then.  pos is a launch constant, so the call
 * can be captured into a hipGraph. */
int dh_beam_bias_logits(float* logits, int ldl, int V, float* group_max, int gm_ld, int n_groups, int group_cols,
                        const int32_t* tokens, int tok_ld, int tok_row_mult, int pos, int rows, int rows_per_img,
                        const int32_t* first_pos, const int32_t* words, const int32_t* word_off, const float* bias,
                        const int32_t* run_off, int n_words, int n_runs, void* stream);

/* ---- BeamSearchHelper's METHOD surface (deephumor/models/beam.py:32-108), for callers that drive the helper the way the
 * reference's own generate() loops do (rnn_models.py:87-128, transformers.py:532-569): one image, host-driven, tensors of the
 * reference's shapes and dtypes.  The batched engine (dh_beam_row_sample / dh_beam_select above) does not need them. */

/* filter_top_k (beam.py:32-37), IN PLACE like the reference: logits[r, c] = -inf where logits[r, c] < (top_k-th largest of row
 * r) -- strict, ties at the threshold stay -- and at column unk_index.  logits fp32 [rows, ldl]. */
int dh_beam_filter_top_k(float* logits, int ldl, int V, int rows, int top_k, int unk_index, void* stream);

/* sample_k_indices (beam.py:39-48): out[r, 0..k) int64 = torch.multinomial(softmax(x[r] / temperature), k) without replacement
 * == the k largest of p / Exp(1) noise in descending order (ties: lower index).  noise NULL -> Philox keyed by (seed ^
 * *seed_ptr, stream_id, draw, row, index); else [rows, noise_ld] Exp(1) samples.  k <= 64.  err: DH_BEAM_ERR_ALL_FILTERED when a
 * row is all -inf, DH_BEAM_ERR_TOO_FEW when it has fewer than k positive-probability entries (informational: the zero-probability entries
 * follow in index order, as current torch.multinomial returns them in an unspecified order; only the all -inf row is an error). */
int dh_beam_sample_k(const float* x, int ld, int V, int rows, int k, float temperature, const float* noise, int noise_ld,
                     uint64_t seed, const uint64_t* seed_ptr, int stream_id, int draw, int64_t* out, int32_t* err, void* stream);

/* filter_by_indices (beam.py:50-53): out[r, j] = values[r, indices[r, j]] (torch.gather along dim 1); an index outside [0, V)
 * ORs DH_BEAM_ERR_OVERFLOW into err (may be NULL) and gives 0. */
int dh_beam_gather(const float* values, int ld, int V, const int64_t* indices, int k, float* out, int rows, int32_t* err,
                   void* stream);

/* The tail of process_logits (beam.py:78-106): new_val = log_softmax(gathered, -1); a live row contributes `beam` candidates, an
 * ended row ONE with token 0 / score 0 (n_cand = sum over rows); out_ended = ended | (token == eos); prev_seqs / prev_vals =
 * repeat_interleave of seqs [n_rows, seq_len] int64 / vals [n_rows, val_width] by the same counts.  Outputs sized n_cand. */
int dh_beam_expand(const int64_t* new_ind, const float* gathered, const uint8_t* ended, const int64_t* seqs, int seq_len,
                   const float* vals, int val_width, int n_rows, int beam, int eos_index, int64_t* prev_seqs, float* prev_vals,
                   int64_t* out_ind, float* out_val, uint8_t* out_ended, void* stream);

/* Per image: final draw ind ~ softmax(vals/T) (k=1 -> arg-max of p/noise), copies
 * tokens[img*beam+ind, 0..len) to out[img, :] (rest = pad) and writes len, where
 * len = (done ? end_step + len_bias_done : full_len).  rnn_models.py:140-141; transformers.py:576-577.
 *   noise: NULL -> Philox; else [n_img, beam]. */
int dh_beam_finalize(const int32_t* tokens, int tok_ld, const float* vals, const uint8_t* done,
                     const int32_t* end_step, int32_t* out, int out_ld, int32_t* out_len,
                     int n_img, int beam, int len_bias_done, int full_len, int pad_index,
                     float temperature, const float* noise, uint64_t seed, const uint64_t* seed_ptr, int img0,
                     void* stream);

/* dh_beam_finalize that keeps EVERY beam (n-best output): the same final draw (same inputs, Philox counters and noise override:
 * out_drawn names the beam dh_beam_finalize copies) and the same len -> out_row_len [n_img]; the image's beams are then ordered by
 * score, descending and stable (slot = #beams with a larger score + #equal-score beams with a smaller engine index; NaN orders like
 * -inf, so dead beams come last), and for every slot j:  out_tokens [n_img, beam, out_ld] the beam's row copied as above,
 * out_score / out_index [n_img, beam] its cumulative score (vals) and its engine beam index, out_len [n_img, beam] its own length
 * -- up to and including its first eos_index at a column >= the image's first generated column (pos, or first_pos[img] when
 * first_pos is not NULL: prompted batches) and < len, or len without one.  out_drawn [n_img] = the slot of the drawn beam.
 * rnn_models.py:139-141; transformers.py:571-577 (the sample_seq / sample_val the final draw indexes). */
int dh_beam_finalize_beams(const int32_t* tokens, int tok_ld, const float* vals, const uint8_t* done,
                           const int32_t* end_step, int32_t* out_tokens, int out_ld, int32_t* out_len,
                           float* out_score, int32_t* out_index, int32_t* out_drawn, int32_t* out_row_len,
                           int n_img, int beam, int len_bias_done, int full_len, int pad_index, int eos_index,
                           int pos, const int32_t* first_pos, float temperature, const float* noise, uint64_t seed,
                           const uint64_t* seed_ptr, int img0, void* stream);

/* The attention maps of the beams dh_beam_finalize_beams kept, one launch behind it:
 *   out[i, j, c, :] = attn_w[c, src[i * beam + index[i, j], c], :]  for c < len[i, j],  else 0
 * attn_w fp32 [n_pos, rows_total, S] (slab c = decode position c, dh_transformer_decode_position_attn), src the ancestor table
 * [rows_total, src_ld] (src[r, c] = the logical row that computed position c of row r's history), index / len = out_index /
 * out_len [n_img, beam], out fp32 [n_img, beam, T, S] with T <= n_pos, T <= src_ld.  A src entry outside [0, rows_total) gives zeros. */
int dh_beam_gather_attention(const float* attn_w, const int32_t* src, int src_ld, const int32_t* index, const int32_t* len,
                             float* out, int n_img, int beam, int T, int n_pos, int rows_total, int S, void* stream);

/* ---- return_logprobs (not in the reference): the model log-probability of every token a beam holds, in three launches of their own
 * around the select and behind the final draw (csrc/beam_logprobs.hip).  Deterministic: no float atomics, every reduction in a fixed
 * order.
 * dh_beam_pick_logprobs, in front of the select: per row of fp32 logits [rows, ldl] as the row step saw it (behind
 * dh_beam_history_logits / dh_beam_constrain_logits, in front of any top-k / nucleus / unk filtering)
 *   pick_lp[r, j] = x[r, pick_idx[r, j]] / temperature - logsumexp(x[r, 0 .. V) / temperature),   j < beam
 * with dh_beam_row_best's sweep (one pass, 16-byte loads) and its exact division.  A row whose `ended` flag is set -- ended [rows_total]
 * is read at the row's beam-state row: r * beam for rows_per_img == 1 (the dense first step's compact rows), r otherwise -- gets
 * zeros; so does a row that holds NaN or +inf or nothing finite (the row step flags those), and a pick outside [0, V).
 * from_vals != 0 (search="beam"): no sweep, pick_lp = pick_val bit for bit under the same `ended` mask (logits, pick_idx unused).
 * first_pos != NULL ([rows / beam] int32, rows_per_img == beam): the prompted phases as in dh_beam_row_best. */
int dh_beam_pick_logprobs(const float* logits, int ldl, int V, int rows, int rows_per_img, int beam, float temperature, int step,
                          const int32_t* first_pos, const uint8_t* ended, const int32_t* pick_idx, const float* pick_val,
                          int from_vals, float* pick_lp, void* stream);

/* Behind the select of position step_index: slab c = step_index of two position-major tables [n_pos, n_img * beam] that the caller
 * filled once with 0 (lp_w, fp32) and with every row's own index (par_w, int32).  Per beam row of an image that took the step:
 *   par_w[c, row] = parent[row];   lp_w[c, row] = pick_lp[prow, j] for the first j with pick_idx[prow, j] == tokens[row, write_pos],
 * 0 without one; prow = parent[row], at a first step the image's compact row img (first_pos == NULL and first != 0) or its base row
 * img * beam (first_pos[img] == step_index).  An image that took no step -- step_index < first_pos[img], or done[img] with
 * end_step[img] < step_index -- writes nothing.  write_pos >= tok_ld (a step that re-draws the beams and writes no column): parents
 * only. */
int dh_beam_record_logprobs(const int32_t* tokens, int tok_ld, const int32_t* parent, const uint8_t* done, const int32_t* end_step,
                            const int32_t* pick_idx, const float* pick_lp, int n_img, int beam, int first,
                            const int32_t* first_pos, int write_pos, int step_index, int n_pos, float* lp_w, int32_t* par_w,
                            void* stream);

/* Behind dh_beam_finalize_beams (index / len = its out_index / out_len [n_img, beam]): per kept beam, from r = i * beam + index[i, j]
 * and from slab n_pos - 1 down to 0,
 *   out[i, j, c] = lp_w[c, r]  for p0 <= c < len[i, j]  (p0 = first_pos[i], or pos without first_pos),   then r = par_w[c, r]
 * and 0 in every other element of out fp32 [n_img, beam, T], T <= n_pos.  A par_w entry outside the table's rows is not followed. */
int dh_beam_gather_logprobs(const float* lp_w, const int32_t* par_w, const int32_t* index, const int32_t* len, int n_img, int beam,
                            int T, int n_pos, int pos, const int32_t* first_pos, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Teacher-forced scoring (deephumor/experiments/metrics.py:4-9; call shape trainer.py:69-81)
 * ------------------------------------------------------------------------------------------- */

/* logp[r] = log_softmax(logits[r, 0..V))[targets[r]]; logits fp32 [rows, ldl]; targets int64 [rows]. */
int dh_token_logprob(const float* logits, int ldl, int V, const int64_t* targets, float* logp, int rows,
                     void* stream);

/* pp[b] = exp(-sum_t [targets[b,t] != pad_index] * logp[b,t] / lengths[b]); logp/targets [n_seq, L]. */
int dh_seq_perplexity(const float* logp, const int64_t* targets, const int64_t* lengths, float* pp,
                      int n_seq, int L, int pad_index, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Native step drivers: one call = every kernel of one decode position / one LSTM time step,
 * sequenced on `stream` from weights described by plain C structs (host arrays of device pointers).
 * Replaces the Python-side per-layer loops of TransformerDecoder.forward (transformers.py:455-488,
 * KV-cached form) and of one nn.LSTM step + classifier (rnn_models.py:107-109).
 * ------------------------------------------------------------------------------------------- */
typedef struct dh_tr_layer {
    const void *wqkv, *wo, *w1, *w2, *wq, *weo;            /* [3D,D] [D,D] [PF,D] [D,PF] [D,D] [D,D], storage dtype */
    const float *bqkv, *bo, *b1, *b2, *bq, *beo;           /* fp32 biases */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
    float ln1_eps, ln2_eps, ln3_eps, sa_scale, ea_scale;
    int _pad;
    void *kcache, *vcache;                                  /* this layer's self-attention cache [pos][rows_total][D] */
    const void* kv;                                         /* this layer's cross-attention K|V [n_img*S][2D] or NULL */
    /* optional (16-bit dtypes): the deferred-LayerNorm chain (dh_linear_ln).  Weights with the gamma of the LayerNorm in
     * FRONT of them folded in, biases with its beta folded in, row sums of the folded weights:
     *   wqkv_f / bqkv_f / cs_qkv : LN3 of the PREVIOUS layer (NULL for layer 0, whose input is the embedding)
     *   wq_f / bq_f / cs_q       : LN1 of this layer (cross-attention query projection)
     *   w1_f / b1_f / cs_1       : the LayerNorm in front of the FFN (LN2; LN1 in the decoder without encoder attention)
     * w1_f == NULL selects the plain chain with dh_add_layernorm launches. */
    const void *wqkv_f, *wq_f, *w1_f;
    const float *bqkv_f, *bq_f, *b1_f, *cs_qkv, *cs_q, *cs_1;
    const void *kp, *vt;                                    /* optional: kv re-laid out by dh_attn_cross_pack (matrix-core cross-attention) */
    int kp_dperm, _pad2;                                    /* kp was packed with dperm = 1: the chain fuses fc_q into the attention launch */
    /* optional: dh_pack_mfma_fragments of (wqkv_f, or wqkv for layer 0), wo, weo, w1_f, w2 -- the register-stationary decode GEMMs
     * (dh_linear_ln_wreg) for positions with many rows; NULL = the tile kernels */
    const void *wqkv_pk, *wo_pk, *weo_pk, *w1_pk, *w2_pk;
    const void* wq_pk;                                      /* optional: dh_pack_mfma_fragments(wq_f): fc_q as its own register-stationary GEMM in front of the packed cross-attention */
    /* optional (DH_F32 models, option "f32_split"): dh_split_f32x planes of wqkv, wo, w1, w2, wq, weo -- the dense layers of a
     * position then run as three fp16 MFMAs on split operands (dh_linear_f32x) instead of v_mfma_f32_32x32x2_f32; NULL = fp32 MFMA */
    const void *wqkv_x, *wo_x, *w1_x, *w2_x, *wq_x, *weo_x;
    /* optional, next to the planes: both planes through dh_pack_mfma_fragments ([2][K / 32][N / 16][64] x 16 bytes) -- the dense layers of a
     * decode position then run on dh_linear_f32x_wreg (weights stationary in registers; bit-identical to dh_linear_f32x) */
    const void *wqkv_xp, *wo_xp, *w1_xp, *w2_xp, *wq_xp, *weo_xp;
} dh_tr_layer_t;

typedef struct dh_tr_model {
    int n_layers, D, n_heads, pf_dim, V, pad_index, cross, S, dtype;
    float emb_scale;
    const dh_tr_layer_t* layers;                            /* host array [n_layers] */
    const void *tok_emb, *pos_emb, *cls_w;
    const float* cls_b;
    const uint8_t* keymask;                                 /* [n_img*S] or NULL */
    const void* cls_w_pk; const float* cls_b_pad;           /* optional: the operands of dh_vocab_logits_wreg (padded, fragment-packed classifier) */
    const void* cls_w_x;                                    /* optional (DH_F32): dh_split_f32x planes of cls_w */
} dh_tr_model_t;

typedef struct dh_tr_scratch {
    void *x, *qkv, *att, *o, *q, *ff;       /* [rows, D|3D|D|D|D|PF] */
    void* y2;                               /* [rows, D]      second pre-LayerNorm row buffer of the deferred chain (or NULL) */
    float *st0, *st1, *st2;                 /* [rows, D/64, 2] partial LayerNorm statistics of x / o / y2 (or NULL) */
    void *xp, *attp, *ffp;                  /* optional (DH_F32, options "f32_split" + "f32_planes"): fp16 planes [2][rows][D | D | PF] of x /
                                               att / ff -- the GEMM operands of the position stored split by their producers; with them
                                               (and the layers' *_xp weights) the position runs on dh_linear_f32xp_wreg / dh_linear_f32xp */
} dh_tr_scratch_t;

/* Hidden state of position t for n_img*rows_per_img compact rows; x_out (optional, [rows,D]) receives the
 * last layer's output instead of scratch->x; logits (optional, fp32 [rows,V], row stride ldl) = classifier(x); with
 * group_max != NULL (bf16 only) the classifier is dh_vocab_logits. */
int dh_transformer_decode_position(const dh_tr_model_t* m, const dh_tr_scratch_t* sc,
                                   const void* start_emb, const int32_t* tokens, int tok_ld,
                                   const int32_t* src, int src_ld, int n_img, int rows_per_img,
                                   int row_mult, int rows_total, int t, void* x_out, float* logits, int ldl,
                                   float* group_max, int gm_ld, void* stream);

/* dh_transformer_decode_position that also keeps the encoder-attention weights of layer attn_layer: right after that layer's fc_q
 * GEMM (on each of the three chains) one launch of dh_attn_cross_weights writes slab t of attn_w [n_pos, rows_total, S] at the rows'
 * logical slots.  A new entry point, not new fields of dh_tr_model_t: no existing prototype or struct changed, so the ABI version
 * stayed. */
int dh_transformer_decode_position_attn(const dh_tr_model_t* m, const dh_tr_scratch_t* sc,
                                        const void* start_emb, const int32_t* tokens, int tok_ld,
                                        const int32_t* src, int src_ld, int n_img, int rows_per_img,
                                        int row_mult, int rows_total, int t, void* x_out, float* logits, int ldl,
                                        float* group_max, int gm_ld, float* attn_w, int attn_layer, void* stream);

typedef struct dh_lstm_layer {
    const void* w; const float* b;          /* [4Hh, in+Hh] = [W_ih|W_hh], b_ih+b_hh (PyTorch gate order i,f,g,o) */
    const void* w_il; const float* b_il;    /* optional (bf16): the same, gate-interleaved: row 4u+g = gate g of unit u */
    const void* w_pk;                       /* optional: dh_pack_mfma_fragments(w_il) -- the register-stationary step (dh_lstm_layer_wreg) */
    const void* w_x;                        /* optional (DH_F32): dh_split_f32x planes of w -- the gate GEMM as dh_linear_f32x */
    const void* w_xp;                       /* optional: those planes fragment-packed -- the gate GEMM as dh_linear_f32x_wreg */
} dh_lstm_layer_t;

typedef struct dh_lstm_model {
    int n_layers, E, Hh, V, dtype, _pad;
    const dh_lstm_layer_t* layers;                          /* host array [n_layers] */
    const void *emb, *cls_w;
    const float* cls_b;
    void* h;                                                /* recurrent state [n_layers, rows_total, Hh], storage dtype */
    float* c;                                               /* cell state, fp32 */
    void* h_alt; float* c_alt;                              /* optional second state buffers (fused bf16 step: ping-pong) */
    const void* cls_w_pk; const float* cls_b_pad;           /* optional: the operands of dh_vocab_logits_wreg */
    const void* cls_w_x;                                    /* optional (DH_F32): dh_split_f32x planes of cls_w */
} dh_lstm_model_t;

typedef struct dh_lstm_scratch {
    void *xcat0, *xcatl; float *c_cur, *gates; void* hout;
    void* topp;                             /* optional (DH_F32, option "f32_split"): fp16 planes [2][rows][Hh] of the top layer's state: the
                                               classifier then runs on dh_linear_f32xp and fills group_max */
    void *xcat0p, *xcatlp;                  /* optional, with topp: planes [2][rows][E + Hh] and [n_layers - 1][2][rows][2 Hh] of the gate
                                               GEMMs' operands (option "f32_planes": dh_lstm_prepare_f32x / dh_lstm_cell_f32x write them,
                                               dh_linear_f32xp_wreg reads them) */
} dh_lstm_scratch_t;

/* One LSTM layer time step in one launch (bf16): gates = [x | h_prev[parent]] * w_il^T + b_il on the matrix cores,
 * cell update in the epilogue.  x row of compact row m: emb[tokens[m*row_mult*tok_ld + tok_pos]] if tokens, else
 * x_rows[(m / x_div) * ldx].  h_prev / c_prev (NULL = zero state) are gathered through hparent (NULL = identity)
 * at logical row m*row_mult; h_next / c_next (different buffers) are written at the logical row, h_out at row m. */
int dh_lstm_layer_fused(const void* x_rows, int ldx, int x_div, const void* emb, const int32_t* tokens, int tok_ld,
                        int tok_pos, const void* h_prev, const float* c_prev, const int32_t* hparent, void* h_next,
                        float* c_next, void* h_out, int ld_out, const void* w_il, const float* b_il, int rows,
                        int row_mult, int E, int Hh, int dtype, void* stream);

/* The same step with the gate weights stationary in registers (decode shapes: E + Hh = 768 or 1024, E % 64 == 0, Hh % 32 == 0):
 * a workgroup owns 128 gate rows x 80 activation rows, its waves load their weight fragments straight from L2 out of
 * w_packed = dh_pack_mfma_fragments(w_il [4 Hh, E + Hh]); only the activation block crosses LDS.  Same arguments and results
 * (bit-identical) as dh_lstm_layer_fused; the outputs are stored 16 bytes per lane: h_next, c_next and h_out 16-byte aligned,
 * ld_out % 8 == 0. */
int dh_lstm_layer_wreg_supported(int E, int Hh);
int dh_lstm_layer_wreg(const void* x_rows, int ldx, int x_div, const void* emb, const int32_t* tokens, int tok_ld,
                       int tok_pos, const void* h_prev, const float* c_prev, const int32_t* hparent, void* h_next,
                       float* c_next, void* h_out, int ld_out, const void* w_packed, const float* b_il, int rows,
                       int row_mult, int E, int Hh, int dtype, void* stream);

/* One LSTM time step for `rows` compact rows and, if logits != NULL, the classifier.  h_out (optional, row stride
 * ld_out) receives the top layer's h instead of scratch->hout.
 *   started == 0: zero initial state; the new state is written to m->h / m->c.
 *   fp32, or bf16 without w_il / h_alt: dh_lstm_prepare + per layer gate GEMM + dh_lstm_cell, state updated in place
 *     (any started != 0 reads m->h / m->c).
 *   bf16 with w_il, b_il, h_alt, c_alt: one dh_lstm_layer_fused launch per layer; started == 1 reads m->h / m->c and
 *     writes h_alt / c_alt, started == 2 the reverse -- the caller alternates 0, 1, 2, 1, 2, ... */
int dh_lstm_decode_step(const dh_lstm_model_t* m, const dh_lstm_scratch_t* sc, const void* img_emb,
                        const int32_t* tokens, int tok_ld, int tok_pos, const int32_t* hparent,
                        int started, int rows, int rows_per_img, int row_mult, int rows_total,
                        void* h_out, int ld_out, float* logits, int ldl, float* group_max, int gm_ld,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 models on the 16-bit matrix cores ("f32x", csrc/gemm_f32x.hip; option "f32_split").  Every fp32 operand x is used as
 * x = hi + lo * 2^-11 with hi = fp16(x), lo = fp16((x - hi) * 2^11); a product sum is three v_mfma_f32_16x16x32_f16 (hi*hi,
 * hi*lo, lo*hi; every fp16 product is exact in fp32) with fp32 accumulation -- fp32-class results (the dropped lo*lo term is
 * 2^-22 relative) at a multiple of the rate of v_mfma_f32_32x32x2_f32 / the vector ALUs.  Replaces the same torch call sites as
 * dh_linear (nn.Linear: encoders.py:61,67; rnn_models.py:45 + the LSTM gate products; transformers.py:97-99,127,162-163,489)
 * and dh_conv2d_bn_act (the torchvision trunk, encoders.py:56) for fp32 tensors.  Range: weights are checked when a plan is built;
 * an ACTIVATION with |x| >= 65504 (hi = inf: the results would hold inf / NaN) sets a sticky per-stream word that
 * dh_f32x_take_overflow hands over and resets -- the Python layer reads it where it synchronises anyway and repeats the call on the
 * exact-fp32 kernels (dh_linear / dh_conv2d_bn_act with DH_F32).
 *   dh_split_f32x      w fp32 [N, ldw] -> planes [2][N][Kp] fp16 (hi plane, then lo * 2^11), Kp = K rounded up to 32, zero padded;
 *                      made once per weight version
 *   dh_linear_f32x     C [M, ldc] fp32 = act(((A W^T + bias) * scale + shift) + residual); A fp32 [M, lda] (lda % 4 == 0, K % 4 == 0),
 *                      bias / scale+shift / residual optional
 *   dh_conv2d_nhwc_f32x  channels-last fp32 convolution + BatchNorm scale / shift (+ residual) (+ ReLU): x [N,H,W,Cin] (Cin % 4 == 0),
 *                      planes of w [Cout][KS][KS][Cin], y / residual [N,Ho,Wo,Cout]
 *   dh_nchw_to_nhwc_f32  [N,C,H,W] -> [N,H,W,Cp] (channels >= C zero): the stem's input
 *   dh_f32x_take_overflow  *dst (device uint32) = 1 if a launch of the two kernels above on `stream` split an out-of-range activation
 *                      since the last call, else 0; resets the stream's word
 *   dh_maxpool3x3s2_nhwc_f32, dh_avgpool_nhwc_f32   MaxPool2d(3, 2, 1) / AdaptiveAvgPool2d(1) on channels-last fp32 tensors
 * ------------------------------------------------------------------------------------------- */
int dh_split_f32x(const float* w, int ldw, void* planes, int N, int K, int Kp, void* stream);
int dh_f32x_take_overflow(uint32_t* dst, void* stream);
/* dh_linear_f32x for the rows of ONE decode position with the weights stationary in registers (csrc/linear_f32x_wreg.hip; the fp32
 * counterpart of dh_linear_ln_wreg): w_packed = the hi plane, then the lo plane of dh_split_f32x(W [N, K]), each through
 * dh_pack_mfma_fragments ([2][K / 32][N / 16][64] x 16 bytes).  C = act(A W^T + bias (+ residual)), bit-identical to dh_linear_f32x.
 * _supported: N % 64 == 0, K % 512 == 0 or K % 384 == 0, M <= 8,192. */
int dh_linear_f32x_wreg_supported(int M, int N, int K);
int dh_linear_f32x_wreg(const float* A, int lda, const void* w_packed, const float* bias, const float* residual, int ldres,
                        float* C, int ldc, int M, int N, int K, int relu, void* stream);
/* dh_linear_f32x_wreg for an activation stored as planes (a_planes [2][M][K], K = the row stride): no split pass in front of the MFMAs; the
 * result as fp32 (C) and / or planes (c_planes [2][M][N]) -- either may be NULL.  dh_add_layernorm_f32x = dh_add_layernorm on fp32 rows
 * with the result stored both ways (out fp32 = the next residual, out_planes = the next GEMM operand). */
int dh_linear_f32xp_wreg(const void* a_planes, const void* w_packed, const float* bias, const float* residual, int ldres,
                         float* C, int ldc, void* c_planes, int M, int N, int K, int relu, void* stream);
int dh_add_layernorm_f32x(const float* x, const float* y, const float* gamma, const float* beta, float* out, void* out_planes,
                          int rows, int D, float eps, void* stream);
int dh_linear_f32x(const float* A, int lda, const void* w_planes, int Kp, const float* bias, const float* scale, const float* shift,
                   const float* residual, int ldres, float* C, int ldc, int M, int N, int K, int relu, void* stream);
int dh_conv2d_nhwc_f32x(const float* x, const void* w_planes, int Kp, const float* scale, const float* shift, const float* residual,
                        float* y, int N, int H, int W, int Cin, int Cout, int KS, int stride, int pad, int relu, void* stream);
int dh_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int H, int W, int Cp, void* stream);
/* The wide 1 x 1 / stride 1 layers of the fp32 trunk (Bottleneck.conv3 + bn3 + identity + relu, layer1's downsample; encoders.py:56) as a
 * persistent streaming kernel (csrc/conv1x1_f32x.hip): weights stationary in registers (w_packed = both planes of dh_split_f32x(w [Cout,
 * Cin]) through dh_pack_mfma_fragments), 32-row activation blocks double-buffered by LDS-DMA, the residual prefetched, the column
 * groups of a row block on one XCD.  x [M, Cin], y / residual [M, Cout] channels-last fp32; bit-identical to dh_conv2d_nhwc_f32x.
 * _supported: Cin = 64 / 128 / 256, Cout = 128 ... 1,024 in steps that divide an XCD's workgroups, M large enough for the grid. */
int dh_conv1x1_f32x_stream_supported(int M, int Cin, int Cout);
int dh_conv1x1_f32x_stream(const float* x, const void* w_packed, const float* scale, const float* shift, const float* residual,
                           float* y, int M, int Cin, int Cout, int relu, void* stream);
/* The same arithmetic on activations STORED split (csrc/gemm_f32xp.hip): a tensor whose only consumers are GEMM operands is kept as the
 * two fp16 planes [2][rows][K] its consumer would make of it (4 bytes per element, the same numbers), so both operands go global ->
 * LDS by DMA, three slabs deep, with no split work in the loop.  Bit-identical to dh_linear_f32x on the same values.
 *   dh_split_act_f32x        A fp32 [M, lda] -> planes [2][M][Kp] (zero padded to Kp = K rounded up to 32); range-guarded like the kernels
 *   dh_linear_f32xp          a_planes [2][M][Kp] x w_planes [2][N][Kp] -> C fp32 [M, ldc] and / or c_planes [2][M][N] (N % 4 == 0), either
 *                            NULL; group_max (optional) [M, gm_ld]: the maxima of the 64-column groups of the stored values -- what
 *                            dh_vocab_logits hands dh_beam_row_sample_groups on the 16-bit paths */
int dh_split_act_f32x(const float* A, int lda, void* planes, int M, int K, int Kp, void* stream);
/* The trunk's 3 x 3 layers of stages 2 - 4 on planes: dh_conv2d_nhwc_f32x_planes_out = dh_conv2d_nhwc_f32x (Bottleneck.conv1) with the result
 * stored as planes [2][N,Ho,Wo,Cout] instead of fp32; dh_conv2d_nhwc_f32xp = the convolution (Bottleneck.conv2) of x_planes [2][N,H,W,Cin]
 * (Cin % 32 == 0) through the planes kernel -> y fp32 and / or y_planes.  Bit-identical to dh_conv2d_nhwc_f32x on the same values. */
int dh_conv2d_nhwc_f32x_planes_out(const float* x, const void* w_planes, int Kp, const float* scale, const float* shift, void* y_planes,
                                   int N, int H, int W, int Cin, int Cout, int KS, int stride, int pad, int relu, void* stream);
int dh_conv2d_nhwc_f32xp(const void* x_planes, const void* w_planes, const float* scale, const float* shift, const float* residual,
                         float* y, void* y_planes, int N, int H, int W, int Cin, int Cout, int KS, int stride, int pad, int relu,
                         void* stream);
int dh_linear_f32xp(const void* a_planes, const void* w_planes, int Kp, const float* bias, const float* scale, const float* shift,
                    const float* residual, int ldres, float* C, int ldc, void* c_planes, float* group_max, int gm_ld, int M, int N,
                    int relu, void* stream);
int dh_maxpool3x3s2_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
int dh_avgpool_nhwc_f32(const float* x, float* y, int N, int HW, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Launch profiler (measurement infrastructure, not on the data path): while enabled, every launch made
 * through this library is bracketed by HIP events on its stream.  Launches are keyed "entry[role]{MxNxK}" (role: qkv /
 * proj / ffn / vocab / 1x1 / 3x3 ...; the shape suffix for GEMM-shaped launches).  filter: NULL/"" = everything, else
 * comma-separated full keys, "entry[role]" prefixes or bare entry-point names.  dh_prof_end() synchronises the recorded
 * events and aggregates per key: calls, total ms, algorithmic flops and bytes.  The recorder is mutex-protected (launches
 * may come from several host threads / streams); the kernels' data path is unaffected.
 * ------------------------------------------------------------------------------------------- */
int dh_prof_begin(const char* filter);
int dh_prof_set_stride(int n);           /* record only every n-th matching launch (default 1): sampling keeps
                                            the perturbation of a timed region small */
int dh_prof_end(void);
int dh_prof_num(void);
int dh_prof_get(int i, char* name, int cap, int* calls, double* ms, double* flops, double* bytes);
void dh_prof_tag(const char* tag);

/* ---------------------------------------------------------------------------------------------
 * Run-time options: every switch that selects between (results-identical) kernels or tile shapes, and the one that
 * selects the arithmetic of fp32 models ("f32_split"), lives in ONE table.  An option's default comes from its
 * environment variable (read once, at the option's first use) or, when that is unset, from the built-in default;
 * dh_set_option overrides it from then on and takes effect at the next call of any entry point (nothing is latched).
 * Weight plans the Python layer has already built keep the kernels they were built for (deephumor_amd.hip.set_option
 * documents which options are plan-time).  Process-global, not thread-safe against concurrent launches.
 *   dh_option_count()              number of options
 *   dh_option_name(i)              "key" of option i (NULL when out of range); dh_option_env(i) its environment variable
 *   dh_get_option(key, &value)     DH_ERR_BAD_ARG for an unknown key
 *   dh_set_option(key, value)
 * ------------------------------------------------------------------------------------------- */
int dh_option_count(void);
const char* dh_option_name(int i);
const char* dh_option_env(int i);
int dh_get_option(const char* key, int* value);
int dh_set_option(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* DEEPHUMOR_HIP_H */
