"""Image / label encoders on the gfx950 kernels.

Drop-in for ``deephumor.models.encoders`` (reference encoders.py:7-144): same class names,
constructor arguments, ``forward`` signatures and state-dict keys.  The modules below are
parameter containers -- the arithmetic runs in ``libdeephumor_hip.so`` (``deephumor_amd.hip``),
batched over images.  Inference only: like the reference's ``generate`` callers
(deephumor_demo.ipynb:1134-1141) the model must be in ``eval()`` mode.
"""
from collections import namedtuple

import torch
from torch import nn

from .. import hip
from ._f32x_guard import f32x_guarded
from .. import f32xp

RESNET50_STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def _require_eval(module, p):
    if module.training and p > 0:
        raise RuntimeError("deephumor_amd implements the inference path (eval mode); "
                           "call model.eval() -- train-mode dropout is out of scope")


class _Bottleneck(nn.Module):
    """Parameter holder with torchvision's Bottleneck attribute names (conv1..bn3, downsample)."""

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))
        else:
            self.downsample = None
        self.stride = stride


def _resnet50_trunk():
    """Children 0..7 of the reference's ``self.resnet`` (encoders.py:37-38): conv1, bn1, relu,
    maxpool, layer1..layer4 -- the 318 trunk tensors of the state dict."""
    mods = [nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64),
            nn.ReLU(inplace=True), nn.MaxPool2d(3, stride=2, padding=1)]
    inplanes = 64
    for planes, blocks, stride in RESNET50_STAGES:
        stage = [_Bottleneck(inplanes, planes, stride, downsample=True)]
        inplanes = planes * 4
        stage += [_Bottleneck(inplanes, planes, 1, downsample=False) for _ in range(1, blocks)]
        mods.append(nn.Sequential(*stage))
    return nn.Sequential(*mods)


def _bn_affine(bn):
    """Eval-mode BatchNorm as y = x*scale + shift (applied in the kernel epilogue, weights untouched)."""
    scale = (bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)).contiguous()
    shift = (bn.bias.detach().float() - bn.running_mean.detach().float() * scale).contiguous()
    return scale, shift


class _Planned:
    """Lazily derived device-side constants, rebuilt when any parameter/buffer changes (storage pointer or in-place
    version counter).  The tensor list is cached -- walking a ResNet-50's modules costs more host time per call than
    the key itself -- and dropped whenever the module is converted or (re)loaded (``_apply``: ``.to`` / ``.cuda`` /
    ``.bfloat16``; ``load_state_dict``), the two ways standard PyTorch code replaces parameter or buffer objects."""

    def _plan_tensors_list(self, refresh=False):
        ts = self.__dict__.get("_plan_tensors")
        if ts is None or refresh:
            ts = list(self.parameters()) + list(self.buffers())
            object.__setattr__(self, "_plan_tensors", ts)
        return ts

    def _plan_key(self, refresh=False):
        ts = self._plan_tensors_list(refresh)
        return tuple(t.data_ptr() for t in ts), tuple(t._version for t in ts), hip.options_epoch

    def _drop_plan(self):
        for m in self.modules():
            if isinstance(m, _Planned):
                m.__dict__.pop("_plan_tensors", None)
                m.__dict__.pop("_plan_cache", None)

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._drop_plan()
        return out

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self._drop_plan()
        return out

    def _get_plan(self):
        key = self._plan_key()
        if self.__dict__.get("_plan_cache") is None or self._plan_cache[0] != key:
            key = self._plan_key(refresh=True)            # something changed: re-walk the modules, then rebuild
            object.__setattr__(self, "_plan_cache", (key, self._build_plan()))
        return self._plan_cache[1]


# One bottleneck of the 16-bit trunk's schedule: the kernel of each convolution, by its ``hip`` function's name -- conv1 None when the
# previous launch computed it; a fused tail is named as both conv2 and conv3; conv3 of a stage's first block includes the downsample
# (the dual GEMM) -- and whether this launch also computes the next bottleneck's conv1 (``fuse``).
Step = namedtuple("Step", "conv1 conv2 conv3 fuse")

TILE = "conv2d_nhwc_bn_act"          # the implicit-GEMM tile kernel: every convolution's reference point


def _schedule(bottlenecks, shape, packed, level):
    """The kernels of the 16-bit trunk for images of ``shape`` (``packed``: [N, H, W, 8], else [N, 3, H, W]) at option
    ``encoder_generic`` = ``level``: ``(stem kernel, [Step per bottleneck])``.  It reads shapes only -- the weights' channel counts and
    strides, the input size -- and the host-side ``hip.*_supported`` predicates, so it runs without a GPU.  Every specialised kernel's
    condition is here, once; level >= 1 switches off the register-streamed kernels (conv1x1_wreg, conv1x1_dual_wreg, conv3x3_s4, the
    stage-1 / 2 tails) and every conv1 fusion, >= 2 also the stage-3 tail, the ring tail and conv3x3_direct (each of them bit-identical
    to the tile kernel), >= 3 also the one-launch stems (another summation order: close, not bit-equal)."""
    n, h, w = (shape[0], shape[1], shape[2]) if packed else (shape[0], shape[2], shape[3])
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1                  # the stem convolution (7 x 7, stride 2, pad 3)
    if level >= 3 or ho % 2 or wo % 2:
        stem = TILE                                              # + maxpool3x3s2_nhwc
    elif h >= 2 and w >= 2:
        stem = "stem_conv7_bn_relu_maxpool"
    else:
        stem = "conv2d_nhwc_bn_relu_maxpool"
    h, w = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1                   # the max-pool (3 x 3, stride 2, pad 1)
    steps = []
    for i, b in enumerate(bottlenecks):
        nxt = bottlenecks[i + 1] if i + 1 < len(bottlenecks) else None
        n1 = nxt.conv1.weight.shape[0] if nxt is not None and nxt.downsample is None else 0      # a conv1 this block's launch may fuse
        cin, c, s = b.conv1.weight.shape[1], b.conv2.weight.shape[0], b.conv2.stride[0]
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        if steps and steps[-1].fuse:
            conv1 = None
        else:
            conv1 = "conv1x1_wreg_nhwc" if level < 1 and hip.conv1x1_wreg_supported(n * h * w, cin, c) else TILE
        if b.downsample is None and level < 1 and n1 and hip.bottleneck_tail_s1_supported(h, w, c, n1):
            # stage 1 (56 x 56 x 64): 4-row strips, weights register-streamed, and the next block's conv1 on the output tile while it is
            # in LDS -- the 411 MB tensor is not read back for it (conv_s1.hip; without the fusion the ring tail is the faster one)
            steps.append(Step(conv1, "bottleneck_tail_s1_nhwc", "bottleneck_tail_s1_nhwc", True))
        elif b.downsample is None and level < 2 and hip.bottleneck_tail_s3_supported(h, w, c):
            # stage 3 (14 x 14 x 256): one image per workgroup, patch-resident 3x3 + 1x1 expansion, weights register-streamed
            steps.append(Step(conv1, "bottleneck_tail_s3_nhwc", "bottleneck_tail_s3_nhwc", False))
        elif b.downsample is None and level < 1 and hip.bottleneck_tail_s2_supported(h, w, c):
            # stage 2 (28 x 28 x 128), three workgroups per CU (conv_s2.hip); + the next block's conv1 (512 -> 128) on the output
            # chunks in LDS: 170 us against 135 + 55 us
            steps.append(Step(conv1, "bottleneck_tail_s2_nhwc", "bottleneck_tail_s2_nhwc", n1 > 0))
        elif b.downsample is None and level < 2 and hip.conv3x3_direct_supported(h, w, c, c):
            # the ring tail: conv2 + bn2 + relu + conv3 + bn3 + residual + relu in one launch, the conv2 output tile stays in LDS
            steps.append(Step(conv1, "bottleneck_tail_nhwc", "bottleneck_tail_nhwc", False))
        else:
            if b.downsample is None and level < 1 and hip.conv3x3_s4_supported(h, w, c):
                conv2 = "conv3x3_s4_nhwc"        # stage 4: two images x half of the channels per workgroup, weights register-streamed
            elif s == 1 and level < 2 and hip.conv3x3_direct_supported(h, w, c, c):
                conv2 = "conv3x3_direct_nhwc"    # patch-resident direct convolution (stages 1-2)
            else:
                conv2 = TILE
            fuse = False
            if b.downsample is not None:
                # conv3 + downsample as one GEMM (the dual); stage 1's also runs the next block's conv1 (its 256 outputs are in the workgroup)
                k, cout = b.conv3.weight.shape[1] + b.downsample[0].weight.shape[1], b.conv3.weight.shape[0]
                if level < 1 and hip.conv1x1_dual_wreg_supported((n, ho, wo, c), (n, h, w, cin), cout):
                    conv3, fuse = "conv1x1_dual_wreg_nhwc", (k, cout, n1) == (128, 256, 64)
                else:
                    conv3 = "conv1x1_dual_nhwc"
            elif level < 1 and c == 512 and hip.conv1x1_wreg_supported(n * h * w, c, b.conv3.weight.shape[0]):
                conv3 = "conv1x1_wreg_nhwc"          # stage 4's conv3 + residual (the kernel's residual form takes Cin = 512)
            else:
                conv3 = TILE
            steps.append(Step(conv1, conv2, conv3, fuse))
        h, w = ho, wo
    return stem, steps


def _conv_launch(name, c):
    """f(x, residual=None): convolution ``c`` of a plan on the kernel ``name``."""
    if name == "conv1x1_wreg_nhwc":
        # weights stationary in registers, pixels streamed (csrc/conv1x1_wreg.hip)
        return lambda x, r=None: hip.conv1x1_wreg_nhwc(x, c["pk"], c["w"].shape[0], c["scale"], c["shift"], relu=c["relu"], residual=r)
    if name == "conv3x3_s4_nhwc":
        return lambda x, r=None: hip.conv3x3_s4_nhwc(x, c["pk"], c["scale"], c["shift"])
    if name == "conv3x3_direct_nhwc":
        return lambda x, r=None: hip.conv3x3_direct_nhwc(x, c["w"], c["scale"], c["shift"])
    assert name == TILE, name
    return lambda x, r=None: hip.conv2d_nhwc_bn_act(x, c["w"], c["scale"], c["shift"], residual=r, relu=c["relu"], stride=c["stride"],
                                                    pad=c["pad"])


def _block_launch(blk, n1, step):
    """step(x, y1_ready) -> (x, y1_for_next_block): bottleneck ``blk`` of a plan on the kernels of ``step`` (``n1``: the next block's
    conv1 when ``step.fuse``)."""
    c1, c2, c3, d = blk["c1"], blk["c2"], blk["c3"], blk["dual"]
    conv1 = (lambda x, ready: ready) if step.conv1 is None else (lambda x, ready, f=_conv_launch(step.conv1, c1): f(x))
    nxt = dict(w1p=n1["pk"], scale1=n1["scale"], shift1=n1["shift"], n1=n1["w"].shape[0]) if step.fuse else {}
    done = (lambda r: r) if step.fuse else (lambda r: (r, None))                # the fused launches return (out, y1_next)
    if step.conv2 == "bottleneck_tail_nhwc":
        return lambda x, ready: (hip.bottleneck_tail_nhwc(conv1(x, ready), c2["w"], c2["scale"], c2["shift"], c3["w"], c3["scale"],
                                                          c3["shift"], x), None)
    if step.conv2 in ("bottleneck_tail_s1_nhwc", "bottleneck_tail_s2_nhwc", "bottleneck_tail_s3_nhwc"):      # weights register-streamed
        tail = getattr(hip, step.conv2)
        return lambda x, ready: done(tail(conv1(x, ready), c2["pk"], c2["scale"], c2["shift"], c3["pk"], c3["scale"], c3["shift"], x,
                                          **nxt))
    conv2 = _conv_launch(step.conv2, c2)
    if step.conv3 == "conv1x1_dual_wreg_nhwc":
        end = lambda y, x: done(hip.conv1x1_dual_wreg_nhwc(y, x, d["pk"], d["w"].shape[0], d["shift"], d["stride"], relu=True, **nxt))
    elif step.conv3 == "conv1x1_dual_nhwc":
        end = lambda y, x: (hip.conv1x1_dual_nhwc(y, x, d["w"], d["shift"], d["stride"], relu=True), None)
    else:
        conv3 = _conv_launch(step.conv3, c3)
        end = lambda y, x: (conv3(y, x), None)                                 # + the identity residual
    return lambda x, ready: end(conv2(conv1(x, ready)), x)


class ImageEncoder(_Planned, nn.Module):
    """ResNet-50 image encoder (reference encoders.py:7-70).

    ``forward(images[N,3,H,W])`` returns ``emb [N, emb_dim]`` or, with ``spatial_features``,
    ``(emb, spatial_emb [N, k*k, emb_dim])``; the Linear is shared, BatchNorm1d only on the global
    branch (encoders.py:61 vs :67).  The reference's ``pretrained=True`` download (encoders.py:34)
    is not reproduced: weights come from ``load_state_dict`` / ``from_pretrained``.
    """

    def __init__(self, emb_dim=256, dropout=0.2, spatial_features=False):
        super().__init__()
        self.spatial_features = spatial_features
        self.resnet = _resnet50_trunk()
        for p in self.resnet.parameters():
            p.requires_grad = False                       # encoders.py:35-36
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.linear = nn.Linear(2048, emb_dim)
        self.bn = nn.BatchNorm1d(emb_dim)
        self.dropout = nn.Dropout(dropout)

    def _build_plan(self):
        """fp32 weights -> NCHW vector-ALU convolutions (the parity path); bf16 weights -> channels-last
        activations with every bottleneck conv on the bf16 matrix cores (weights repacked once to
        [Cout, kh, kw, Cin]; the stem's 3 input channels are zero-padded to 8)."""
        wdt = self.linear.weight.dtype
        bf16 = wdt in hip.HALF_DTYPES            # the 16-bit paths (bf16 / fp16 storage and MFMA operands)
        # fp32 weights with option "f32_split": channels-last fp32 activations, every convolution / linear layer as three fp16 MFMAs
        # on split operands (csrc/gemm_f32x.hip) -- fp32-class results on the matrix cores instead of the vector ALUs
        split = (wdt == torch.float32 and self.linear.weight.is_cuda and bool(hip.option("f32_split"))
                 and all(hip.f32_split_ok(p) for p in self.parameters() if p.dim() > 1))

        def conv(c, bn, relu, residual=False, stem=False):
            s, b = _bn_affine(bn)
            w = c.weight.detach()
            if split:
                wl = w.permute(0, 2, 3, 1)                                   # [Cout, kh, kw, Cin]: ci fastest
                if wl.shape[3] % 4:                                          # the stem: 3 input channels zero-padded to 4
                    w4 = torch.zeros(tuple(wl.shape[:3]) + ((wl.shape[3] + 3) // 4 * 4,), dtype=w.dtype, device=w.device)
                    w4[..., :wl.shape[3]] = wl
                    wl = w4
                ent = dict(w=w.contiguous(), wx=hip.split_f32x(wl.reshape(wl.shape[0], -1).contiguous()), ks=w.shape[2], cin=wl.shape[3],
                           scale=s, shift=b, stride=c.stride[0], pad=c.padding[0], relu=relu, residual=residual)
                if ent["ks"] == 1 and ent["stride"] == 1 and hip.option("f32_planes"):
                    # the wide 1 x 1 layers (conv3, layer1's downsample) as a persistent streaming kernel (csrc/conv1x1_f32x.hip)
                    ent["wxs"] = f32xp.pack_conv1x1(ent["wx"])
                return ent
            if bf16 and stem:
                # 3 input channels zero-padded to 8: the stem becomes a Cin=8 channels-last conv on the matrix cores
                w8 = torch.zeros((w.shape[0], w.shape[2], w.shape[3], 8), dtype=w.dtype, device=w.device)
                w8[..., :w.shape[1]] = w.permute(0, 2, 3, 1)
                w = w8.contiguous()
            elif bf16:
                w = w.permute(0, 2, 3, 1).contiguous()
            else:
                w = w.contiguous()
            return dict(w=w, scale=s, shift=b, stride=c.stride[0], pad=c.padding[0], relu=relu, residual=residual)

        blocks = []
        stem = conv(self.resnet[0], self.resnet[1], True, stem=True)
        if bf16:
            stem["wpk"] = hip.pack_stem_weight(self.resnet[0].weight, wdt)      # the direct-convolution stem kernel's weight layout
        for blk in self._bottlenecks():
            ent = dict(
                down=conv(blk.downsample[0], blk.downsample[1], False) if blk.downsample is not None else None,
                c1=conv(blk.conv1, blk.bn1, True), c2=conv(blk.conv2, blk.bn2, True),
                c3=conv(blk.conv3, blk.bn3, True, residual=True), dual=None)
            if bf16 and ent["down"] is not None:
                # first block of a stage on the 16-bit path: relu(bn3(conv3(y)) + bn_d(downsample(x))) as ONE GEMM over
                # [y | x at the strided pixels] with the BatchNorm scales folded into the weights -- the identity
                # tensor (411 MB in stage 1 at 256 images) is neither written nor read back
                c3, dn = ent["c3"], ent["down"]
                cout = c3["w"].shape[0]
                w_cat = torch.cat([c3["w"].float().view(cout, -1) * c3["scale"][:, None],
                                   dn["w"].float().view(cout, -1) * dn["scale"][:, None]], 1)
                ent["dual"] = dict(w=w_cat.to(wdt).contiguous(), shift=(c3["shift"] + dn["shift"]).contiguous(), stride=dn["stride"])
            if bf16:
                # ``pk``: the weights in MFMA fragment order, which the register-streamed kernels read -- one copy per weight, chosen by
                # channel shapes alone (the same at every image size; ``_schedule`` picks the kernels): conv1 with 256 - 1,024 input
                # channels (conv1x1_wreg; the conv1 a tail or dual launch runs for the block before), conv2 / conv3 of the blocks
                # without downsample (the fused tails, conv3x3_s4, conv3 + residual on conv1x1_wreg), the dual GEMM's folded weight
                # up to K = 768 (conv1x1_dual_wreg).  Stage 4's wider layers (Cin 2,048, K = 1,536) stay unpacked.
                packed = [ent["c1"]] if 256 <= ent["c1"]["w"].shape[3] <= 1024 else []
                if ent["down"] is None:
                    packed += [ent["c2"], ent["c3"]]
                elif ent["dual"]["w"].shape[1] <= 768:
                    packed.append(ent["dual"])
                for c in packed:
                    c["pk"] = hip.pack_mfma_fragments(c["w"].reshape(c["w"].shape[0], -1).contiguous())
            blocks.append(ent)
        s, b = _bn_affine(self.bn)
        return dict(stem=stem, blocks=blocks, bn_scale=s, bn_shift=b, bf16=bf16, dtype=wdt, split=split,
                    lin_w=self.linear.weight.detach(), lin_b=self.linear.bias.detach().float().contiguous(),
                    lin_wx=hip.split_f32x(self.linear.weight.detach().contiguous()) if split else None)

    def _bottlenecks(self):
        return [blk for stage in list(self.resnet)[4:] for blk in stage]

    TRUNK_MAX_IMAGES = 384

    def _features_split(self, images, plan):
        """The trunk on channels-last fp32 tensors with split-operand MFMAs (plan["split"]) -> [N, H/32, W/32, 2048] fp32."""
        def cv(x, c, residual=None):
            if c.get("wxs") is not None and f32xp.conv1x1_stream_supported(x.shape[0] * x.shape[1] * x.shape[2], x.shape[3], c["wx"].shape[1]):
                return f32xp.conv1x1_stream(x, c["wxs"], c["scale"], c["shift"], residual=residual, relu=c["relu"])
            return hip.conv2d_nhwc_f32x(x, c["wx"], c["ks"], c["scale"], c["shift"], residual=residual, relu=c["relu"], stride=c["stride"],
                                        pad=c["pad"])
        def c12(x, c1, c2):
            # conv1 -> conv2 of stages 2 - 4 (3 x 3 at >= 128 channels): conv1 stores its output as fp16 planes, conv2 reads them through the
            # planes kernel (csrc/gemm_f32xp.hip: both operands by LDS-DMA, two wave groups a phase apart; 13 - 27 % faster, bit-identical)
            if hip.option("f32_planes") and c2["ks"] == 3 and c2["cin"] % 32 == 0 and c2["wx"].shape[1] >= 128 and not c1["residual"]:
                yp = f32xp.conv2d_nhwc_planes_out(x, c1["wx"], c1["ks"], c1["scale"], c1["shift"], relu=c1["relu"], stride=c1["stride"], pad=c1["pad"])
                return f32xp.conv2d_nhwc(yp, c2["wx"], 3, c2["scale"], c2["shift"], relu=c2["relu"], stride=c2["stride"], pad=c2["pad"])
            return cv(cv(x, c1), c2)
        st = plan["stem"]
        x = hip.nchw_to_nhwc_f32(images.float().contiguous(), cp=st["cin"])
        x = hip.maxpool3x3s2_nhwc_f32(cv(x, st))
        for blk in plan["blocks"]:
            y = c12(x, blk["c1"], blk["c2"])
            idt = x if blk["down"] is None else cv(x, blk["down"])
            x = cv(y, blk["c3"], residual=idt)
        return x

    @staticmethod
    def _features_f32(images, plan):
        """The parity path: NCHW fp32 tensors, every convolution on the vector ALUs -> [N, 2048, H/32, W/32]."""
        def cv(x, c, residual=None):
            return hip.conv2d_bn_act(x, c["w"], c["scale"], c["shift"], residual=residual, relu=c["relu"], stride=c["stride"], pad=c["pad"])
        x = hip.maxpool3x3s2(cv(images.contiguous(), plan["stem"]))
        for blk in plan["blocks"]:
            y = cv(cv(x, blk["c1"]), blk["c2"])
            x = cv(y, blk["c3"], residual=x if blk["down"] is None else cv(x, blk["down"]))
        return x

    def features(self, images):
        """Trunk output (encoders.py:56): ``[N, 2048, H/32, W/32]`` fp32 on the parity path,
        channels-last ``[N, H/32, W/32, 2048]`` bf16 on the bf16 path."""
        plan = self._get_plan()
        nhwc = plan["bf16"]
        # what torch's conv2d would refuse (the kernels take the layout on trust: a 1- or 4-channel tensor read as 3 channels is foreign
        # memory or garbage, not an error -- round 5 probe)
        if images.dim() != 4:
            raise RuntimeError(f"Expected 4D (batched) input to conv2d, but got input of size: {list(images.shape)}")
        packed_in = nhwc and images.shape[-1] == 8 and images.dtype == plan["dtype"]      # experiments.inference.preprocess_images' layout
        if not packed_in:
            if images.shape[1] != 3:
                raise RuntimeError(f"Given groups=1, weight of size [64, 3, 7, 7], expected input{list(images.shape)} to have 3 channels, "
                                   f"but got {images.shape[1]} channels instead")
            if images.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise TypeError(f"unsupported image dtype {images.dtype}: float32 (or the model's 16-bit type) NCHW images, or the packed "
                                "tensor of experiments.inference.preprocess_images")
        if plan["split"]:
            return self._features_split(images, plan)
        if not nhwc:
            return self._features_f32(images, plan)
        if images.shape[0] > self.TRUNK_MAX_IMAGES:
            #  the streaming / register-streamed 16-bit kernels index pixels with 32-bit magic divisions and are tuned for
            # <= 256 images per launch (the stage-1 dual kernel stops applying near 436 images): larger batches go through the trunk
            # in chunks of 256 -- every image's arithmetic is independent of its batch, so the features are the same bit for bit
            return torch.cat([self.features(images[i:i + 256]) for i in range(0, images.shape[0], 256)], 0)
        key = (tuple(images.shape), packed_in, hip.options_epoch)
        table = plan.setdefault("_trunk_tables", {}).get(key)
        if table is None:
            table = plan["_trunk_tables"][key] = self._trunk_table(plan, tuple(images.shape), packed_in)
        x, ready = images, None                           # ready: the NEXT block's conv1 output when the previous launch computed it
        for step in table:
            x, ready = step(x, ready)
        return x

    def _trunk_table(self, plan, shape, packed):
        """The 16-bit trunk for images of ``shape`` (``packed``: the [N, H, W, 8] layout) as [step(x, y1_ready) -> (x, y1_for_next_block)]:
        the stem, then one step per bottleneck, each running the kernels ``_schedule`` picks at the current ``encoder_generic`` level
        (0 = every specialised kernel; 1 = round 3's set; 2 = every bottleneck convolution through the implicit-GEMM tile kernel -- all
        three bit-identical; 3 = also the implicit-GEMM stem).  Built once per (shape, options epoch) and kept with the plan: it only
        binds the plan's tensors, so building it launches nothing (it may happen inside a hipGraph capture)."""
        stem, steps = _schedule(self._bottlenecks(), shape, packed, hip.option("encoder_generic"))
        st, blocks = plan["stem"], plan["blocks"]
        if stem == "stem_conv7_bn_relu_maxpool":
            # conv1 + bn1 + relu + maxpool as ONE direct-convolution launch that reads the caller's tensor as it is (fp32 NCHW
            # or the preprocessing kernels' packed 16-bit layout): no packing launch, no im2col traffic, no un-pooled activation
            table = [lambda x, _: (hip.stem_conv7_bn_relu_maxpool(x.contiguous() if packed else x.float().contiguous(), st["wpk"], st["scale"],
                                                                  st["shift"]), None)]
        else:
            # a packed input is already normalised + packed (experiments.inference.preprocess_images)
            pack = (lambda x: x.contiguous()) if packed else (lambda x: hip.pack_nchw_to_nhwc8(x.float().contiguous(), out_dtype=plan["dtype"]))
            if stem == "conv2d_nhwc_bn_relu_maxpool":
                # conv1 + bn1 + relu + maxpool in one launch: the un-pooled 112 x 112 x 64 activation never exists
                table = [lambda x, _: (hip.conv2d_nhwc_bn_relu_maxpool(pack(x), st["w"], st["scale"], st["shift"], st["stride"], st["pad"]), None)]
            else:
                conv = _conv_launch(stem, st)
                table = [lambda x, _: (hip.maxpool3x3s2_nhwc(conv(pack(x))), None)]
        for i, (blk, step) in enumerate(zip(blocks, steps)):
            table.append(_block_launch(blk, blocks[i + 1]["c1"] if step.fuse else None, step))
        return table

    @f32x_guarded
    def forward(self, images):
        _require_eval(self, self.dropout.p)
        plan = self._get_plan()
        feats = self.features(images)
        n = feats.shape[0]
        w, b = plan["lin_w"], plan["lin_b"]
        if plan["bf16"]:
            pooled, rows = hip.avgpool_nhwc(feats), feats.view(n, -1, feats.shape[-1])     # already [N, k*k, 2048]
        elif plan["split"]:
            pooled, rows = hip.avgpool_nhwc_f32(feats), feats.view(n, -1, feats.shape[-1])
            emb = hip.linear_f32x(pooled, plan["lin_wx"], b, scale=plan["bn_scale"], shift=plan["bn_shift"])
            if not self.spatial_features:
                return emb
            return emb, hip.linear_f32x(rows.reshape(-1, rows.shape[-1]), plan["lin_wx"], b).view(n, rows.shape[1], -1)
        else:
            pooled = hip.avgpool_rows(feats)
        emb = hip.linear(pooled, w, b, scale=plan["bn_scale"], shift=plan["bn_shift"])
        if not self.spatial_features:
            return emb
        if not plan["bf16"]:
            rows = hip.nchw_to_rows(feats)                                    # [N, k*k, 2048]
        rows2 = rows.reshape(-1, rows.shape[-1])
        if rows2.dtype == torch.float16:
            # fp16 underflows below 3e-8 where fp32 / bf16 do not, and TransformerDecoder reads a row with any exactly-zero feature as
            # padding (transformers.py:480): fp32 out of the GEMM, then a rounding that keeps non-zero values non-zero
            spatial = hip.round16_keep_nonzero(hip.linear(rows2, w, b, out_dtype=torch.float32), torch.float16)
        else:
            spatial = hip.linear(rows2, w, b)
        return emb, spatial.view(n, rows.shape[1], -1)


class LabelEncoder(nn.Module):
    """Mean label embedding (reference encoders.py:73-106)."""

    def __init__(self, num_tokens, emb_dim=256, dropout=0.2):
        super().__init__()
        self.embedding = nn.Embedding(num_tokens, emb_dim)
        self.dropout = nn.Dropout(dropout)

    def check(self, labels):
        """``nn.Embedding``'s IndexError for a label outside the table: one ``aminmax`` + a host read -- a blocking sync on the current
        stream, so the image + label encoders make it BEFORE the image trunk is queued (``ImageLabelEncoder.forward``), not behind it."""
        from .beam import check_ids
        check_ids(labels, self.embedding.num_embeddings)

    def forward(self, labels, out=None, checked=False):
        _require_eval(self, self.dropout.p)
        if not checked:
            self.check(labels)
        w = self.embedding.weight.detach()
        if out is None:
            out = torch.empty((labels.shape[0], w.shape[1]), dtype=w.dtype, device=w.device)
        return hip.label_mean(w, labels.contiguous(), out)


class ImageLabelEncoder(nn.Module):
    """Image + label encoder (reference encoders.py:109-144): Linear(cat[image_emb, label_emb])."""

    def __init__(self, num_tokens, emb_dim=256, dropout=0.2):
        super().__init__()
        self.image_encoder = ImageEncoder(emb_dim, dropout)
        self.label_encoder = LabelEncoder(num_tokens, emb_dim, dropout)
        self.linear = nn.Linear(2 * emb_dim, emb_dim)
        self.dropout = nn.Dropout(dropout)

    def _combine(self, image_emb, labels):
        n, e = image_emb.shape
        both = torch.empty((n, 2 * e), dtype=image_emb.dtype, device=image_emb.device)
        both[:, :e].copy_(image_emb)
        self.label_encoder(labels, out=both[:, e:], checked=True)
        return hip.linear(both, self.linear.weight.detach(), self.linear.bias.detach().float())

    @f32x_guarded
    def forward(self, images, labels):
        _require_eval(self, self.dropout.p)
        self.label_encoder.check(labels)                    # host sync in front of the trunk's launches, not behind them
        return self._combine(self.image_encoder(images), labels)


class SpatialImageLabelEncoder(ImageLabelEncoder):
    """BASELINE config 5 composition (no reference class): the image encoder
    keeps its spatial branch, the start embedding is Linear(cat[global_emb, label_emb])."""

    def __init__(self, num_tokens, emb_dim=512, dropout=0.2):
        super().__init__(num_tokens, emb_dim, dropout)
        self.image_encoder.spatial_features = True

    @f32x_guarded
    def forward(self, images, labels):
        _require_eval(self, self.dropout.p)
        self.label_encoder.check(labels)
        emb, spatial = self.image_encoder(images)
        return self._combine(emb, labels), spatial
