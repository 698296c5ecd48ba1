"""Teacher-forced (prefill) kernels at every history length they hold, against a plain fp64 statement of the reference's
attention (transformers.py:106-120: ``softmax(masked_fill(q k^T / scale, mask, -1e8)) v``) on the same operands -- rounded to
the 16-bit type first for bf16 / fp16 -- plus the model-level forward on both sides of the prefill switch (``_prefill_ok``).

``attn_self_prefill`` keeps a query's whole history in registers: 8 keys per loop iteration, 5 iterations in fp32 (40 keys),
7 in 16 bits (56 keys).  The tests below reach the top iteration with live, unmasked keys at every ``n_pos`` up to the limit.

Gates.  fp32: ``atol = 2e-5`` (as the decode kernels' tests).  16-bit: the kernels compute in fp32 and round once, so the error
is about half a unit in the last place of the output type at ``|want|``; the gates below are 1.25x the worst error measured
over each test's cases, in ulps (never looser than one ulp for the kernels that round once).  Below ``|want| = 2^-6`` the
fp32 accumulation of up to 56 products, not the 16-bit rounding, sets the error, so the ulp is taken at ``max(|want|, 2^-6)``."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attn_ref import BF16, DT_IDS, DTYPES, F16, F32, Gate as _Gate, attn_ref, rnd  # noqa: E402
from helpers import synthetic_sd, synth_images  # noqa: E402

LIMIT = {F32: 40, BF16: 56, F16: 56}           # _prefill_ok / dh_attn_self_prefill: 5 or 7 iterations of 8 keys
# 1.25 x the worst 16-bit error measured on an MI355X over each test's cases (ulps at max(|want|, 2^-6)); Gate.check prints it.
# The matrix-core cross-attention rounds the softmax weights to the operand type before its P V product (attn_items.h
# cross_core), so its error is set by those roundings, not by the output's: its worst case (S = 7, weights ~1/7, |out| near 0)
# is exactly that of the same arithmetic restated in torch.
ULP_GATE = {
    "self_prefill": {BF16: 1.25 * 0.5004, F16: 1.25 * 0.5061},
    "cross_prefill": {BF16: 1.25 * 0.5001, F16: 1.25 * 0.5027},
    "cross_prefill_packed": {BF16: 1.25 * 30.21, F16: 1.25 * 31.56},
    "attn_masked": {BF16: 1.25 * 0.5002, F16: 1.25 * 0.5180},
}


def Gate(name, dt):
    """attn_ref.Gate against this file's ULP_GATE: fp32 cases assert ``atol = 2e-5`` as they come, 16-bit cases record the
    error in ulps (at max(|want|, 2^-6)); ``check`` asserts the worst against the gate and prints it."""
    return _Gate(name, dt, ULP_GATE)


@pytest.fixture(scope="module")
def hip():
    from deephumor_amd import hip as h
    h.load()
    assert torch.cuda.is_available()
    return h


# ---- 1. attn_self_prefill: every history length --------------------------------------------------------------------------
def self_prefill_ref(qkv, tokens, n_seq, n_pos, n_heads, scale, pad_index):
    """Rows n * n_pos + t; key j of position t is row n * n_pos + j, masked when j > t (causal) or when j >= 1 and
    ``tokens[n, j - 1] == pad_index`` (key 0 is the image slot: never masked)."""
    x = qkv.view(n_seq, n_pos, 3, n_heads, 64).permute(2, 0, 3, 1, 4)            # [3, n, h, t, 64]
    j = torch.arange(n_pos)
    masked = (j[None, :] > j[:, None])[None, None]
    if pad_index >= 0:
        padk = torch.zeros(n_seq, n_pos, dtype=torch.bool)
        padk[:, 1:] = tokens[:, :n_pos - 1] == pad_index
        masked = masked | padk[:, None, None, :]
    return attn_ref(x[0], x[1], x[2], masked, scale).permute(0, 2, 1, 3).reshape(n_seq * n_pos, n_heads * 64)


@pytest.mark.parametrize("pad_index", [-1, 0, 5])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_attn_self_prefill_every_history_length(hip, dt, pad_index):
    gate = Gate("self_prefill", dt)
    live_top = False
    for n_pos in range(1, LIMIT[dt] + 1):
        for n_heads in (1, 8):
            for n_seq in (1, 3):                              # 3 * n_pos rows: the last workgroup of 4 waves is partial unless 4 | n_pos
                d = 64 * n_heads
                qkv = rnd(n_seq * n_pos, 3 * d, seed=n_pos + 100 * n_heads).to(dt)
                g = torch.Generator().manual_seed(1000 * n_pos + 10 * n_seq + n_heads)
                tok = torch.randint(0, 7, (n_seq, n_pos + 5), generator=g, dtype=torch.int32)   # <pad> here and there
                if pad_index >= 0 and n_pos >= 2:
                    tok[0, n_pos - 2] = pad_index              # the last key of sequence 0's last position
                    if n_seq > 1:
                        tok[-1] = pad_index                    # a sequence that is all <pad> after the image slot
                tokens = tok.cuda()[:, :max(n_pos - 1, 1)]     # row stride n_pos + 5 (tok_ld > n_pos - 1)
                got = hip.attn_self_prefill(qkv.cuda(), tokens, n_seq, n_pos, d, n_heads, 8.0, pad_index)
                want = self_prefill_ref(qkv.double(), tok, n_seq, n_pos, n_heads, 8.0, pad_index)
                gate.add(got, want, dict(n_pos=n_pos, n_heads=n_heads, n_seq=n_seq))
                # some sequence's last position sees live, unmasked keys in the top iteration
                if n_pos == LIMIT[dt]:
                    top = [j for j in range(n_pos - 8, n_pos) if pad_index < 0 or int(tok[0, j - 1]) != pad_index]
                    live_top |= len(top) > 0
    assert live_top
    gate.check()
    with pytest.raises(RuntimeError):                          # DH_REQUIRE(n_pos <= limit)
        n_pos = LIMIT[dt] + 1
        hip.attn_self_prefill(torch.zeros(n_pos, 3 * 64, dtype=dt, device="cuda"),
                              torch.zeros(1, n_pos, dtype=torch.int32, device="cuda"), 1, n_pos, 64, 1, 8.0, pad_index)


# ---- 2. attn_cross_prefill / attn_cross_prefill_packed ---------------------------------------------------------------------
def cross_ref(q, kv, keymask, n_img, n_pos, s, n_heads, scale):
    d = q.shape[1]
    dh = d // n_heads
    qq = q.double().view(n_img, n_pos, n_heads, dh).transpose(1, 2)
    k = kv[:, :d].double().reshape(n_img, s, n_heads, dh).transpose(1, 2)
    v = kv[:, d:].double().reshape(n_img, s, n_heads, dh).transpose(1, 2)
    out = attn_ref(qq, k, v, keymask.view(n_img, 1, 1, s).bool(), scale)
    return out.transpose(1, 2).reshape(n_img * n_pos, d)


def cross_case(dt, n_img, n_pos, s, d=512):
    """q as a column slice of a wider matrix (ldq = d + 128, 16-byte aligned), kv [n_img * s, 2d], one masked key in image 0
    and every key of image 1 masked (uniform attention)."""
    wide = rnd(n_img * n_pos, d + 128, seed=n_pos + s).to(dt)
    kv = rnd(n_img * s, 2 * d, seed=3 * s + n_img).to(dt)
    mask = torch.zeros(n_img * s, dtype=torch.uint8)
    mask[min(3, s - 1)] = 1
    if n_img > 1:
        mask[s:2 * s] = 1
    return wide, kv, mask


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_attn_cross_prefill(hip, dt):
    gate = Gate("cross_prefill", dt)
    d, h = 512, 8
    for n_img in (1, 3):
        for s in (1, 7, 49, 64, 65, 100):
            for n_pos in (1, 15, 16, 17, 33, 56):              # chunks of DH_ATTN_RPB = 16 positions
                wide, kv, mask = cross_case(dt, n_img, n_pos, s, d)
                qg = wide.cuda()[:, 64:64 + d]
                assert qg.stride(0) == d + 128
                got = hip.attn_cross_prefill(qg, kv.cuda(), mask.cuda(), n_img, n_pos, s, d, h, 8.0)
                gate.add(got, cross_ref(wide[:, 64:64 + d], kv, mask, n_img, n_pos, s, h, 8.0), dict(n_img=n_img, s=s, n_pos=n_pos))
    gate.check()


@pytest.mark.parametrize("dt", [BF16, F16], ids=DT_IDS[1:])
def test_attn_cross_prefill_packed(hip, dt):
    """The matrix-core form (16 positions per MFMA tile).  ``dperm = 1`` packs K's head-dim slots in the decode chain's order
    and reads q in the same order: the same dot products, summed in another order, so the same fp64 reference holds."""
    gate = Gate("cross_prefill_packed", dt)
    d, h = 512, 8
    for n_img in (1, 3):
        for s in (1, 7, 49, 64):
            kvs = {}
            for n_pos in (1, 15, 16, 17, 33, 56):
                wide, kv, mask = cross_case(dt, n_img, n_pos, s, d)
                qg = wide.cuda()[:, 64:64 + d]
                want = cross_ref(wide[:, 64:64 + d], kv, mask, n_img, n_pos, s, h, 8.0)
                for dperm in (0, 1):
                    if (s, dperm) not in kvs:
                        kvs[s, dperm] = hip.attn_cross_pack(kv.cuda(), n_img, s, d, h, dperm=bool(dperm))
                    kp, vt = kvs[s, dperm]
                    got = hip.attn_cross_prefill_packed(qg, kp, vt, mask.cuda(), n_img, n_pos, s, d, h, 8.0, dperm=bool(dperm))
                    gate.add(got, want, dict(n_img=n_img, s=s, n_pos=n_pos, dperm=dperm))
    gate.check()


# ---- 3. embed_prefill ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_embed_prefill_is_bit_exact(hip, dt):
    """x = src / scale + pos in fp32, rounded once: src is the start embedding at slot 0 and token t - 1 at position t (with a
    start embedding), else token t.  Both fp32 operations are correctly rounded in fp64 and rounded back, so bit for bit."""
    v = 50
    for d in (8, 64, 512):
        scale = math.sqrt(d)
        s32 = float(np.float32(scale))
        tok, pos = rnd(v, d, seed=1).to(dt), rnd(64, d, seed=2).to(dt)
        for n_seq in (1, 3):
            start = rnd(n_seq, d, seed=3).to(dt)
            for n_pos in (1, 2, 31, 32, 40, 41, 56, 57):
                ids = torch.randint(0, v, (n_seq, n_pos + 2), generator=torch.Generator().manual_seed(n_pos), dtype=torch.int32)
                idg = ids.cuda()
                for with_start in (True, False):
                    src = (torch.cat([start[:, None], tok[ids[:, :n_pos - 1].long()]], 1) if with_start
                           else tok[ids[:, :n_pos].long()])                                   # [n_seq, n_pos, d]
                    want = ((src.double() / s32).float().double() + pos[:n_pos].double()).float().to(dt).reshape(n_seq * n_pos, d)
                    got = hip.embed_prefill(tok.cuda(), pos.cuda(), start.cuda() if with_start else None,
                                            idg[:, :max(n_pos - 1, 1)] if with_start else idg[:, :n_pos], n_seq, n_pos, scale)
                    assert torch.equal(got.cpu(), want), (dt, d, n_seq, n_pos, with_start)


# ---- 4. attn_masked / MultiHeadAttentionLayer.forward ----------------------------------------------------------------------
def masked_ref(q, k, v, mask, bs, L, n_heads, scale):
    d = q.shape[1]
    dh = d // n_heads
    qq, kk, vv = (x.double().view(bs, L, n_heads, dh).transpose(1, 2) for x in (q, k, v))
    out = attn_ref(qq, kk, vv, None if mask is None else mask[:, None], scale)
    return out.transpose(1, 2).reshape(bs * L, d)


def masks(bs, L, g):
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool), 1).expand(bs, L, L).contiguous()
    rand = torch.rand(bs, L, L, generator=g) < 0.3
    full = rand.clone()
    full[bs - 1, L // 2] = True                                # a fully masked query row -> uniform weights
    return {"none": None, "causal": causal, "random": rand, "full_row": full}


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_attn_masked(hip, dt):
    gate = Gate("attn_masked", dt)
    bs, h = 2, 2
    for dh in (8, 64, 96, 128):                               # dh > 64: the second lane pass over the head dim
        d = h * dh
        scale = math.sqrt(dh)
        for L in (1, 63, 64, 65, 129):                        # keys in strides of 64 lanes
            g = torch.Generator().manual_seed(L + dh)
            wide = rnd(bs * L, 3 * d + 24, seed=L + dh).to(dt)
            q, k, v = wide[:, :d], wide[:, d + 8:2 * d + 8], wide[:, 2 * d + 24:]   # strided rows: ld = 3d + 24
            wg = wide.cuda()
            qg, kg, vg = wg[:, :d], wg[:, d + 8:2 * d + 8], wg[:, 2 * d + 24:]
            for name, m in masks(bs, L, g).items():
                got = hip.attn_masked(qg, kg, vg, None if m is None else m.cuda(), bs, L, d, h, scale)
                gate.add(got, masked_ref(q, k, v, m, bs, L, h, scale), dict(dh=dh, L=L, mask=name))
    gate.check()


def test_attn_masked_at_the_lds_limit(hip):
    """4 waves x (dh + L) fp32 scores in LDS <= 64 KiB: L = 4096 - dh is accepted, one more key is refused."""
    dh = 64
    L = 4096 - dh
    q, k, v = (rnd(L, dh, seed=i) for i in range(3))
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool), 1)[None]
    got = hip.attn_masked(q.cuda(), k.cuda(), v.cuda(), causal.cuda(), 1, L, dh, 1, 8.0)
    np.testing.assert_allclose(got.cpu().double().numpy(), masked_ref(q, k, v, causal, 1, L, 1, 8.0).numpy(), atol=2e-5, rtol=0)
    L += 1
    with pytest.raises(RuntimeError):
        hip.attn_masked(*(torch.zeros(L, dh, device="cuda") for _ in range(3)), None, 1, L, dh, 1, 8.0)


def test_multi_head_attention_layer_head_dim_96():
    """MultiHeadAttentionLayer.forward (two heads of 96) at L = 65 against the oracle's restatement."""
    import deephumor_amd.models as M
    from oracle import ref_path as R
    torch.manual_seed(5)
    layer = M.MultiHeadAttentionLayer(192, 2).eval()
    sd = {"a." + k: t.clone() for k, t in layer.state_dict().items()}
    layer = layer.cuda()
    g = torch.Generator().manual_seed(6)
    bs, L = 2, 65
    q, k, v = (torch.randn(bs, L, 192, generator=g) for _ in range(3))
    mask = masks(bs, L, g)["full_row"] | masks(bs, L, g)["causal"]
    for m in (None, mask):
        with torch.no_grad():
            got = layer(q.cuda(), k.cuda(), v.cuda(), mask=None if m is None else m.cuda())
        want = R.mha(sd, "a", q, k, v, m, 2)
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-5, rtol=1e-4)


# ---- 5. model level, at the switch -----------------------------------------------------------------------------------------
_SD = {}


def model(kind, dt=F32):
    import deephumor_amd.models as M
    if kind not in _SD:
        _SD[kind] = synthetic_sd(kind)
    sd, hp = _SD[kind]
    m = getattr(M, kind)(**hp).eval()
    m.load_state_dict(sd)
    return m.cuda().to(dt), sd, hp


def long_captions(cap_len, v=1000):
    """4 captions of cap_len tokens: rows 0 and 2 have no <pad> at all (every key live up to the last position), row 1 has
    <pad> from the middle on, row 3 is short."""
    g = np.random.Generator(np.random.Philox(key=[1234, cap_len]))
    cap = torch.from_numpy(g.integers(6, v, size=(4, cap_len)).astype(np.int64))
    lengths = torch.tensor([cap_len + 1, cap_len // 2, cap_len + 1, 6])
    for r, n in enumerate(lengths.tolist()):
        cap[r, n - 1:] = 0
    labels = torch.from_numpy(g.integers(6, v, size=(4, 3)).astype(np.int64))
    return cap, lengths, labels


def seq_of(kind, cap_len):
    return cap_len + 1 if kind == "CaptioningTransformerBase" else max(cap_len + 1, 49)      # 49 encoder rows


def run(m, kind, images, cap, lengths, labels):
    args = (images.cuda(), cap.cuda(), lengths) + ((labels.cuda(),) if "WithLabels" in kind else ())
    with torch.no_grad():
        return m(*args).float().cpu()


@pytest.fixture(scope="module")
def images():
    return synth_images(4, seed=0)


@pytest.mark.parametrize("kind", ["CaptioningTransformerBase"])
def test_forward_fp32_at_the_prefill_limit(kind, images):
    """seq = 40 (prefill, top iteration live) and 41 (position by position): logits within 1e-3 of the oracle, with and
    without the split-operand fp32 GEMMs.  (The decoders with encoder rows pad the sequence to the encoder's 49 positions
    (transformers.py:450), so in fp32 only the Base model reaches the prefill form.)"""
    from deephumor_amd import hip
    from oracle import ref_path as R
    m, sd, hp = model(kind)
    dec = m.decoder
    for cap_len in (39, 40):
        seq = seq_of(kind, cap_len)
        assert dec._prefill_ok(dec._get_plan(), seq) == (seq <= 40)
        cap, lengths, labels = long_captions(cap_len)
        want = R.model_forward(kind, sd, hp, images, cap, lengths, labels if "WithLabels" in kind else None)
        for split in (0, 1):
            with hip.option_scope(f32_split=split):
                got = run(m, kind, images, cap, lengths, labels)
            assert got.shape == want.shape == (4, seq, hp["num_tokens"])
            np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-3, rtol=0, err_msg=f"seq {seq} f32_split {split}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=DT_IDS[1:])
@pytest.mark.parametrize("kind", ["CaptioningTransformerBase", "CaptioningTransformer", "CaptioningTransformerWithLabels"])
def test_forward_16bit_at_the_prefill_limit(kind, dt, images):
    """seq = 56 (prefill) equals the position-by-position form (test_forward_prefill_equals_position_by_position's 2e-2), and
    56 and 57 agree with the fp32 HIP logits at test_models_bf16_close_to_reference's gates."""
    m32, _, hp = model(kind)
    m16, _, _ = model(kind, dt)
    assert m32.decoder._prefill_ok(m32.decoder._get_plan(), 56) is False         # the fp32 side runs position by position
    dec = m16.decoder
    for cap_len in (55, 56):
        seq = seq_of(kind, cap_len)
        assert dec._prefill_ok(dec._get_plan(), seq) == (seq <= 56)
        cap, lengths, labels = long_captions(cap_len)
        ref = run(m32, kind, images, cap, lengths, labels)
        out = run(m16, kind, images, cap, lengths, labels)
        assert out.shape == ref.shape == (4, seq, hp["num_tokens"])
        err = (out - ref).abs()
        if dt == BF16:
            assert float(err.max()) < 0.6 and float(err.mean()) < 0.08, (seq, float(err.max()), float(err.mean()))
            assert float((out.argmax(-1) == ref.argmax(-1)).float().mean()) > 0.93
        else:
            assert float(err.max()) < 0.1 and float(err.mean()) < 0.012, (seq, float(err.max()), float(err.mean()))
            assert float((out.argmax(-1) == ref.argmax(-1)).float().mean()) > 0.98
        if seq <= 56:
            dec._prefill_ok = lambda plan, s: False
            try:
                slow = run(m16, kind, images, cap, lengths, labels)
            finally:
                del dec._prefill_ok
            np.testing.assert_allclose(out.numpy(), slow.numpy(), atol=2e-2, rtol=0)
