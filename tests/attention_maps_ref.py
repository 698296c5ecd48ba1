"""What the attention-map tests share (test_attention_maps_cpu.py, test_attention_maps_gpu.py): the fp64 statement of the
reference decoder's teacher-forced forward that also returns what the reference throws away -- the last layer's
encoder-attention softmax (transformers.py:106-115), averaged over the heads -- and the sharpened weights the model-level
tests load.  Plain module, no GPU use.

``teacher_forced_maps`` follows ``oracle/ref_path.transformer_forward`` statement by statement (same padding of ``x`` and
``enc_out`` to a common length, same masks, post-LN layers), in fp64 on whatever weights it is given: fp32 weights restate the
reference, 16-bit-rounded weights restate what a bf16 / fp16 model would compute without any rounding of its own.
tests/test_attention_maps_cpu.py pins it to golden G23 (the real reference's hook output) and to the oracle's logits."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("CaptioningTransformer", "CaptioningTransformerWithLabels")
GAIN = 8.0
N_KEYS = 49


def golden(kind):
    return np.load(os.path.join(GOLDEN, f"g23_attention_{kind}.npz"))


def last_layer(sd, p="decoder"):
    n = 0
    while f"{p}.layers.{n + 1}.self_attn.fc_q.weight" in sd:
        n += 1
    return n


def sharpened(sd, gain=GAIN, p="decoder"):
    """A copy of the state dict with the LAST layer's encoder-attention query projection multiplied by ``gain``: the energies of
    that one softmax grow ``gain``-fold, nothing in front of it changes.  On the synthetic weights the maps are almost flat
    (largest weight 0.029 against the uniform 0.0204); with gain 8 maps of different rows or positions are >= 1.6e-2 apart."""
    out = {k: v.clone() for k, v in sd.items()}
    lp = f"{p}.layers.{last_layer(sd, p)}.enc_attn.fc_q."
    out[lp + "weight"] = out[lp + "weight"] * gain
    out[lp + "bias"] = out[lp + "bias"] * gain
    return out


def _mha(sd, p, query, key, value, mask, n_heads):
    """MultiHeadAttentionLayer.forward (transformers.py:82-129) -> (output, softmax weights [bs, H, seq, seq])."""
    bs, seq, hid = query.shape
    dh = hid // n_heads
    q = F.linear(query, sd[p + ".fc_q.weight"], sd[p + ".fc_q.bias"]).view(bs, seq, n_heads, dh).permute(0, 2, 1, 3)
    k = F.linear(key, sd[p + ".fc_k.weight"], sd[p + ".fc_k.bias"]).view(bs, seq, n_heads, dh).permute(0, 2, 3, 1)
    v = F.linear(value, sd[p + ".fc_v.weight"], sd[p + ".fc_v.bias"]).view(bs, seq, n_heads, dh).permute(0, 2, 1, 3)
    energy = (q @ k) / sd[p + ".scale"]
    energy = energy.masked_fill(mask.unsqueeze(1), -1e8)                            # :110-111
    att = torch.softmax(energy, dim=-1)
    x = (att @ v).permute(0, 2, 1, 3).reshape(bs, seq, hid)
    return F.linear(x, sd[p + ".fc_o.weight"], sd[p + ".fc_o.bias"]), att


def _ln(sd, p, x):
    return F.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def teacher_forced_maps(sd, start_emb, enc_out, tokens, pad_index, n_heads, p="decoder", with_logits=False):
    """``tokens`` int64 ``[bs, L]`` teacher-forced behind the image slot -> fp64 ``maps [bs, L + 1, seq]``: row ``c`` is the mean
    over heads of the last layer's encoder-attention softmax at position ``c`` (the position that has seen ``tokens[:, :c]`` and
    whose logits decide token ``c``), over all ``seq = max(L + 1, S)`` keys of the reference's padded formulation -- the
    image's S patches first.  ``with_logits``: also the fp64 logits ``[bs, seq, V]`` (``oracle.ref_path.transformer_forward``'s)."""
    sd = {k: v.double() for k, v in sd.items() if k.startswith(p + ".")}
    start_emb, enc_out, x = start_emb.double(), enc_out.double(), tokens.long()
    bs, dec_len = x.shape
    dec_len += 1
    enc_len, hid = enc_out.shape[1:3]
    seq = max(dec_len, enc_len)                                                     # :450
    x = torch.cat([x, torch.full((bs, seq - dec_len), pad_index, dtype=torch.long)], dim=1)
    enc_out = torch.cat([enc_out, torch.zeros(bs, seq - enc_len, hid, dtype=torch.float64)], dim=1)
    tok = torch.cat([start_emb.unsqueeze(1), sd[p + ".tok_embedding.weight"][x]], dim=1) / sd[p + ".scale"]      # :462
    h = tok + sd[p + ".pos_embedding.weight"][torch.arange(seq)][None]
    ids = torch.cat([torch.ones(bs, 1, dtype=torch.long), x], dim=1)                # :474
    self_mask = (ids == pad_index)[:, None, :].expand(bs, seq, seq) | torch.triu(torch.ones(seq, seq), 1).bool()[None]
    row_nonzero = (enc_out != 0.).all(dim=-1)                                       # :480
    enc_mask = (row_nonzero.long() == pad_index)[:, None, :].expand(bs, seq, seq)   # :481
    att = None
    for n in range(last_layer(sd, p) + 1):
        lp = f"{p}.layers.{n}"
        h = _ln(sd, lp + ".self_attn_ln", h + _mha(sd, lp + ".self_attn", h, h, h, self_mask, n_heads)[0])
        o, att = _mha(sd, lp + ".enc_attn", h, enc_out, enc_out, enc_mask, n_heads)
        h = _ln(sd, lp + ".enc_attn_ln", h + o)
        ff = F.linear(torch.relu(F.linear(h, sd[lp + ".pf.fc_1.weight"], sd[lp + ".pf.fc_1.bias"])),
                      sd[lp + ".pf.fc_2.weight"], sd[lp + ".pf.fc_2.bias"])
        h = _ln(sd, lp + ".pf_ln", h + ff)
    maps = att.mean(1)[:, :dec_len]
    if with_logits:
        return maps, F.linear(h, sd[p + ".classifier.weight"], sd[p + ".classifier.bias"])
    return maps
