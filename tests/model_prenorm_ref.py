"""Torch restatement of the keypoint-set predictor with the reference's pre-norm transformer (`--pre_norm`:
REV/models/transformer.py forward_pre of TransformerEncoderLayer / TransformerDecoderLayer, TransformerEncoder's
closing LayerNorm, TransformerDecoder's shared norm), for both backbones.  Test infrastructure only.

Everything up to src is oracle/model_ref.py's / tests/model_s16_ref.py's own backbone; the transformer is restated
here.  Pinned against tests/golden/model_prenorm_*.npz, which tools/gen_golden_prenorm.py records from the
reference's model code.

emulate_bf16=True rounds every GEMM / convolution operand (FrozenBN folded into the weights first, as a
deployment does) and every stored activation to bf16 and keeps the accumulation, softmax, LayerNorm statistics
and heads in `dtype`: the arithmetic a bf16 implementation with fp32 accumulation performs, whatever its kernels.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import model_ref
import model_s16_ref
from attention_map_ref import head_avg_probs


def _rounder(emulate):
    if not emulate:
        return lambda x: x
    return lambda x: x.to(torch.bfloat16).to(x.dtype)


def _conv_bn(x, sd, conv, bn, r, stride=1, padding=0, bias=None):
    """conv (+ FrozenBN folded into its weights) over rounded operands"""
    w = sd[conv + ".weight"]
    b = sd[bias] if bias else None
    if bn:
        scale = sd[bn + ".weight"] * (sd[bn + ".running_var"] + 1e-5).rsqrt()
        b = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        w = w * scale[:, None, None, None]
    return F.conv2d(r(x), r(w), b, stride=stride, padding=padding)


def _src_emulated(images, sd, cfg, r):
    """src [B,d,h,w] with bf16 operands and bf16 stored activations"""
    b = "backbone.0.body"
    y = r(F.relu(_conv_bn(images, sd, b + ".conv1", b + ".bn1", r, 2, 3)))
    y = F.max_pool2d(y, 3, 2, 1)
    feats = {}
    for li, n in ((1, 3), (2, 4), (3, 6)):
        for k in range(n):
            p = f"{b}.layer{li}.{k}"
            s = 2 if (k == 0 and li > 1) else 1
            t = r(F.relu(_conv_bn(y, sd, p + ".conv1", p + ".bn1", r)))
            t = r(F.relu(_conv_bn(t, sd, p + ".conv2", p + ".bn2", r, s, 1)))
            t = _conv_bn(t, sd, p + ".conv3", p + ".bn3", r)
            idt = _conv_bn(y, sd, p + ".downsample.0", p + ".downsample.1", r, s) if k == 0 else y
            y = r(F.relu(t + idt))
        feats[li] = y
    if cfg.backbone == "resnet50":
        return _conv_bn(feats[3], sd, "input_proj", None, r, bias="input_proj.bias")
    a = _conv_bn(feats[2], sd, "backbone.0.s8_latern", None, r)
    up = r(F.interpolate(feats[3], scale_factor=2, mode="bilinear", align_corners=True))
    c = _conv_bn(up, sd, "backbone.0.s16_latern", None, r, padding=1)
    neck = r(_conv_bn(r(torch.cat([a, c], 1)), sd, "backbone.0.output_conv", None, r, padding=1,
                      bias="backbone.0.output_conv.bias"))
    return _conv_bn(neck, sd, "input_proj", None, r, bias="input_proj.bias")


def _lin(x, sd, p, r, rows=None):
    w, b = sd[p + "weight"], sd[p + "bias"]
    if rows is not None:
        w, b = w[rows], b[rows]
    return F.linear(r(x), r(w), b)


def _mha(q_in, k_in, v_in, sd, p, nh, r, maps=None):
    """nn.MultiheadAttention, batch-first; q, k, V, the probabilities and the attention output are stored
    activations (rounded when emulating)"""
    d = q_in.shape[-1]
    hd = d // nh
    q = r(_lin(q_in, sd, p + ".in_proj_", r, slice(0, d)))
    k = r(_lin(k_in, sd, p + ".in_proj_", r, slice(d, 2 * d)))
    v = r(_lin(v_in, sd, p + ".in_proj_", r, slice(2 * d, 3 * d)))
    B, Lq, _ = q.shape
    q = q.view(B, Lq, nh, hd).transpose(1, 2)
    k = k.view(B, -1, nh, hd).transpose(1, 2)
    v = v.view(B, -1, nh, hd).transpose(1, 2)
    if maps is not None:
        maps.append(head_avg_probs(q, k))
    a = r(torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2), dim=-1)) @ v
    a = r(a.transpose(1, 2).reshape(B, Lq, d))
    return _lin(a, sd, p + ".out_proj.", r)


def _ffn(x, sd, p, r):
    return _lin(r(F.relu(_lin(x, sd, p + ".linear1.", r))), sd, p + ".linear2.", r)


def forward(images, sd, cfg, dtype=torch.float32, emulate_bf16=False, return_maps=False):
    """images [B,3,S,S] -> dict(pred_logits [B,Q,12], pred_points [B,Q,2], hs [L,B,Q,d], aux_logits, aux_points,
    memory), computed in `dtype`.  return_maps adds enc_maps / dec_maps, every layer's head-averaged attention
    weights."""
    assert cfg.pre_norm
    r = _rounder(emulate_bf16)
    images = torch.as_tensor(images, dtype=torch.float32).to(dtype)
    sd = {k: torch.as_tensor(v, dtype=torch.float32).to(dtype) for k, v in sd.items()}
    nh = cfg.nheads
    if emulate_bf16:
        src = _src_emulated(images, sd, cfg, r)
    elif cfg.backbone == "resnet50":
        src = F.conv2d(model_s16_ref.backbone_s16(images, sd), sd["input_proj.weight"], sd["input_proj.bias"])
    else:
        src = F.conv2d(model_ref.backbone_s8(images, sd)[2], sd["input_proj.weight"], sd["input_proj.bias"])
    B, _, h, w = src.shape
    pos = model_ref.sine_pos(h, w, cfg.hidden_dim).to(dtype)[None].expand(B, -1, -1, -1)
    s = r(src.flatten(2).transpose(1, 2))               # the residual stream [B, HW, d]
    pos = r(pos.flatten(2).transpose(1, 2))
    ln = lambda x, p: r(model_ref._ln(x, sd, p))        # noqa: E731
    enc_maps, dec_maps = ([], []) if return_maps else (None, None)
    for i in range(cfg.enc_layers):
        p = f"transformer.encoder.layers.{i}"
        n = ln(s, p + ".norm1")
        qk = n + pos
        s = r(s + _mha(qk, qk, n, sd, p + ".self_attn", nh, r, enc_maps))
        s = r(s + _ffn(ln(s, p + ".norm2"), sd, p, r))
    memory = ln(s, "transformer.encoder.norm")
    kpos = r(memory + pos)
    qpos = r(sd["query_embed.weight"])[None].expand(B, -1, -1)
    t = torch.zeros_like(qpos)
    hs = []
    for i in range(cfg.dec_layers):
        p = f"transformer.decoder.layers.{i}"
        n = ln(t, p + ".norm1")
        qk = n + qpos
        t = r(t + _mha(qk, qk, n, sd, p + ".self_attn", nh, r))
        t = r(t + _mha(ln(t, p + ".norm2") + qpos, kpos, memory, sd, p + ".multihead_attn", nh, r, dec_maps))
        t = r(t + _ffn(ln(t, p + ".norm3"), sd, p, r))
        hs.append(model_ref._ln(t, sd, "transformer.decoder.norm"))
    hs = torch.stack(hs)                                # [L, B, Q, d]
    logits = F.linear(hs, sd["cls_embed.weight"], sd["cls_embed.bias"])
    points = model_ref._mlp3(hs, sd, "point_embed").sigmoid()
    out = {"pred_logits": logits[-1], "pred_points": points[-1], "hs": hs,
           "aux_logits": logits[:-1], "aux_points": points[:-1], "memory": memory}
    if return_maps:
        out.update(enc_maps=enc_maps, dec_maps=dec_maps)
    return out
