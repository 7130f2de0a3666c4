"""Torch restatement of the keypoint-set predictor with the reference's GroupNorm backbone (`--bn group_bn`:
REV/models/backbone.py:168-181, MyGroupNorm = nn.GroupNorm(32, C) in all 43 norm positions of the ResNet-50), for both
backbones and both transformer orders.  Test infrastructure only.

The backbone is restated here with F.group_norm; the neck and the transformer are oracle/model_ref.py's and
tests/model_prenorm_ref.py's arithmetic.  Pinned against tests/golden/model_groupnorm_*.npz, which
tools/gen_golden_groupnorm.py records from the reference's model code.

emulate_bf16=True rounds every GEMM / convolution operand and every stored activation to bf16 and keeps the
accumulation, the GroupNorm / LayerNorm statistics, the softmax and the heads in `dtype`: a conv's bare output is
stored (rounded), its GroupNorm reads the stored values and the normalised, residual-added, rectified result is
rounded once -- the arithmetic a bf16 implementation with fp32 accumulation performs, whatever its kernels.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import model_ref
from model_prenorm_ref import _conv_bn, _ffn, _mha, _rounder


def _gn(x, sd, p):
    return F.group_norm(x, 32, sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def src_gn(images, sd, cfg, r):
    """src [B,d,h,w]: the GroupNorm ResNet-50 (+ the stride-8 neck) + input_proj; r rounds operands and stores"""
    conv = lambda x, key, stride=1, padding=0: r(F.conv2d(r(x), r(sd[key + ".weight"]), None, stride, padding))  # noqa: E731
    b = "backbone.0.body"
    y = r(F.relu(_gn(conv(images, b + ".conv1", 2, 3), sd, b + ".bn1")))
    y = F.max_pool2d(y, 3, 2, 1)
    feats = {}
    for li, n in ((1, 3), (2, 4), (3, 6)):
        for k in range(n):
            p = f"{b}.layer{li}.{k}"
            s = 2 if (k == 0 and li > 1) else 1
            t = r(F.relu(_gn(conv(y, p + ".conv1"), sd, p + ".bn1")))
            t = r(F.relu(_gn(conv(t, p + ".conv2", s, 1), sd, p + ".bn2")))
            t = _gn(conv(t, p + ".conv3"), sd, p + ".bn3")
            idt = r(_gn(conv(y, p + ".downsample.0", s), sd, p + ".downsample.1")) if k == 0 else y
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


def forward(images, sd, cfg, dtype=torch.float32, emulate_bf16=False):
    """images [B,3,S,S] -> dict(pred_logits [B,Q,12], pred_points [B,Q,2], hs [L,B,Q,d], aux_logits, aux_points,
    memory), computed in `dtype`."""
    assert cfg.norm == "group_bn"
    r = _rounder(emulate_bf16)
    images = torch.as_tensor(images, dtype=torch.float32).to(dtype)
    sd = {k: torch.as_tensor(v, dtype=torch.float32).to(dtype) for k, v in sd.items()}
    nh, pre = cfg.nheads, cfg.pre_norm
    src = src_gn(images, sd, cfg, r)
    B, _, h, w = src.shape
    pos = model_ref.sine_pos(h, w, cfg.hidden_dim).to(dtype)[None].expand(B, -1, -1, -1)
    s = r(src.flatten(2).transpose(1, 2))               # [B, HW, d]
    pos = r(pos.flatten(2).transpose(1, 2))
    ln = lambda x, p: r(model_ref._ln(x, sd, p))        # noqa: E731
    for i in range(cfg.enc_layers):
        p = f"transformer.encoder.layers.{i}"
        if pre:
            n = ln(s, p + ".norm1")
            qk = n + pos
            s = r(s + _mha(qk, qk, n, sd, p + ".self_attn", nh, r))
            s = r(s + _ffn(ln(s, p + ".norm2"), sd, p, r))
        else:
            qk = s + pos
            s = ln(s + _mha(qk, qk, s, sd, p + ".self_attn", nh, r), p + ".norm1")
            s = ln(s + _ffn(s, sd, p, r), p + ".norm2")
    memory = ln(s, "transformer.encoder.norm") if pre else s
    kpos = r(memory + pos)
    qpos = r(sd["query_embed.weight"])[None].expand(B, -1, -1)
    t = torch.zeros_like(qpos)
    hs = []
    for i in range(cfg.dec_layers):
        p = f"transformer.decoder.layers.{i}"
        if pre:
            n = ln(t, p + ".norm1")
            qk = n + qpos
            t = r(t + _mha(qk, qk, n, sd, p + ".self_attn", nh, r))
            t = r(t + _mha(ln(t, p + ".norm2") + qpos, kpos, memory, sd, p + ".multihead_attn", nh, r))
            t = r(t + _ffn(ln(t, p + ".norm3"), sd, p, r))
        else:
            qk = t + qpos
            t = ln(t + _mha(qk, qk, t, sd, p + ".self_attn", nh, r), p + ".norm1")
            t = ln(t + _mha(t + qpos, kpos, memory, sd, p + ".multihead_attn", nh, r), p + ".norm2")
            t = ln(t + _ffn(t, sd, p, r), p + ".norm3")
        hs.append(model_ref._ln(t, sd, "transformer.decoder.norm"))
    hs = torch.stack(hs)                                # [L, B, Q, d]
    logits = F.linear(hs, sd["cls_embed.weight"], sd["cls_embed.bias"])
    points = model_ref._mlp3(hs, sd, "point_embed").sigmoid()
    return {"pred_logits": logits[-1], "pred_points": points[-1], "hs": hs,
            "aux_logits": logits[:-1], "aux_points": points[:-1], "memory": memory}
