"""Torch restatement of the keypoint-set predictor behind the reference's plain backbone (`--backbone
resnet50`, REV/models/backbone.py:57-102,188-190): torchvision ResNet-50 cut after layer3, no neck,
input_proj a 1x1 conv 1024 -> 256 straight on the stride-16 map (REV/models/detr_speed.py:54-55,81).
Test infrastructure only.

Everything is oracle/model_ref.py's own functions (bottleneck, position table, attention, LayerNorm, head
MLP) in model_ref.forward's order; only the backbone's tail differs.  Pinned against
tests/golden/model_r50s16_*.npz, which tools/gen_golden_s16.py records from the reference's model code.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import model_ref
from attention_map_ref import mha_weights_from_inputs


def backbone_s16(x, sd):
    """xs16 [B,1024,S/16,S/16]: stem, max-pool, layer1..3 (layer4 and fc are never built into the model)."""
    b = "backbone.0.body"
    y = F.relu(model_ref._frozen_bn(F.conv2d(x, sd[b + ".conv1.weight"], stride=2, padding=3), sd, b + ".bn1"))
    y = F.max_pool2d(y, 3, 2, 1)
    for li, n in ((1, 3), (2, 4), (3, 6)):
        for k in range(n):
            y = model_ref._bottleneck(y, sd, f"{b}.layer{li}.{k}", 2 if (k == 0 and li > 1) else 1)
    return y


def forward(images, sd, cfg, dtype=torch.float32, return_stages=False, return_maps=False):
    """images [B,3,S,S] -> dict(pred_logits [B,Q,12], pred_points [B,Q,2], hs [L,B,Q,d], aux_logits,
    aux_points), computed in `dtype` (float64: the conditioning check of tools/gen_golden_s16.py).
    return_stages adds xs16 / src / memory; return_maps adds enc_maps / dec_maps, every layer's head-averaged
    attention weights (tests/attention_map_ref.py)."""
    assert cfg.backbone == "resnet50"
    images = torch.as_tensor(images, dtype=torch.float32).to(dtype)
    sd = {k: torch.as_tensor(v, dtype=torch.float32).to(dtype) for k, v in sd.items()}
    nh = cfg.nheads
    xs16 = backbone_s16(images, sd)
    B, _, h, w = xs16.shape
    src = F.conv2d(xs16, sd["input_proj.weight"], sd["input_proj.bias"])
    src0 = src
    pos = model_ref.sine_pos(h, w, cfg.hidden_dim).to(dtype)[None].expand(B, -1, -1, -1)   # the model's fp32 table
    src = src.flatten(2).transpose(1, 2)               # [B, HW, d] (row-major h*W + w)
    pos = pos.flatten(2).transpose(1, 2)
    enc_maps, dec_maps = [], []
    for i in range(cfg.enc_layers):
        p = f"transformer.encoder.layers.{i}"
        qk = src + pos
        if return_maps:
            enc_maps.append(mha_weights_from_inputs(qk, qk, sd, p + ".self_attn", nh))
        src = model_ref._ln(src + model_ref._mha(qk, qk, src, sd, p + ".self_attn", nh), sd, p + ".norm1")
        ff = F.linear(F.relu(F.linear(src, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])),
                      sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
        src = model_ref._ln(src + ff, sd, p + ".norm2")
    memory = src
    qpos = sd["query_embed.weight"][None].expand(B, -1, -1)
    tgt = torch.zeros_like(qpos)
    hs = []
    for i in range(cfg.dec_layers):
        p = f"transformer.decoder.layers.{i}"
        qk = tgt + qpos
        tgt = model_ref._ln(tgt + model_ref._mha(qk, qk, tgt, sd, p + ".self_attn", nh), sd, p + ".norm1")
        if return_maps:
            dec_maps.append(mha_weights_from_inputs(tgt + qpos, memory + pos, sd, p + ".multihead_attn", nh))
        tgt = model_ref._ln(tgt + model_ref._mha(tgt + qpos, memory + pos, memory, sd, p + ".multihead_attn", nh),
                            sd, p + ".norm2")
        ff = F.linear(F.relu(F.linear(tgt, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"])),
                      sd[p + ".linear2.weight"], sd[p + ".linear2.bias"])
        tgt = model_ref._ln(tgt + ff, sd, p + ".norm3")
        hs.append(model_ref._ln(tgt, sd, "transformer.decoder.norm"))
    hs = torch.stack(hs)                                # [L, B, Q, d]
    logits = F.linear(hs, sd["cls_embed.weight"], sd["cls_embed.bias"])
    points = model_ref._mlp3(hs, sd, "point_embed").sigmoid()
    out = {"pred_logits": logits[-1], "pred_points": points[-1], "hs": hs,
           "aux_logits": logits[:-1], "aux_points": points[:-1]}
    if return_stages:
        out.update(xs16=xs16, src=src0, memory=memory)
    if return_maps:
        out.update(enc_maps=enc_maps, dec_maps=dec_maps)
    return out
