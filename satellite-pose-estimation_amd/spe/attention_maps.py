"""The array side of the reference's attention heat maps (REV/visualize_features.py:171-227), over the maps
DETR.forward_with_attention returns.  No plotting: each function returns the [feat, feat] arrays the
reference hands to imshow, one per query, for a caller to draw.

Tokens are in row-major order over the feature map (token = y * feat + x, feat = cfg.feat_size: stride 8, or 16
behind the plain resnet50 backbone), as the model flattens
them (REV/models/transformer.py:51-55).
"""
from __future__ import annotations

import torch


def _check(m, feat, name):
    m = torch.as_tensor(m)
    if m.dim() != 3 or m.shape[-1] != feat * feat:
        raise ValueError(f"{name}: expected [B, rows, {feat * feat}], got {tuple(m.shape)}")
    return m


def decoder_heatmaps(dec_map, feat: int):
    """visualize_dec_features: query q's cross-attention over the memory tokens as an image.
    dec_map [B,Q,feat*feat] -> [B,Q,feat,feat] (a view)."""
    m = _check(dec_map, feat, "dec_map")
    return m.reshape(m.shape[0], m.shape[1], feat, feat)


def encoder_heatmaps_at(enc_map, points_norm, feat: int):
    """visualize_enc_features: for each predicted keypoint, the encoder self-attention that every token
    pays to the token under that keypoint.  The reference views the [T,T] map as [qy,qx,ky,kx] and
    shows [..., int(py), int(px)] with (px, py) = pred_points * feat: the image runs over the QUERY
    tokens, the keypoint picks the KEY token.
    enc_map [B,T,T], points_norm [B,Q,2] crop-normalised (x, y) in [0,1] -> [B,Q,feat,feat].
    A coordinate of exactly 1.0 (a saturated sigmoid) is clamped to the last cell, where the reference's
    index would fall outside the map."""
    m = _check(enc_map, feat, "enc_map")
    if m.shape[1] != feat * feat:
        raise ValueError(f"enc_map: expected [B, {feat * feat}, {feat * feat}], got {tuple(m.shape)}")
    p = torch.as_tensor(points_norm).to(device=m.device, dtype=torch.float32)
    if p.dim() != 3 or p.shape[0] != m.shape[0] or p.shape[2] != 2:
        raise ValueError(f"points_norm: expected [{m.shape[0]}, Q, 2], got {tuple(p.shape)}")
    cell = (p * feat).to(torch.int64).clamp_(0, feat - 1)          # int() truncates, like the reference
    key = cell[..., 1] * feat + cell[..., 0]                       # [B,Q]: token of (ky, kx)
    cols = torch.gather(m, 2, key[:, None, :].expand(-1, m.shape[1], -1))   # [B,T,Q]: every query's weight on it
    return cols.permute(0, 2, 1).reshape(m.shape[0], key.shape[1], feat, feat)
