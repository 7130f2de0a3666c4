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


def rtdetr_decoder_heatmaps(dec_map, level_sizes):
    """The RT-DETR decoder map (RTDETR.forward_with_attention's "dec_map" [B,Q,L], tokens level-major, row-major
    inside a level) as images.  level_sizes: the side s_l of each level's map, finest first (maps["level_sizes"]).
    Returns (per_level, combined): per_level[l] is [B,Q,s_l,s_l] (a view); combined [B,Q,s_0,s_0] is every level
    on the finest grid, a coarser cell's weight spread equally over the k x k finest cells it covers (each gets
    weight / k^2, k = s_0 / s_l), so combined.sum((-1, -2)) == dec_map.sum(-1): the mass is kept."""
    sizes = [int(s) for s in level_sizes]
    m = torch.as_tensor(dec_map)
    if m.dim() != 3 or m.shape[-1] != sum(s * s for s in sizes):
        raise ValueError(f"dec_map: expected [B, Q, {sum(s * s for s in sizes)}], got {tuple(m.shape)}")
    if not sizes or any(s < 1 or sizes[0] % s for s in sizes):
        raise ValueError(f"level_sizes: sides dividing the finest one, got {sizes}")
    B, Q = m.shape[:2]
    per_level, start = [], 0
    for s in sizes:
        per_level.append(m[..., start:start + s * s].reshape(B, Q, s, s))
        start += s * s
    combined = torch.zeros(B, Q, sizes[0], sizes[0], dtype=m.dtype, device=m.device)
    for s, lv in zip(sizes, per_level):
        k = sizes[0] // s
        combined += (lv / (k * k)).repeat_interleave(k, dim=-2).repeat_interleave(k, dim=-1)
    return per_level, combined


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
