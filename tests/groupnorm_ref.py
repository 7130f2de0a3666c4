"""CPU restatement of the GroupNorm kernel contract (csrc/groupnorm.hip, spe_debug_groupnorm).  Test infrastructure only.

NHWC input x [B, H, W, C], 32 groups of C / 32 consecutive channels; per (image, group) the mean and the BIASED
variance over H * W * C / 32 elements; y = (x - mean) * rsqrt(var + 1e-5) * gamma[c] + beta[c], then the optional
residual add, then the optional ReLU (torchvision Bottleneck.forward's order with norm_layer = nn.GroupNorm(32, C)).

  group_norm(...)            the contract in float64 (or any numpy float type)
  group_norm_bf16(...)       bf16 storage: the bf16 inputs as they are stored, statistics and arithmetic in fp32,
                             ONE rounding to bf16 at the end
  welford_tiles(...)         the statistics the way the kernel takes them: a (count, mean, M2) triple per pixel tile,
                             merged with Chan's update -- pinned against F.group_norm by tests/test_groupnorm.py
  one_pass_f32(...)          the variance a one-pass E[x^2] - E[x]^2 in fp32 gives (what the kernel must NOT do)
"""
from __future__ import annotations

import numpy as np
import torch

GROUPS = 32
EPS = 1e-5
TILE_ELEMS = 16384            # elements of one statistics tile: TILE_ELEMS / C pixels (include/spe.h)


def tiles(H, W, C):
    pt = TILE_ELEMS // C
    return (H * W + pt - 1) // pt


def to_bf16(a):
    """float array -> the nearest bf16 values (round to nearest even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def bf16_bits(a):
    """bf16-valued float32 array -> its int32 bit patterns >> 16, monotone in the value (for ulp distances)"""
    u = np.ascontiguousarray(a, np.float32).view(np.int32) >> 16
    return np.where(u < 0, -(u & 0x7FFF), u)


def stats(x, dtype=np.float64):
    """x [B, H, W, C] -> (mean, biased var), each [B, 32]"""
    B, H, W, C = x.shape
    g = np.asarray(x, dtype).reshape(B, H * W, GROUPS, C // GROUPS).transpose(0, 2, 1, 3).reshape(B, GROUPS, -1)
    return g.mean(-1), g.var(-1)


def _finish(x, mean, var, gamma, beta, residual, relu, dtype):
    B, H, W, C = x.shape
    cpg = C // GROUPS
    mean_c = np.repeat(np.asarray(mean, dtype), cpg, axis=1)[:, None, None, :]
    rstd_c = np.repeat((1.0 / np.sqrt(np.asarray(var, dtype) + dtype(EPS))).astype(dtype), cpg, axis=1)[:, None, None, :]
    y = (np.asarray(x, dtype) - mean_c) * (rstd_c * np.asarray(gamma, dtype)) + np.asarray(beta, dtype)
    if residual is not None:
        y = y + np.asarray(residual, dtype)
    return np.maximum(y, 0) if relu else y


def group_norm(x, gamma, beta, residual=None, relu=False, dtype=np.float64):
    mean, var = stats(x, dtype)
    return _finish(x, mean, var, gamma, beta, residual, relu, dtype)


def group_norm_bf16(x, gamma, beta, residual=None, relu=False):
    """x and residual hold bf16 values.  Statistics in float64 rounded to fp32 (an fp32 accumulation that loses no
    digits to cancellation agrees with that to a few fp32 ulps), the affine, residual and ReLU in fp32, one bf16 rounding."""
    mean, var = stats(x, np.float64)
    y = _finish(x, mean.astype(np.float32), var.astype(np.float32), gamma, beta, residual, relu, np.float32)
    return to_bf16(y)


def chan_merge(a, b):
    """(n, mean, M2) of the union of two disjoint sets (arrays broadcast); either side may be empty"""
    na, ma, qa = a
    nb, mb, qb = b
    n = na + nb
    r = np.where(n > 0, nb / np.maximum(n, 1), 0.0)
    d = mb - ma
    return n, ma + d * r, qa + qb + d * d * na * r


def welford_tiles(x, dtype=np.float64):
    """(mean, biased var) [B, 32] from per-tile triples merged in tile order, the tiles being the kernel's"""
    B, H, W, C = x.shape
    cpg, pt = C // GROUPS, TILE_ELEMS // C
    rows = np.asarray(x, dtype).reshape(B, H * W, GROUPS, cpg)
    acc = (np.zeros((B, GROUPS), dtype), np.zeros((B, GROUPS), dtype), np.zeros((B, GROUPS), dtype))
    for p0 in range(0, H * W, pt):
        t = rows[:, p0:p0 + pt].transpose(0, 2, 1, 3).reshape(B, GROUPS, -1)
        m = t.mean(-1)
        acc = chan_merge(acc, (np.full((B, GROUPS), t.shape[-1], dtype), m, ((t - m[..., None]) ** 2).sum(-1)))
    return acc[1], acc[2] / acc[0]


def one_pass_f32(x):
    """(mean, var) [B, 32] as E[x^2] - E[x]^2 with fp32 running sums in element order"""
    B, H, W, C = x.shape
    g = np.asarray(x, np.float32).reshape(B, H * W, GROUPS, C // GROUPS).transpose(0, 2, 1, 3).reshape(B, GROUPS, -1)
    s = np.cumsum(g, axis=-1, dtype=np.float32)[..., -1]
    q = np.cumsum(g * g, axis=-1, dtype=np.float32)[..., -1]
    n = np.float32(g.shape[-1])
    mean = s / n
    return mean, q / n - mean * mean
