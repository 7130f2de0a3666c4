"""Restatements of the maps RTDETR.forward_with_attention exports (csrc/rtdetr.hip deform_map, csrc/attn_map.hip on
the AIFI layer).  Test infrastructure only.

The decoder map.  MSDeformableAttention (UNC/src/zoo/rtdetr/rtdetr_decoder.py:105-196, utils.py:15-64) reads, per
query and head, levels x points bilinear samples of the head's value maps and sums them with softmaxed weights w.
grid_sample (align_corners=False, zero padding) of one sample at pixel (ix, iy) is
    nw v[y0][x0] + ne v[y0][x0+1] + sw v[y0+1][x0] + se v[y0+1][x0+1],   corners off the map read 0,
so the head's output is A_h . value_h with A_h[q][t] = sum over the samples of w . (corner weight on cell t), and the
exported map is (1/H) sum_h A_h over the tokens of one image (level-major, y * W_l + x inside a level).  Dropped
corners make a row sum to <= 1.
"""
import numpy as np
import torch
import torch.nn.functional as F

import attention_map_ref
import rtdetr_ref

HEADS = 8


def splat(loc, weights, lvl_h, lvl_w):
    """loc [rows,H,NL,NP,2] normalised (x, y), weights [rows,H,NL,NP] -> (map [rows,L], per_head_A [rows,H,L]) in
    loc's dtype.  The pairs are added in (h, l, p, nw/ne/sw/se) order, like the kernel's list."""
    f = loc.dtype.type
    rows, H, NL, NP, _ = loc.shape
    Wl = np.asarray(lvl_w, loc.dtype).reshape(1, 1, NL, 1)
    Hl = np.asarray(lvl_h, loc.dtype).reshape(1, 1, NL, 1)
    start = np.concatenate([[0], np.cumsum([h * w for h, w in zip(lvl_h, lvl_w)])]).astype(np.int64)
    locx, locy = loc[..., 0], loc[..., 1]
    ix = ((f(2) * locx - f(1) + f(1)) * Wl - f(1)) / f(2)
    iy = ((f(2) * locy - f(1) + f(1)) * Hl - f(1)) / f(2)
    fx, fy = np.floor(ix), np.floor(iy)
    tx, ty = ix - fx, iy - fy
    # (far-away samples: every corner is off the map whatever the clip leaves of the index)
    x0 = np.clip(np.nan_to_num(fx), -4, 1 << 20).astype(np.int64)
    y0 = np.clip(np.nan_to_num(fy), -4, 1 << 20).astype(np.int64)
    nw, ne, sw, se = (f(1) - tx) * (f(1) - ty), tx * (f(1) - ty), (f(1) - tx) * ty, tx * ty
    Wi, Hi = Wl.astype(np.int64), Hl.astype(np.int64)
    toks, vals = [], []
    for y, x, bw in ((y0, x0, nw), (y0, x0 + 1, ne), (y0 + 1, x0, sw), (y0 + 1, x0 + 1, se)):
        inside = (x >= 0) & (x < Wi) & (y >= 0) & (y < Hi)
        toks.append(np.where(inside, start[:NL].reshape(1, 1, NL, 1) + y * Wi + x, -1))
        vals.append(np.where(inside, weights * bw, f(0)))
    tok, val = np.stack(toks, -1), np.stack(vals, -1).astype(loc.dtype)       # [rows,H,NL,NP,4]
    L = int(start[NL])
    r = np.broadcast_to(np.arange(rows).reshape(rows, 1, 1, 1, 1), tok.shape)
    h = np.broadcast_to(np.arange(H).reshape(1, H, 1, 1, 1), tok.shape)
    keep = tok >= 0
    A = np.zeros((rows, H, L), loc.dtype)
    np.add.at(A, (r[keep], h[keep], tok[keep]), val[keep])
    m = np.zeros((rows, L), loc.dtype)
    np.add.at(m, (r[keep], tok[keep]), val[keep])                            # C order: (row, h, l, p, corner)
    return m / f(H), A


def deform_map(so_aw, ref, Q, heads, levels, points, lvl_h, lvl_w, dtype=np.float64):
    """The kernel's inputs -> (map [rows,L], loc [rows,H,NL,NP,2], weights [rows,H,NL,NP], per_head_A [rows,H,L]),
    every operation in `dtype` (float64: the reference; float32: the same code, what fp32 arithmetic loses).
    so_aw [rows][>= 3 n], n = heads*levels*points: n (x, y) offsets then n logits; ref [rows][2]."""
    dt = np.dtype(dtype)
    so, ref = np.asarray(so_aw).astype(dt), np.asarray(ref).astype(dt)
    rows, n = so.shape[0], heads * levels * points
    off = so[:, :2 * n].reshape(rows, heads, levels, points, 2)
    lg = so[:, 2 * n:3 * n].reshape(rows, heads, levels * points)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    weights = (e / e.sum(-1, keepdims=True)).reshape(rows, heads, levels, points)
    norm = np.stack([np.asarray(lvl_w, dt), np.asarray(lvl_h, dt)], -1).reshape(1, 1, levels, 1, 2)
    loc = ref.reshape(rows, 1, 1, 1, 2) + off / norm
    m, A = splat(loc, weights, lvl_h, lvl_w)
    return m, loc, weights, A


def distance32(so_aw, ref, Q, heads, levels, points, lvl_h, lvl_w):
    """max |float32 restatement - float64 restatement| over map, loc and weights: what the GPU tolerance is 4 x of."""
    a = deform_map(so_aw, ref, Q, heads, levels, points, lvl_h, lvl_w, np.float64)
    b = deform_map(so_aw, ref, Q, heads, levels, points, lvl_h, lvl_w, np.float32)
    return max(float(np.abs(x - y.astype(np.float64)).max()) for x, y in zip(a[:3], b[:3]))


# ---- the kernel test's inputs (shared by tests/test_rtdetr_attention.py and tests/test_gpu_rtdetr_attention.py)
EDGE_LVL_H, EDGE_LVL_W = [5, 2, 1], [3, 4, 1]          # non-square levels 5x3, 2x4, 1x1 (H x W)
EDGE_ROWS, EDGE_Q, EDGE_POINTS = 7, 3, 4
ROW_INTERIOR = (0, 1)                                   # rows whose every sample has its four corners on the map
ROW_EDGES = 2


def _offset_for(pix, size, r):
    """the offset that puts the sample at pixel coordinate `pix` on an axis of `size` cells from reference r"""
    return ((pix + 0.5) / size - r) * size


def edge_case_inputs():
    """-> (so_aw [7][3*96] fp32, ref [7][2] fp32).  Rows 0, 1: every sample interior (reference point 0.5, 0.5; the
    1x1 level sampled at its centre), so the row sums to 1.  Row 2: head 0 / level 0 has a corner pair straddling the
    left, right, top and bottom edge; head 1 / level 0 a sample wholly off each edge; head 2 / level 1 a sample on an
    integer x (2.0), one on an integer y (1.0), and two samples in one cell; head 3 / level 2 samples off the 1x1
    level (two partly, two wholly; locations stay below 4 so that their fp32 ulp does not swamp the measured
    distance).  Rows 3..6: random reference points and offsets (inside and outside)."""
    g = np.random.default_rng(20)
    H, NL, NP = HEADS, 3, EDGE_POINTS
    off = np.zeros((EDGE_ROWS, H, NL, NP, 2))
    ref = np.full((EDGE_ROWS, 2), 0.5)
    half = np.array([[1.0, 2.0], [1.5, 0.5], [0.0, 0.0]])          # interior half-ranges of (off_x, off_y) per level
    off[:3] = g.uniform(-0.9, 0.9, off[:3].shape) * half.reshape(1, 1, NL, 1, 2)
    W0, H0 = EDGE_LVL_W[0], EDGE_LVL_H[0]
    for p, (ix, iy) in enumerate([(-0.7, 1.3), (2.4, 0.6), (1.2, -0.3), (0.8, 4.6)]):      # straddling each edge
        off[2, 0, 0, p] = _offset_for(ix, W0, 0.5), _offset_for(iy, H0, 0.5)
    for p, (ix, iy) in enumerate([(-1.5, 2.0), (3.2, 1.0), (1.0, -2.2), (1.5, 6.1)]):      # wholly off each edge
        off[2, 1, 0, p] = _offset_for(ix, W0, 0.5), _offset_for(iy, H0, 0.5)
    off[2, 2, 1, 0] = 0.5, 0.0               # W 4: locx 0.625, ix = 2.0 exactly; iy = 0.5
    off[2, 2, 1, 1] = -0.25, 0.5             # H 2: locy 0.75, iy = 1.0 exactly (its lower corners are off the map)
    off[2, 2, 1, 2] = 0.10, 0.10             # two samples in the cell (x 1, y 0): ix 1.6 / 1.65, iy 0.6 / 0.55
    off[2, 2, 1, 3] = 0.15, 0.05
    off[2, 3, 2] = [[0.7, 0.0], [0.0, -0.8], [3.0, 0.0], [-2.5, 3.0]]
    ref[3:] = g.uniform(0.0, 1.0, (EDGE_ROWS - 3, 2))
    off[3:] = g.normal(0.0, 1.5, off[3:].shape)
    logits = g.normal(0.0, 2.0, (EDGE_ROWS, H, NL * NP))
    so = np.concatenate([off.reshape(EDGE_ROWS, -1), logits.reshape(EDGE_ROWS, -1)], 1)
    return so.astype(np.float32), ref.astype(np.float32)


def single_case_inputs():
    """levels = 1, points = 1, one 1x1 level, 3 rows: every head's one weight is 1; samples near the cell centre,
    partly off it, and wholly off it."""
    g = np.random.default_rng(21)
    rows = 3
    ref = g.uniform(0.3, 0.7, (rows, 2))
    off = g.normal(0.0, 0.4, (rows, HEADS, 1, 1, 2))
    off[2, :4, 0, 0, 0] = 3.0
    logits = g.normal(0.0, 2.0, (rows, HEADS))
    return np.concatenate([off.reshape(rows, -1), logits], 1).astype(np.float32), ref.astype(np.float32)


# ---- the whole model: the oracle with its two attention functions wrapped
def oracle_rtdetr_maps(images, w, cfg):
    """Runs oracle/rtdetr_ref.py's forward with ms_deform_attn and mha wrapped (the oracle itself is not edited) and
    records, per decoder layer, the query's sampling offsets, softmaxed weights and reference points, and the AIFI
    layer's q / k inputs.  -> (out, enc_map [B,T5,T5] float64, dec_maps: per layer [B,Q,L] float64, rec), the maps
    restated in float64 from the oracle's fp32 records.  `out` is asserted equal to the plain forward's."""
    rec = {"deform": [], "mha": []}
    orig_ms, orig_mha = rtdetr_ref.ms_deform_attn, rtdetr_ref.mha

    def ms(query, ref, value_in, w_, p, cfg_):
        B, Lq, _ = query.shape
        Hn, nl, npt = cfg_.nheads, cfg_.num_levels, cfg_.num_points
        t = rtdetr_ref._t
        off = F.linear(query, t(w_, f"{p}.sampling_offsets.weight"), t(w_, f"{p}.sampling_offsets.bias"))
        aw = F.linear(query, t(w_, f"{p}.attention_weights.weight"), t(w_, f"{p}.attention_weights.bias"))
        aw = F.softmax(aw.reshape(B, Lq, Hn, nl * npt), dim=-1)
        rec["deform"].append(dict(off=off.reshape(B, Lq, Hn, nl, npt, 2), aw=aw.reshape(B, Lq, Hn, nl, npt),
                                  ref=ref.reshape(B, Lq, 2)))
        return orig_ms(query, ref, value_in, w_, p, cfg_)

    def mha(q_in, k_in, v_in, w_, p, nheads=8):
        rec["mha"].append(dict(p=p, q_in=q_in, k_in=k_in))
        return orig_mha(q_in, k_in, v_in, w_, p, nheads)

    rtdetr_ref.ms_deform_attn, rtdetr_ref.mha = ms, mha
    try:
        out = rtdetr_ref.forward(images, w, cfg)
    finally:
        rtdetr_ref.ms_deform_attn, rtdetr_ref.mha = orig_ms, orig_mha
    plain = rtdetr_ref.forward(images, w, cfg)
    assert all(torch.equal(out[k], plain[k]) for k in plain)
    assert len(rec["deform"]) == cfg.dec_layers and rec["mha"][0]["p"] == "encoder.encoder.0.layers.0.self_attn"
    a = rec["mha"][0]
    sd = {k: rtdetr_ref._t(w, a["p"] + k).double() for k in (".in_proj_weight", ".in_proj_bias")}
    sd = {a["p"] + k: v for k, v in sd.items()}
    enc_map = attention_map_ref.mha_weights_from_inputs(a["q_in"].double(), a["k_in"].double(), sd, a["p"], cfg.nheads)
    sizes = list(cfg.level_sizes)
    dec_maps = []
    for d in rec["deform"]:
        B, Q = d["ref"].shape[:2]
        norm = np.asarray(sizes, np.float64).reshape(1, 1, len(sizes), 1, 1)
        loc = d["ref"].double().numpy().reshape(B * Q, 1, 1, 1, 2) + d["off"].double().numpy().reshape(B * Q, *d["off"].shape[2:]) / norm
        m, _ = splat(loc, d["aw"].double().numpy().reshape(B * Q, *d["aw"].shape[2:]), sizes, sizes)
        dec_maps.append(m.reshape(B, Q, -1))
    return out, enc_map.numpy(), dec_maps, rec
