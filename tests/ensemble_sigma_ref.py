"""numpy / Python fp64 restatement of the sigma-weighted ensemble fusion (include/spe.h
spe_ensemble_fuse_sigma), written from the header's text, not from the kernel: scalar Python loops over
Python floats (IEEE doubles) in the order the header states, one operation per expression, so there is
nothing for an interpreter to contract or reorder.  Also the synthetic inputs that
tests/test_ensemble_sigma.py and tests/test_gpu_ensemble_sigma.py share.

fuse_batch returns fp64 arrays: a caller that compares with the kernel rounds them to float32 itself.
"""
from __future__ import annotations

import math

import numpy as np


def _finite(v):
    return math.isfinite(v)


def label_and_score(row):
    """argmax of a probability row, the lower class on ties (a NaN never takes over)."""
    lab, sc = 0, row[0]
    for c in range(1, len(row)):
        if row[c] > sc:
            lab, sc = c, row[c]
    return lab, sc


def measurements(points, probs, sigmas, scale, sigma_floor):
    """One image.  points [M,Q,2], probs [M,Q,C], sigmas [M,Q,2] float32; scale (sx, sy) or None.
    -> {label: list over the models that carry it of dict(m, q, first, usable, x, y, sx, sy, score)}."""
    M, Q, C = probs.shape
    scx, scy = (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))
    scale_ok = _finite(scx) and _finite(scy) and scx > 0.0 and scy > 0.0
    out = {}
    for m in range(M):
        best = {}                                   # label -> [first q, best q, best score]
        for q in range(Q):
            lab, sc = label_and_score(probs[m, q])
            if lab == C - 1:
                continue
            if lab not in best:
                best[lab] = [q, q, sc]
            elif sc > best[lab][2]:
                best[lab][1], best[lab][2] = q, sc
        for lab, (first, q, sc) in best.items():
            x, y = float(points[m, q, 0]), float(points[m, q, 1])
            ux, uy = float(sigmas[m, q, 0]) * scx, float(sigmas[m, q, 1]) * scy
            usable = scale_ok and all(_finite(v) for v in (x, y, ux, uy, float(sc)))
            rec = dict(m=m, q=q, first=first, usable=usable, x=x, y=y, score=float(sc))
            if usable:
                rec["sx"] = max(ux, float(sigma_floor))
                rec["sy"] = max(uy, float(sigma_floor))
            out.setdefault(int(lab), []).append(rec)
    return out


def weighted_mean(kept):
    swx = swy = ax = ay = 0.0
    for r in kept:
        wx = 1.0 / (r["sx"] * r["sx"])
        wy = 1.0 / (r["sy"] * r["sy"])
        swx = swx + wx
        swy = swy + wy
        ax = ax + wx * r["x"]
        ay = ay + wy * r["y"]
    return ax / swx, ay / swy, swx, swy


def fuse_label(recs, gate, margins):
    """The usable measurements of one label, ascending model order -> (kept, mux, muy, swx, swy).
    Every gate decision's |largest d - gate| is appended to `margins`."""
    kept = list(recs)
    while True:
        mux, muy, swx, swy = weighted_mean(kept)
        if len(kept) < 3:
            break
        dmax, imax = -1.0, -1
        for i, r in enumerate(kept):
            dx = (r["x"] - mux) / r["sx"]
            dy = (r["y"] - muy) / r["sy"]
            d2 = dx * dx + dy * dy
            if d2 > dmax:
                dmax, imax = d2, i
        d = math.sqrt(dmax)
        margins.append(abs(d - gate))
        if not d > gate:
            break
        del kept[imax]
    return kept, mux, muy, swx, swy


def fuse_image(points, probs, sigmas, scale=None, sigma_floor=1e-3, gate=3.0):
    """-> rows: list of dict(label, x, y, sx, sy, score, n_pooled, n_kept, kept_models) in output order,
    and the list of gate margins."""
    M, Q, C = probs.shape
    gate = float(np.float32(gate))
    floor = float(np.float32(sigma_floor))
    meas = measurements(points, probs, sigmas, scale, floor)
    scx, scy = (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))
    rows, margins = [], []
    for lab, recs in meas.items():
        usable = [r for r in recs if r["usable"]]
        if not usable:
            continue
        kept, mux, muy, swx, swy = fuse_label(usable, gate, margins)
        n = len(kept)
        cx = cy = ss = 0.0
        for r in kept:
            wx = 1.0 / (r["sx"] * r["sx"])
            wy = 1.0 / (r["sy"] * r["sy"])
            ex = r["x"] - mux
            ey = r["y"] - muy
            cx = cx + wx * (ex * ex)
            cy = cy + wy * (ey * ey)
            ss = ss + r["score"]
        bx = by = 1.0
        if n > 1:
            bx = max(1.0, math.sqrt(cx / (n - 1)))
            by = max(1.0, math.sqrt(cy / (n - 1)))
        rows.append(dict(label=lab, x=mux, y=muy, sx=math.sqrt(1.0 / swx) * bx / scx,
                         sy=math.sqrt(1.0 / swy) * by / scy, score=ss / n, n_pooled=len(recs), n_kept=n,
                         kept_models=[r["m"] for r in kept],
                         seen=recs[0]["m"] * Q + recs[0]["first"]))
    rows.sort(key=lambda r: r["seen"])                   # first-seen order, model-major then by query
    return rows, margins


def fuse_batch(points, probs, sigmas, sigma_scale=None, sigma_floor=1e-3, gate=3.0):
    """points [M,B,Q,2], probs [M,B,Q,C], sigmas [M,B,Q,2] float32, sigma_scale [B,2] or None ->
    dict(points [B,K,2], probs [B,K,C], sigmas [B,K,2] fp64; n_pooled, n_kept [B,K] int32; labels: per image
    the emitted labels in row order; kept: per image and row the kept models; min_margin: the smallest
    |largest d - gate| over every gate decision, inf without one)."""
    points, probs, sigmas = (np.asarray(a, np.float32) for a in (points, probs, sigmas))
    M, B, Q, C = probs.shape
    K = C - 1
    o = dict(points=np.zeros((B, K, 2)), probs=np.zeros((B, K, C)), sigmas=np.zeros((B, K, 2)),
             n_pooled=np.zeros((B, K), np.int32), n_kept=np.zeros((B, K), np.int32), labels=[], kept=[])
    o["probs"][:, :, K] = 1.0
    margin = math.inf
    for b in range(B):
        sc = None if sigma_scale is None else np.asarray(sigma_scale, np.float32)[b]
        rows, margins = fuse_image(points[:, b], probs[:, b], sigmas[:, b], sc, sigma_floor, gate)
        margin = min([margin] + margins)
        for i, r in enumerate(rows):
            o["points"][b, i] = r["x"], r["y"]
            o["sigmas"][b, i] = r["sx"], r["sy"]
            o["probs"][b, i] = 0.0
            o["probs"][b, i, r["label"]] = r["score"]
            o["n_pooled"][b, i], o["n_kept"][b, i] = r["n_pooled"], r["n_kept"]
        o["labels"].append([r["label"] for r in rows])
        o["kept"].append([r["kept_models"] for r in rows])
    o["min_margin"] = margin
    return o


# ---------------------------------------------------------------- shared synthetic inputs
def simple_case(xs, sig, C=12, label=0, scores=None):
    """M models of one query each that all carry `label`: xs [M,2] points, sig [M,2] sigmas ->
    points [M,1,2], probs [M,1,C], sigmas [M,1,2] of one image."""
    xs = np.asarray(xs, np.float32).reshape(-1, 1, 2)
    M = len(xs)
    probs = np.full((M, 1, C), 0.01, np.float32)
    probs[:, 0, label] = 0.8 if scores is None else np.asarray(scores, np.float32)
    return xs, probs, np.broadcast_to(np.asarray(sig, np.float32).reshape(-1, 1, 2), (M, 1, 2)).copy()


def ensemble_inputs(M, B, Q, C, seed, scaled=False):
    """M models' outputs for B images with what the kernel must get right: labels that some models lack,
    a query that repeats a label with a bit-identical score (the earlier one must win) and one with a
    lower score before the selected one, a 40 px outlier with a small sigma among 3 or more models (gated),
    two of them where 6 or more models carry the label (two gate passes), an infinite and a NaN sigma, a
    sigma below the floor, and -- from B = 2 on -- an image that is all background (the last).  Honest
    sigmas otherwise: noise of the reported size, log-uniform in [0.3, 3] px per axis.
    -> points [M,B,Q,2], probs [M,B,Q,C], sigmas [M,B,Q,2] float32 (in units of `scale` when scaled),
    scale [B,2] float32 or None."""
    rng = np.random.default_rng(seed)
    K = C - 1
    pts = rng.uniform(0, 1900, (M, B, Q, 2)).astype(np.float32)
    probs = np.full((M, B, Q, C), 0.02, np.float32)
    probs[..., K] = 0.7                                       # background unless made a keypoint below
    sig_px = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (M, B, Q, 2)))
    scale = rng.uniform(150.0, 700.0, (B, 2)).astype(np.float32) if scaled else None
    for b in range(B):
        if B >= 2 and b == B - 1:
            continue
        truth = rng.uniform(100, 1800, (K, 2))
        where = {}                                            # (m, label) -> q
        for m in range(M):
            room = max(1, Q - 2)
            labs = [l for l in rng.permutation(K) if rng.random() < 0.85][:room] or [int(rng.integers(K))]
            slots = rng.permutation(Q)
            for l, q in zip(labs, slots[:len(labs)]):
                pts[m, b, q] = truth[l] + rng.normal(size=2) * sig_px[m, b, q]
                probs[m, b, q, K] = 0.02
                probs[m, b, q, l] = np.float32(rng.uniform(0.5, 0.95))
                where[(m, int(l))] = int(q)
            spare = [int(q) for q in slots[len(labs):]]
            if len(spare) >= 1:                               # the tie: same score, 40 px off
                l = int(labs[0])
                q0, q1 = where[(m, l)], spare[0]
                lo, hi = min(q0, q1), max(q0, q1)
                good, row, s = pts[m, b, q0].copy(), probs[m, b, q0].copy(), sig_px[m, b, q0].copy()
                probs[m, b, lo] = probs[m, b, hi] = row
                sig_px[m, b, lo] = sig_px[m, b, hi] = s
                pts[m, b, lo], pts[m, b, hi] = good, good + np.float32(40.0)
                where[(m, l)] = lo
            if len(spare) >= 2 and len(labs) >= 2:            # a lower score on another query of a label
                l = int(labs[1])
                q0, q1 = where[(m, l)], spare[1]
                probs[m, b, q1] = probs[m, b, q0]
                probs[m, b, q1, l] = probs[m, b, q0, l] * np.float32(0.5)
                probs[m, b, q1, K] = 0.02
                pts[m, b, q1] = pts[m, b, q0] - np.float32(55.0)
        carried = {l: [m for m in range(M) if (m, l) in where] for l in range(K)}
        many = [l for l in range(K) if len(carried[l]) >= 3]
        rng.shuffle(many)
        edits = ["outlier", "inf", "nan", "floor", "outlier"]
        for l, what in zip(many, edits):
            ms = carried[l]
            m = ms[int(rng.integers(len(ms)))]
            q = where[(m, l)]
            if what == "outlier":
                pts[m, b, q] += np.float32(40.0)
                sig_px[m, b, q] = 0.5
                if len(ms) >= 6:
                    m2 = [x for x in ms if x != m][0]
                    pts[m2, b, where[(m2, l)]] -= np.float32(60.0)
                    sig_px[m2, b, where[(m2, l)]] = 0.5
            elif what == "inf":
                sig_px[m, b, q, 1] = np.inf
            elif what == "nan":
                sig_px[m, b, q, 0] = np.nan
            else:
                sig_px[m, b, q] = 1e-5
    sig = sig_px if scale is None else sig_px / scale[None, :, None, :].astype(np.float64)
    return pts, probs, sig.astype(np.float32), scale


def pose_ensemble(M, B, Q, seed, clip, world, K):
    """M models' outputs for B images of one solvable pose each (C = 12): the keypoints of
    pose_covariance_ref.keypoint_set plus each model's own noise of its reported size (0.3 .. 1.5 px per
    axis), model 1 being 40 px off on one label per image with a sigma of 40 px; the scores differ by
    model.  clip [B,4]: the sigmas are returned crop-normalised (sigma_px / (width, height)).
    -> points [M,B,Q,2], probs [M,B,Q,12], sigmas [M,B,Q,2] float32."""
    import pose_covariance_ref as pc
    rng = np.random.default_rng(seed)
    base, probs0, _, _, _ = pc.keypoint_set(B, Q, 12, world, K, seed=seed, noise=0.0)
    clip = np.asarray(clip, np.float32)
    scale = np.stack([clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]], 1).astype(np.float64)
    sig_px = np.exp(rng.uniform(np.log(0.3), np.log(1.5), (M, B, Q, 2)))
    off = np.zeros((M, B, Q, 2))
    for b in range(B):
        q = int(rng.integers(min(Q, 11)))
        off[1 % M, b, q] = 40.0
        sig_px[1 % M, b, q] = 40.0
    pts = base[None] + rng.normal(size=(M, B, Q, 2)) * np.where(off != 0, 1.0, sig_px) + off
    probs = np.repeat(probs0[None], M, 0)
    for m in range(M):
        fg = probs[m] > 0.5
        probs[m][fg] = probs[m][fg] * np.float32(1.0 - 0.03 * m)
    return pts.astype(np.float32), probs.astype(np.float32), (sig_px / scale[None, :, None, :]).astype(np.float32)
