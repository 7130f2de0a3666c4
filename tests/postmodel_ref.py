"""References and seeded cases for the kernels that run after the model (the ensemble fusion, the DETR
set criterion, the solver's front end), shared by tests/test_postmodel_ref.py (CPU pins) and
tests/test_gpu_postmodel_edges.py (device).

The ensemble reference here calls numpy and scipy themselves, like the reference's mean_and_filter
(REV/utils/speed_eval.py:54-71): `p.mean(0)` on the float32 points, scipy's cdist for the fp64
distances, `np.std` on them and `p[keep].mean(0)`.  It shares no summation code with
oracle/ensemble_ref.py, whose restated sums (and through them the kernel's) it pins.
"""
import warnings

import numpy as np

from spe.config import project, world_points

# ---------------------------------------------------------------- ensemble fusion
POOL_SIZES = (1, 2, 3, 7, 8, 9, 127, 128, 129, 136, 200, 255, 256)


def mean_and_filter_numpy(points):
    """points float32 [n, 2] of one label -> fused float32 [2], by numpy / scipy directly."""
    from scipy.spatial.distance import cdist
    p = np.asarray(points, np.float32)
    m = p.mean(0)
    if len(p) < 3:
        return m
    d = cdist(p, m[None]).flatten()
    keep = d < np.std(d) * 3
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)      # the mean of an empty selection is NaN
        return p[keep].mean(0)


def fuse_batch_numpy(multi_points, multi_probs):
    """[M,B,Q,2], [M,B,Q,C] -> (points [B,C-1,2], one-hot probs [B,C-1,C]): labels by argmax, background
    (C - 1) dropped, pooled per label in model-then-query order, labels in first-seen order."""
    mp, mr = np.asarray(multi_points, np.float32), np.asarray(multi_probs, np.float32)
    M, B, Q, C = mr.shape
    pts = np.zeros((B, C - 1, 2), np.float32)
    prb = np.zeros((B, C - 1, C), np.float32)
    prb[:, :, C - 1] = 1.0
    lab = mr.argmax(-1)
    for b in range(B):
        pool = {}                                            # insertion order = first-seen order
        for m in range(M):
            for q in range(Q):
                if lab[m, b, q] != C - 1:
                    pool.setdefault(int(lab[m, b, q]), []).append(mp[m, b, q])
        for i, (l, rows) in enumerate(pool.items()):
            pts[b, i] = mean_and_filter_numpy(np.stack(rows))
            prb[b, i] = 0.0
            prb[b, i, l] = 1.0
    return pts, prb


def pool_points(rng, n, spread=3.0, outliers=0.05):
    """n float32 pixel points around one landmark, a few of them gross outliers."""
    p = rng.normal(0.0, spread, (n, 2)) + rng.uniform(200, 1700, 2)
    far = rng.random(n) < outliers
    p[far] += rng.uniform(-300, 300, (int(far.sum()), 2))
    return p.astype(np.float32)


def one_hot(labels, C, hi=0.9, lo=0.01):
    """labels int [...] -> probs [..., C] whose argmax is the label."""
    labels = np.asarray(labels)
    p = np.full(labels.shape + (C,), lo, np.float32)
    np.put_along_axis(p, labels[..., None], np.float32(hi), -1)
    return p


def _random_case(seed, M, B, Q, C, bg=0.15):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C - 1, (M, B, Q))
    lab[rng.random((M, B, Q)) < bg] = C - 1
    centre = rng.uniform(200, 1700, (B, C, 2))
    pts = centre[np.arange(B)[None, :, None], lab] + rng.normal(0, 3.0, (M, B, Q, 2))
    far = rng.random((M, B, Q)) < 0.05
    pts[far] += rng.uniform(-300, 300, (int(far.sum()), 2))
    prb = one_hot(lab, C, hi=0.9)
    prb[..., 0] += rng.uniform(0, 0.3, (M, B, Q)).astype(np.float32)      # scores differ, argmax unchanged
    return pts.astype(np.float32), prb


def _single_label(seed, M, Q, C, label, n, B=2):
    """The first n of the M * Q pooled slots (model-then-query order) take `label`, the rest background."""
    rng = np.random.default_rng(seed)
    lab = np.full((M, B, Q), C - 1)
    pts = np.zeros((M, B, Q, 2), np.float32)
    for b in range(B):
        flat = np.full(M * Q, C - 1)
        flat[:n] = label
        lab[:, b] = flat.reshape(M, Q)
        p = rng.uniform(0, 1900, (M * Q, 2))                             # background points: never pooled
        p[:n] = pool_points(rng, n)
        pts[:, b] = p.reshape(M, Q, 2)
    return pts, one_hot(lab, C)


def ensemble_cases():
    """name -> (points [M,B,Q,2], probs [M,B,Q,C]): the shapes and pools at which spe_ensemble_fuse's
    indexing, its d[256] buffer and its pooling order can go wrong (M * Q <= 256, C <= 17)."""
    cases = {"m4_q64": _random_case(1, 4, 3, 64, 12),                     # M * Q = 256, about 20 points a label
             "m16_q16": _random_case(2, 16, 3, 16, 12),
             "one_label_256": _single_label(3, 4, 64, 12, 5, 256),        # d[] exactly full
             "one_label_129": _single_label(4, 3, 43, 12, 3, 129),        # first size past one sum block
             "one_label_255": _single_label(5, 5, 51, 12, 0, 255),        # second half (135) splits again
             "c2": _random_case(6, 5, 3, 7, 2, bg=0.4),
             "b1": _random_case(7, 2, 1, 11, 12), "b64": _random_case(8, 2, 64, 11, 12),
             "b65": _random_case(9, 2, 65, 11, 12)}
    # C = 17, every one of the 16 labels seen, first in an order that is not sorted
    pts, prb = _random_case(10, 3, 2, 20, 17, bg=0.1)
    first = np.array([9, 3, 15, 0, 12, 7, 1, 14, 5, 10, 2, 8, 13, 4, 11, 6])
    prb[0, :, :16] = one_hot(np.broadcast_to(first, (2, 16)), 17)
    cases["c17_all_labels"] = (pts, prb)
    # labels with exactly 1, 2 and 3 points (3 is the first size that filters); the rest background
    rng = np.random.default_rng(11)
    lab = np.full((3, 2, 4), 11)
    lab[0, :, 0] = 4                                                     # label 4: one point
    lab[0, :, 1] = lab[2, :, 3] = 7                                      # label 7: two
    lab[0, :, 2] = lab[1, :, 0] = lab[2, :, 0] = 1                       # label 1: three
    cases["pools_of_1_2_3"] = (rng.uniform(100, 1800, (3, 2, 4, 2)).astype(np.float32), one_hot(lab, 12))
    # a label whose 4 points coincide (std 0 -> NaN) beside an ordinary one; image 1 without foreground
    pts, prb = _random_case(12, 4, 3, 6, 12, bg=0.0)
    lab = np.full((4, 3, 6), 11)
    lab[:, 0, 2] = 8
    lab[:, 0, 4] = 2
    lab[:, 2, :3] = 6
    pts[:, 0, 2] = np.float32([1234.5, 321.25])
    cases["coincide_and_no_foreground"] = (pts, one_hot(lab, 12))
    # argmax ties: the first class wins (a row of equal probabilities is class 0; foreground 3 beats
    # the background it ties with)
    pts, prb = _random_case(13, 3, 2, 5, 12)
    prb[0, :, 0] = np.float32(1.0 / 12)
    prb[1, :, 1] = 0.01
    prb[1, :, 1, 3] = prb[1, :, 1, 11] = 0.45
    cases["argmax_ties"] = (pts, prb)
    return cases


# ---------------------------------------------------------------- DETR set criterion
CRITERION_SHAPES = [(64, 32, 12), (64, 1, 12), (32, 32, 12), (1, 1, 12), (33, 32, 32), (40, 11, 12), (11, 11, 2)]


def criterion_case(seed, L, B, Q, T, C):
    """Random logits, points and targets in [0, 1]: logits [L,B,Q,C], points [L,B,Q,2], labels [B,T]
    (background excluded), target points [B,T,2].

    Two targets of one label share their class cost, and the L1 point cost of swapping their queries is
    exactly zero in real arithmetic whenever both queries lie on one side of both targets in x and in y
    (|a - s| - |a - t| is constant outside [s, t]).  Such a pair is decided by the last bit of
    cost_pts * cp + cost_class * cc, which moves with the last bit of the softmax, and fp32 exp is not
    the same function in numpy, torch and the device library.  So the labels of an image are distinct
    wherever T <= C - 1 allows it (normal logits), and where duplicates are forced (T = 32 with 11 or 31
    labels, C = 2) every logit is 0 or -200: exp(-200) is exactly 0 in fp32, the softmax is exactly 1 / k
    or 0 in every implementation, still different from query to query and class to class, and every
    cost entry of the device equals the oracle's bit for bit -- the uniform-logits argument of the tie
    cases (criterion_tie_case), with a softmax that is not constant."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(0, 1, (L, B, Q, 2)).astype(np.float32)
    tpts = rng.uniform(0, 1, (B, T, 2)).astype(np.float32)
    if T <= C - 1:
        logits = rng.normal(0, 2.0, (L, B, Q, C)).astype(np.float32)
        labels = np.stack([rng.permutation(C - 1)[:T] for _ in range(B)]).astype(np.int64)
    else:
        logits = np.where(rng.random((L, B, Q, C)) < 0.3, 0.0, -200.0).astype(np.float32)
        labels = rng.integers(0, C - 1, (B, T)).astype(np.int64)
    return logits, points, labels, tpts


def criterion_tie_case(kind, Q, T, B=16, C=12, seed=0):
    """Exact cost ties under uniform logits (softmax exactly 1 / C everywhere): 'queries' -- queries 2k
    and 2k + 1 identical; 'targets' -- targets 0 and 1 identical (label and point); 'labels' -- every
    target carries one of two labels, points all different."""
    rng = np.random.default_rng(seed + 17 * Q + T)
    logits = np.zeros((1, B, Q, C), np.float32)
    points = rng.uniform(0, 1, (1, B, Q, 2)).astype(np.float32)
    labels = np.stack([rng.permutation(C - 1)[:T] for _ in range(B)]).astype(np.int64)
    tpts = rng.uniform(0, 1, (B, T, 2)).astype(np.float32)
    if kind == "queries":
        points[:, :, 1::2] = points[:, :, 0:2 * (Q // 2):2]
    elif kind == "targets":
        labels[:, 1] = labels[:, 0]
        tpts[:, 1] = tpts[:, 0]
    else:
        labels = rng.integers(3, 5, (B, T)).astype(np.int64)
    return logits, points, labels, tpts


def tie_matrices(shape, seed):
    """Cost matrices with repeated rows and repeated columns (fp64, drawn from a few values)."""
    rng = np.random.default_rng(seed)
    nr, nc = shape
    out = []
    for k in range(6):
        c = rng.integers(0, 5, shape).astype(np.float64) if k % 2 else rng.normal(size=shape)
        rows = rng.integers(0, max(1, nr // 2), nr) if k < 4 else np.arange(nr)     # row i copies row rows[i]
        cols = rng.integers(0, max(1, nc // 2), nc) if k >= 2 else np.arange(nc)
        out.append(np.ascontiguousarray(c[rows][:, cols]))
    return out


# ---------------------------------------------------------------- solver front end
# Five more landmarks for num_classes = 17 (16 labels = the solver's MAXN): fixed, off the planes of the
# 11 real ones (z about 0.25, 0.32 and 0.0) and of each other.
EXTRA_WORLD = np.array([[0.10, 0.05, 0.55], [-0.20, 0.15, -0.30], [0.45, -0.10, 0.12],
                        [-0.05, -0.50, -0.15], [0.25, 0.60, 0.40]], np.float64)


def world16():
    return np.vstack([world_points(), EXTRA_WORLD])


def world_for(C):
    return world16() if C == 17 else world_points()


def solver_set(B, Q, C, seed):
    """tests/helpers.solver_stress_set on the landmarks of `C` classes, plus per-image thresholds for
    the EPnP-Ceres mode: (points, probs, q, t, sigmas, repro_per_image)."""
    from helpers import solver_stress_set
    pts, probs, q, t, sig = solver_stress_set(B, seed=seed, Q=Q, C=C, world=world_for(C))
    th = np.random.default_rng(seed + 1000).choice(np.array([1.5, 4.0, 9.0, 20.0], np.float32), B)
    return pts, probs, q, t, sig, th.astype(np.float32)


def clean_projection(q, t, labels, C):
    """Exact projections of the landmarks `labels` ([Q], C - 1 = background -> the origin's projection)."""
    W = world_for(C)
    lm = project(W, q, t)
    return np.stack([lm[l] if l < C - 1 else project(np.zeros((1, 3)), q, t)[0] for l in labels]).astype(np.float32)
