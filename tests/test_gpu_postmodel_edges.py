"""The kernels that run after the model, at the limits of their C contracts (include/spe.h): the
ensemble fusion (csrc/ensemble.hip), the DETR set criterion (csrc/criterion.hip) and the solver's
front end -- correspondence selection, self-assessment and SPEED score (csrc/pnp.hip).

References: the numpy-direct fusion of tests/postmodel_ref.py, oracle/criterion_ref.criterion and
oracle/pnp_ref (the C oracle, which takes Q and C from the array shapes); all three are pinned on the
CPU in tests/test_postmodel_ref.py, tests/test_criterion.py and tests/test_reference_front.py.
Bounds are the project's existing ones: integer outputs and the fusion bit-exact (NaN for NaN),
losses 1e-5 * max(1, |v|) (tests/test_criterion.py), poses |dq| <= 1e-5 and |dt| / |t| <= 1e-6
(tests/test_gpu_parity.py).  Every refusal is checked to come back SPE_E_ARG with the output
buffers, pre-filled with a sentinel, untouched.

What the fusion's device cases can and cannot see.  The fused point depends on the standard
deviation only through the decisions d < 3 * sd, so a last-bit error in the kernel's fp64 sums shows
on the device only when it flips one, which random inputs practically never do (the distances move
in steps of about 2^-24 of their size with the float32 inputs, the window is about 2^-52 of it).
The guard for the arithmetic is therefore the CPU pin of the restated sums against np.add.reduce
(test_postmodel_ref.test_pairwise_sum_is_numpys), which the kernel's pairwise_sum follows line by
line; the device cases guard the indexing, the d[256] buffer, the split points of the sum (a wrong
offset there moves sd by far more than a bit) and the order of pooling.  An input on which the
one-block sum and numpy's split sum select different points needs a distance within about 2^-52 of
3 * sd, some 2^28 draws at the float32 inputs' step: none was constructed, so none is a case here.
"""
import numpy as np
import pytest

import criterion_ref as cr
import postmodel_ref as pr

pytestmark = pytest.mark.gpu

SPE_E_ARG = -1
FILL = -7


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _filled(shape, dtype, dev):
    import torch
    return torch.full(shape, FILL, dtype=dtype, device=dev)


def _untouched(*tensors):
    return all(bool((t == FILL).all()) for t in tensors)


# ================================================================ A. ensemble fusion
def call_fuse(dev, pts, prb, M=None, B=None, Q=None, C=None):
    """spe_ensemble_fuse on [M,B,Q,2] / [M,B,Q,C]; the size arguments override the arrays' (refusals,
    B = 0).  Outputs start filled with the sentinel.  -> rc, fused points, fused probs (device)."""
    import torch
    from spe import _lib
    m, b, q, c = prb.shape
    M, B, Q, C = (m if M is None else M), (b if B is None else B), (q if Q is None else Q), (c if C is None else C)
    fp = _filled((max(B, b), max(C, c) - 1, 2), torch.float32, dev)
    fr = _filled((max(B, b), max(C, c) - 1, max(C, c)), torch.float32, dev)
    p, r = _dev(pts, dev), _dev(prb, dev)
    rc = _lib.lib().spe_ensemble_fuse(_lib.stream_ptr(), _lib.ptr(p), _lib.ptr(r), M, B, Q, C, _lib.ptr(fp), _lib.ptr(fr))
    torch.cuda.synchronize()
    return rc, fp, fr


_fusion_ref = {}


def fusion_ref(name):
    if not _fusion_ref:
        for k, (pts, prb) in pr.ensemble_cases().items():
            _fusion_ref[k] = (pts, prb) + pr.fuse_batch_numpy(pts, prb)
    return _fusion_ref[name]


@pytest.mark.parametrize("name", sorted(pr.ensemble_cases()))
def test_fusion_is_numpy_direct(gpu_device, name):
    pts, prb, rp, rr = fusion_ref(name)
    rc, fp, fr = call_fuse(gpu_device, pts, prb)
    assert rc == 0
    np.testing.assert_array_equal(fr.cpu().numpy(), rr)
    got = fp.cpu().numpy()
    assert np.array_equal(got, rp, equal_nan=True), np.argwhere(~((got == rp) | (np.isnan(got) & np.isnan(rp))))
    if name == "coincide_and_no_foreground":
        assert np.isnan(got[0, 0]).all() and not np.isnan(got[0, 1:]).any() and (got[1] == 0).all()


def test_fusion_of_an_empty_batch_touches_nothing(gpu_device):
    pts, prb, _, _ = fusion_ref("b1")
    rc, fp, fr = call_fuse(gpu_device, pts, prb, B=0)
    assert rc == 0 and _untouched(fp, fr)


@pytest.mark.parametrize("case", ["mq257", "m257_q1", "c18", "c1", "q0"])
def test_fusion_refusals(gpu_device, case):
    from spe import _lib
    M, Q, C = {"mq257": (1, 257, 12), "m257_q1": (257, 1, 12), "c18": (2, 11, 18), "c1": (2, 11, 1), "q0": (2, 0, 12)}[case]
    pts = np.zeros((M, 2, max(Q, 1), 2), np.float32)
    prb = np.zeros((M, 2, max(Q, 1), max(C, 2)), np.float32)
    rc, fp, fr = call_fuse(gpu_device, pts, prb, Q=Q, C=C)
    assert rc == SPE_E_ARG and b"bad argument" in _lib.lib().spe_last_error()
    assert _untouched(fp, fr)


# ================================================================ B. DETR set criterion
def call_criterion(dev, logits, points, labels, tpts, num_points=None, Q=None, T=None, C=None):
    """spe_criterion on logits [L,B,Q,C], points [L,B,Q,2], labels [B,T], target points [B,T,2]; Q / T / C
    override the arrays' sizes (refusals).  -> rc, match [L,B,T], losses [L,4] (numpy), untouched flag."""
    import torch
    from spe import _lib
    L, B, q, c = logits.shape
    t = labels.shape[1]
    Q, T, C = (q if Q is None else Q), (t if T is None else T), (c if C is None else C)
    match = _filled((L, B, max(T, t)), torch.int32, dev)
    res = _filled((L, 4), torch.float64, dev)
    args = [_dev(logits, dev), _dev(points, dev), _dev(labels.astype(np.int32), dev), _dev(tpts, dev)]
    rc = _lib.lib().spe_criterion(_lib.stream_ptr(), *[_lib.ptr(a) for a in args], L, B, Q, C, T, 1.0, 5.0, 0.1,
                                  float(B * T) if num_points is None else num_points, _lib.ptr(match), _lib.ptr(res))
    torch.cuda.synchronize()
    return rc, match.cpu().numpy(), res.cpu().numpy(), _untouched(match, res)


def close(a, b):
    return abs(a - b) <= 1e-5 * max(1.0, abs(b))


def check_criterion(dev, logits, points, labels, tpts, num_points=None, ref_labels=None, solver=cr.lsap):
    """Device against oracle/criterion_ref.criterion: matching exact, the four losses of every layer
    within the bound.  ref_labels: what the oracle sees in place of `labels`."""
    L = logits.shape[0]
    ref, match = cr.criterion([(logits[l], points[l]) for l in range(L)], labels if ref_labels is None else ref_labels,
                              tpts, num_points=num_points, solver=solver)
    rc, m, v, _ = call_criterion(dev, logits, points, labels, tpts, num_points)
    assert rc == 0
    np.testing.assert_array_equal(m, match)
    for l in range(L):
        sfx = "" if l == L - 1 else f"_{l}"
        for i, k in enumerate(("loss_ce", "class_error", "cardinality_error", "loss_points")):
            if k + sfx in ref:                               # class_error: last layer only
                assert close(v[l, i], ref[k + sfx]), (l, k, v[l, i], ref[k + sfx])
    return m, v


@pytest.mark.parametrize("L,B", [(1, 1), (6, 1), (1, 37), (6, 37)])
@pytest.mark.parametrize("Q,T,C", pr.CRITERION_SHAPES)
def test_criterion_shapes(gpu_device, Q, T, C, L, B):
    """Both orientations of the cost matrix (Q > T transposed), the full LDS arrays (Q = 64 with T = 32,
    C = 32), one row / one column, and the per-layer, per-image indexing.  Normal logits where an image's
    labels can be distinct, 0 / -200 logits where duplicates are forced (postmodel_ref.criterion_case says why)."""
    from scipy.optimize import linear_sum_assignment
    logits, points, labels, tpts = pr.criterion_case(1000 * Q + 10 * T + C + L + B, L, B, Q, T, C)
    # scipy itself as the oracle's assignment (oracle/criterion_ref.lsap is pinned to it; the pure-Python
    # restatement takes seconds at 6 x 37 images of 64 x 32)
    m, _ = check_criterion(gpu_device, logits, points, labels, tpts, solver=linear_sum_assignment)
    assert (m >= 0).all() and (m < Q).all()
    for row in m.reshape(-1, T):
        assert len(set(row)) == T                            # a matching: no query twice


@pytest.mark.parametrize("Q,T", [(8, 8), (12, 5)])
@pytest.mark.parametrize("kind", ["queries", "targets", "labels"])
def test_criterion_exact_ties(gpu_device, kind, Q, T):
    """Exactly equal costs: scipy's tie-break order decides, square and transposed."""
    check_criterion(gpu_device, *pr.criterion_tie_case(kind, Q, T))


def test_criterion_num_points(gpu_device):
    """num_points other than B * T divides loss_points and nothing else."""
    logits, points, labels, tpts = pr.criterion_case(5, 2, 3, 11, 11, 12)
    _, v0 = check_criterion(gpu_device, logits, points, labels, tpts)
    m1, v1 = check_criterion(gpu_device, logits, points, labels, tpts, num_points=7.5)
    np.testing.assert_array_equal(v1[:, :3], v0[:, :3])
    for l in range(2):
        assert close(v1[l, 3] * 7.5, v0[l, 3] * 33.0) and v1[l, 3] > 4 * v0[l, 3]


@pytest.mark.parametrize("case", ["q65", "t33", "t_gt_q", "c33", "c1", "num_points_0", "num_points_nan"])
def test_criterion_refusals(gpu_device, case):
    from spe import _lib
    Q, T, C, npts = {"q65": (65, 11, 12, None), "t33": (64, 33, 12, None), "t_gt_q": (5, 6, 12, None),
                     "c33": (30, 11, 33, None), "c1": (30, 11, 1, None), "num_points_0": (11, 11, 12, 0.0),
                     "num_points_nan": (11, 11, 12, float("nan"))}[case]
    logits, points, labels, tpts = pr.criterion_case(3, 1, 2, Q, T, max(C, 2))
    rc, _, _, untouched = call_criterion(gpu_device, logits, points, labels, tpts, num_points=npts, C=C)
    assert rc == SPE_E_ARG and b"bad argument" in _lib.lib().spe_last_error()
    assert untouched


@pytest.mark.parametrize("Q,T,C", [(11, 11, 12), (40, 11, 12), (33, 32, 32)])
def test_criterion_out_of_range_labels_count_as_no_object(gpu_device, Q, T, C):
    """A target label outside [0, C) is class C - 1 (include/spe.h), as in spe_criterion_sigma: equal to
    the oracle on the clamped labels, in the cost, the cross entropy and the class error."""
    logits, points, labels, tpts = pr.criterion_case(7 + Q, 2, 5, Q, T, C)
    # one per image, so that no image gains two targets of one class (postmodel_ref.criterion_case)
    labels[0, 0], labels[1, T // 2], labels[2, -1], labels[3, 0], labels[4, 1] = -1, C, 2 ** 31 - 1, -2 ** 31, C + 5
    clamped = np.where((labels >= 0) & (labels < C), labels, C - 1)
    assert (clamped != labels).sum() == 5
    check_criterion(gpu_device, logits, points, labels, tpts, ref_labels=clamped)


# ================================================================ C. solver front end
MODES = [0, 1, 2, 3, 4]
SOLVER_SHAPES = [(64, 12), (40, 12), (30, 17), (64, 17), (4, 12), (1, 12)]
OUT_KEYS = ("quat", "tvec", "rvec", "status", "n_corr", "corr_label", "inlier_mask")


def mode_args(mode, sig, th):
    """(sigmas, repro, repro_per_image) as each mode is run: sigma modes take the sigmas, EPnP-Ceres the
    per-image thresholds."""
    return (sig if mode in (2, 4) else None), (25.0 if mode == 2 else 20.0), (th if mode == 4 else None)


def call_pnp(dev, pts, probs, C_world, mode, sig=None, repro=20.0, th=None, iters=100, conf=0.99, nulls=False,
             B=None, Q=None, C=None):
    """spe_pnp_batch through ctypes.  nulls: every nullable output NULL.  B / Q / C override the arrays'
    sizes.  -> rc, dict of device tensors (sentinel-filled before the call)."""
    import torch
    from spe import _lib
    from spe.config import Camera
    b, q, c = probs.shape
    B, Q, C = (b if B is None else B), (q if Q is None else Q), (c if C is None else C)
    n = max(B, b, 1)
    out = dict(quat=_filled((n, 4), torch.float32, dev), tvec=_filled((n, 3), torch.float64, dev),
               rvec=_filled((n, 3), torch.float64, dev), status=_filled((n,), torch.int32, dev),
               n_corr=_filled((n,), torch.int32, dev), corr_label=_filled((n, 16), torch.int32, dev),
               inlier_mask=_filled((n,), torch.int32, dev))
    ins = [_dev(pts, dev), _dev(probs, dev), None if sig is None else _dev(sig, dev)]
    K, W = _dev(Camera.K, dev), _dev(pr.world_for(C_world), dev)
    thd = None if th is None else _dev(th, dev)
    opt = [None if nulls else _lib.ptr(out[k]) for k in OUT_KEYS[2:]]
    rc = _lib.lib().spe_pnp_batch(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], B, Q, C, _lib.ptr(K), _lib.ptr(W), mode,
                                  repro, iters, conf, _lib.ptr(out["quat"]), _lib.ptr(out["tvec"]), *opt, _lib.ptr(thd))
    torch.cuda.synchronize()
    return rc, out


def check_solve(h, o):
    """Device dict (numpy) against the oracle's: discrete outputs exact, poses within the bounds where
    the oracle has one, zero elsewhere.  -> the mask of images with a pose."""
    np.testing.assert_array_equal(h["status"], o["status"])
    np.testing.assert_array_equal(h["n_corr"], o["n_corr"])
    np.testing.assert_array_equal(h["corr_label"], o["corr_label"])
    np.testing.assert_array_equal(h["inlier_mask"].astype(np.uint32), o["inlier_mask"])
    ok = (o["status"] == 0) | (o["status"] == 3)
    if ok.any():
        dq = np.abs(np.abs((h["quat"].astype(np.float64) * o["quat"]).sum(1)) - 1)
        assert dq[ok].max() <= 1e-5
        dt = np.linalg.norm(h["tvec"] - o["tvec"], axis=1) / np.maximum(np.linalg.norm(o["tvec"], axis=1), 1e-9)
        assert dt[ok].max() <= 1e-6
    assert np.all(h["quat"][~ok] == 0) and np.all(h["tvec"][~ok] == 0) and np.all(h["rvec"][~ok] == 0)
    return ok


def to_numpy(out, B):
    return {k: v.cpu().numpy()[:B] for k, v in out.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Q,C", SOLVER_SHAPES)
def test_solver_front_end_shapes(gpu_device, Q, C, mode):
    """The selection at Q = 64 (a full wave), 40, 30, 4 and 1 queries and at 12 and 17 classes (16 labels,
    order[] full), under every mode of spe_pnp_batch, repro_per_image in the EPnP-Ceres one."""
    import pnp_ref
    from spe.config import Camera
    B = 48
    pts, probs, q, t, sig, th = pr.solver_set(B, Q, C, seed=Q * 100 + C)
    s, repro, thr = mode_args(mode, sig, th)
    rc, out = call_pnp(gpu_device, pts, probs, C, mode, s, repro, thr)
    assert rc == 0
    o = pnp_ref.pnp_batch(pts, probs, Camera.K, pr.world_for(C), mode=mode, repro=repro, sigmas=s, repro_per_image=thr)
    ok = check_solve(to_numpy(out, B), o)
    if Q >= 11:
        assert ok.sum() >= B // 2
    if C == 17:
        assert (o["n_corr"] == 16).any()                     # all 16 labels in one image


def tie_images(C=12):
    """Four images of Q = 12 clean projections (-> points, probs, q, t, expected corr_label rows).
    0: queries 1 and 7 both carry label 3 with bit-identical scores; query 1 sits on the landmark, query 7
       300 px off -- the earlier one is selected, the pose is exact.
    1: the same with the two swapped -- the earlier one is still selected, now the wrong point.
    2: label 2 appears only in a row whose maximum it shares with the background class, label 0 only in a
       row of all-equal probabilities: the lower class index wins both, so both are correspondences.
    3: a row whose maximum is shared by the classes 4 and 9: label 4, at query 0, before label 9's own."""
    rng = np.random.default_rng(31)
    Q = 12
    lab = np.array([[5, 3, 8, 1, 10, 6, 0, 3, 9, 2, 7, 4],
                    [5, 3, 8, 1, 10, 6, 0, 3, 9, 2, 7, 4],
                    [5, 11, 8, 1, 10, 6, 11, 3, 9, 11, 7, 4],
                    [4, 3, 8, 1, 10, 6, 0, 11, 9, 2, 7, 5]])
    B = len(lab)
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.normal(0, .2, B), rng.normal(0, .2, B), rng.uniform(5, 12, B)], 1)
    probs = pr.one_hot(lab, C, hi=0.8)
    true = lab.copy()
    true[2, 1], true[2, 6] = 2, 0                            # what the tie rows of image 2 resolve to
    pts = np.stack([pr.clean_projection(q[b], t[b], true[b], C) for b in range(B)])
    pts[0, 7] += 300
    pts[1, 1] += 300
    probs[2, 1] = 0.02
    probs[2, 1, 2] = probs[2, 1, C - 1] = 0.4
    probs[2, 6] = np.float32(1.0 / C)
    probs[3, 0, 9] = probs[3, 0, 4]
    expect = np.full((B, 16), -1, np.int32)
    for b in range(B):
        seen = list(dict.fromkeys(int(l) for l in true[b] if l != C - 1))
        expect[b, :len(seen)] = seen
    return pts, probs, q, t, expect


def test_selection_ties(gpu_device):
    import pnp_ref
    from spe.config import Camera
    from spe.solver import PoseSolver
    pts, probs, q, t, expect = tie_images()
    rc, out = call_pnp(gpu_device, pts, probs, 12, 0)
    assert rc == 0
    h = to_numpy(out, len(pts))
    np.testing.assert_array_equal(h["corr_label"], expect)
    np.testing.assert_array_equal(h["n_corr"], [11, 11, 11, 11])
    assert list(h["corr_label"][2, :8]) == [5, 2, 8, 1, 10, 6, 0, 3]
    o = pnp_ref.pnp_batch(pts, probs, Camera.K, pr.world_for(12), mode=0)
    check_solve(h, o)
    # the selected query is visible in the pose: exact where the point on the landmark was taken, far
    # off where the one 300 px away was (EPnP on all 11 points, no RANSAC)
    err = [pnp_ref.speed_score(h["quat"][b], h["tvec"][b], q[b], t[b]) for b in range(len(pts))]
    for b in (0, 2, 3):
        assert h["status"][b] == 0 and err[b][0] < 1e-4 and err[b][1] < 1e-3, (b, err[b])
    assert err[1][0] > 1e-2 or err[1][1] > 1e-2, err[1]
    # the self-assessment re-derives the same selection: with sigma = the query's index, the mean over
    # image 0's inliers holds query 1 and not query 7
    import torch
    sig = np.broadcast_to(np.arange(12, dtype=np.float32)[None, :, None], (len(pts), 12, 2)).copy()
    s = PoseSolver()
    d = gpu_device
    a = s.self_assess(_dev(probs, d), _dev(sig, d), out, score_th=0.0, sigma_th=100.0, min_inliers=1)
    torch.cuda.synchronize()
    ms, nc, rel = pnp_ref.self_assess(probs, sig, h["status"], h["corr_label"], h["inlier_mask"].astype(np.uint32),
                                      0.0, 100.0, 1)
    np.testing.assert_array_equal(a["n_confident"].cpu().numpy(), nc)
    np.testing.assert_array_equal(a["reliable"].cpu().numpy(), rel)
    np.testing.assert_allclose(a["mean_sigma"].cpu().numpy(), ms, rtol=1e-6)
    assert h["inlier_mask"][0] == 0x7FF and ms[0] == np.float32(sum(range(12)) - 7) / 11


def test_all_sixteen_labels_by_hand(gpu_device):
    """C = 17, Q = 16, every label once in scrambled order on clean projections: n_corr = 16, corr_label is
    the query order, the EPnP pose is the true one."""
    import pnp_ref
    from spe.config import Camera
    rng = np.random.default_rng(8)
    order = np.array([9, 3, 15, 0, 12, 7, 1, 14, 5, 10, 2, 8, 13, 4, 11, 6])
    B = 3
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.normal(0, .2, B), rng.normal(0, .2, B), rng.uniform(5, 12, B)], 1)
    lab = np.stack([np.roll(order, b) for b in range(B)])
    pts = np.stack([pr.clean_projection(q[b], t[b], lab[b], 17) for b in range(B)])
    probs = pr.one_hot(lab, 17, hi=0.7)
    for mode in (0, 1, 3):
        rc, out = call_pnp(gpu_device, pts, probs, 17, mode)
        assert rc == 0
        h = to_numpy(out, B)
        np.testing.assert_array_equal(h["corr_label"], lab)
        np.testing.assert_array_equal(h["n_corr"], [16] * B)
        np.testing.assert_array_equal(h["inlier_mask"], [0xFFFF] * B)
        check_solve(h, pnp_ref.pnp_batch(pts, probs, Camera.K, pr.world16(), mode=mode))
        for b in range(B):
            s_t, s_q = pnp_ref.speed_score(h["quat"][b], h["tvec"][b], q[b], t[b])
            assert s_t < 1e-4 and s_q < 1e-3, (mode, b, s_t, s_q)


@pytest.mark.parametrize("mode", MODES)
def test_nullable_outputs(gpu_device, mode):
    """rvec, status, n_corr, corr_label and inlier_mask all NULL: the same quat and tvec, bit for bit."""
    pts, probs, q, t, sig, th = pr.solver_set(48, 40, 12, seed=4012)
    s, repro, thr = mode_args(mode, sig, th)
    rc0, full = call_pnp(gpu_device, pts, probs, 12, mode, s, repro, thr)
    rc1, bare = call_pnp(gpu_device, pts, probs, 12, mode, s, repro, thr, nulls=True)
    assert rc0 == 0 and rc1 == 0
    np.testing.assert_array_equal(bare["quat"].cpu().numpy(), full["quat"].cpu().numpy())
    np.testing.assert_array_equal(bare["tvec"].cpu().numpy(), full["tvec"].cpu().numpy())
    assert _untouched(*[bare[k] for k in OUT_KEYS[2:]])


@pytest.mark.parametrize("mode", MODES)
def test_batches_of_zero_and_one(gpu_device, mode):
    import pnp_ref
    from spe.config import Camera
    pts, probs, q, t, sig, th = pr.solver_set(48, 40, 12, seed=4012)
    s, repro, thr = mode_args(mode, sig, th)
    rc, out = call_pnp(gpu_device, pts, probs, 12, mode, s, repro, thr, B=0)
    assert rc == 0 and _untouched(*out.values())
    one = slice(5, 6)
    s1, th1 = (None if s is None else s[one]), (None if thr is None else thr[one])
    rc, out = call_pnp(gpu_device, pts[one], probs[one], 12, mode, s1, repro, th1)
    assert rc == 0
    o = pnp_ref.pnp_batch(pts[one], probs[one], Camera.K, pr.world_for(12), mode=mode, repro=repro, sigmas=s1,
                          repro_per_image=th1)
    assert check_solve(to_numpy(out, 1), o).all()


@pytest.mark.parametrize("case", ["q65", "q0", "c18", "c1", "iters0", "iters256", "conf0", "conf1", "conf_nan", "mode_neg",
                                  "mode_exhaustive", "mode6"])
def test_solver_refusals(gpu_device, case):
    from spe import _lib
    kw = {"q65": dict(Q=65), "q0": dict(Q=0), "c18": dict(C=18), "c1": dict(C=1), "iters0": dict(iters=0),
          "iters256": dict(iters=256), "conf0": dict(conf=0.0), "conf1": dict(conf=1.0), "conf_nan": dict(conf=float("nan")),
          "mode_neg": dict(mode=-1), "mode_exhaustive": dict(mode=5), "mode6": dict(mode=6)}[case]
    Q, C = max(kw.get("Q", 11), 1), max(kw.get("C", 12), 2)
    pts, probs = np.zeros((2, Q, 2), np.float32), np.zeros((2, Q, C), np.float32)
    sig = np.ones((2, Q, 2), np.float32)
    mode = kw.pop("mode", 2)
    rc, out = call_pnp(gpu_device, pts, probs, 12, mode, sig, 25.0, **kw)
    what = b"bad solver mode" if case.startswith("mode") else b"ransac_iters" if case[:4] in ("iter", "conf") else b"bad argument"
    assert rc == SPE_E_ARG and what in _lib.lib().spe_last_error()
    assert _untouched(*out.values())


def call_self_assess(dev, probs, sig, status, corr_label, mask, score_th, sigma_th, min_inl, Q=None, C=None):
    import torch
    from spe import _lib
    B, q, c = probs.shape
    out = [_filled((B,), torch.float32, dev), _filled((B,), torch.int32, dev), _filled((B,), torch.uint8, dev)]
    ins = [_dev(probs, dev), _dev(sig, dev), _dev(status.astype(np.int32), dev), _dev(corr_label.astype(np.int32), dev),
           _dev(mask.astype(np.uint32).view(np.int32), dev)]
    rc = _lib.lib().spe_self_assess(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], B, q if Q is None else Q,
                                    c if C is None else C, score_th, sigma_th, min_inl, *[_lib.ptr(a) for a in out])
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("Q,C", [(64, 17), (40, 12)])
def test_self_assess_shapes(gpu_device, Q, C):
    """spe_self_assess on the sigma solver's own outputs at the widest shapes, with two doctored images:
    0 keeps its status and loses its inliers (mean_sigma = inf, not reliable), 1 fails with a mask of
    ones (the mask of an image without a pose is ignored)."""
    import pnp_ref
    B = 48
    pts, probs, q, t, sig, th = pr.solver_set(B, Q, C, seed=Q * 100 + C)
    sig = (sig * 0.4).astype(np.float32)                     # mean sigmas on both sides of the thresholds
    rc, out = call_pnp(gpu_device, pts, probs, C, 2, sig, 25.0)
    assert rc == 0
    h = to_numpy(out, B)
    status, mask = h["status"].copy(), h["inlier_mask"].astype(np.uint32)
    solved = np.nonzero((status == 0) & (mask != 0))[0]
    a, b = solved[0], solved[1]
    mask[a] = 0
    status[b], mask[b] = 2, 0xFFFFFFFF
    for sigma_th, score_th, min_inl in ((5.0, 0.5, 4), (4.2, 0.6, 5), (12.0, 0.0, 0)):
        rc, (hm, hn, hr) = call_self_assess(gpu_device, probs, sig, status, h["corr_label"], mask, score_th, sigma_th, min_inl)
        assert rc == 0
        ms, nc, rel = pnp_ref.self_assess(probs, sig, status, h["corr_label"], mask, score_th, sigma_th, min_inl)
        hm = hm.cpu().numpy()
        np.testing.assert_array_equal(hn.cpu().numpy(), nc)
        np.testing.assert_array_equal(hr.cpu().numpy().astype(bool), rel)
        fin = np.isfinite(ms)
        np.testing.assert_array_equal(np.isfinite(hm), fin)
        np.testing.assert_allclose(hm[fin], ms[fin], rtol=1e-6)
        for i in (a, b):
            assert np.isposinf(hm[i]) and hn.cpu().numpy()[i] == 0 and not hr.cpu().numpy()[i]
        assert 0 < rel.sum() < B or sigma_th != 5.0
    rc, outs = call_self_assess(gpu_device, probs, sig, status, h["corr_label"], mask, 0.5, 5.0, -1)
    assert rc == SPE_E_ARG and _untouched(*outs)
    rc, outs = call_self_assess(gpu_device, probs, sig, status, h["corr_label"], mask, 0.5, 5.0, 4, Q=65)
    assert rc == SPE_E_ARG and _untouched(*outs)
    rc, outs = call_self_assess(gpu_device, probs, sig, status, h["corr_label"], mask, 0.5, 5.0, 4, C=18)
    assert rc == SPE_E_ARG and _untouched(*outs)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_speed_score_batches(gpu_device, B):
    """score_kernel around its 128-thread block and the 64-lane wave: zero, non-unit and sign-flipped
    predicted quaternions, a last row that only a correct bound check leaves alone."""
    import torch
    import pnp_ref
    from spe import _lib
    rng = np.random.default_rng(B)
    q = rng.normal(size=(B, 4)).astype(np.float32)           # non-unit: |q . q_gt| may exceed 1
    q[::5] /= np.linalg.norm(q[::5], axis=1, keepdims=True)
    q[::7] = 0
    q[-1] *= 3
    t = rng.normal(size=(B, 3)) + [0, 0, 9]
    t[::7] = 0
    qg = rng.normal(size=(B, 4))
    qg /= np.linalg.norm(qg, axis=1, keepdims=True)
    tg = rng.normal(size=(B, 3)) + [0, 0, 10]
    d = gpu_device
    s_t, s_q = _filled((B + 1,), torch.float64, d), _filled((B + 1,), torch.float64, d)
    ins = [_dev(q, d), _dev(t, d), _dev(qg, d), _dev(tg, d)]
    rc = _lib.lib().spe_speed_score(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], B, _lib.ptr(s_t), _lib.ptr(s_q))
    torch.cuda.synchronize()
    assert rc == 0
    s_t, s_q = s_t.cpu().numpy(), s_q.cpu().numpy()
    assert s_t[B] == FILL and s_q[B] == FILL                 # nothing past row B - 1
    for i in range(B):
        a, b = pnp_ref.speed_score(q[i].astype(np.float64), t[i], qg[i], tg[i])
        assert abs(s_t[i] - a) < 1e-12 and abs(s_q[i] - b) < 1e-9, (i, s_t[i], a, s_q[i], b)
    assert abs(s_q[0] - np.pi) < 1e-9 and abs(s_t[0] - 1.0) < 1e-12      # row 0: the zero pose of a failure
