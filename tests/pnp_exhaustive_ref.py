"""numpy restatement of the UNC exhaustive solver: PoseSolver.exhausive_pnp
(UNC/utils/speed_eval_ceres.py:326-399) behind SimplePoseSolver.__call__ (:473-522), on the oracle's
primitives (oracle/pnp_ref.py: epnp, project, sigma_lm_core, rodrigues, blender_quat,
select_correspondences, sigma_weights_f32).  The checker of the HIP solver's SPE_PNP_EXHAUSTIVE mode;
the rules the reference leaves open are the ones include/spe.h states for that mode:

  * the four-point error is the float32 sum of the 4 squared reprojection errors (cv2 returns its RMSE,
    only the order is used); a hypothesis whose pose or error is not finite gets +inf;
  * the top-K sort is stable (ties to the lower subset index) and never keeps an +inf record;
  * the threshold after s failing candidates is th0 + 5 s in float64;
  * ceres_pnp gets the selected sigmas (unit sigmas without a sigma input), weights normalised over the
    inliers, as in EPnPCeresSolver;
  * where the reference would never return (no finite hypothesis, no kept candidate that can reach 4
    inliers, every qualifying candidate's error sum >= 100000 or NaN) the status is UNPINNED, zero pose.
"""
import ctypes
import itertools

import numpy as np

import pnp_ref

MAXN = 16
_hyp_cache = {}      # hypotheses of a correspondence set: shared by every topk / threshold / sigma variant


def subsets(n):
    """The subset table in the reference's order (:347)."""
    return list(itertools.combinations(range(n), 4))


def repro_errors(wld, img, rvec, tvec, K):
    """np.linalg.norm(projectPoints(...) - obj, axis=-1) per point, float32 throughout (:367-369)."""
    uv = pnp_ref.project(wld, rvec, tvec, K)
    d = (uv - img).astype(np.float32)
    d2 = (d * d).astype(np.float32)
    return np.sqrt((d2[:, 0] + d2[:, 1]).astype(np.float32)).astype(np.float32)


def np_sum_f32(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.float32(pnp_ref.lib().oracle_np_sum_f32(a.ctypes.data_as(ctypes.c_void_p), len(a)))


def four_point_error(wld4, img4, rvec, tvec, K):
    """float32 sum, in point order, of the squared reprojection errors of the subset's own points."""
    uv = pnp_ref.project(wld4, rvec, tvec, K)
    d = (img4 - uv).astype(np.float32)
    d2 = (d * d).astype(np.float32)
    e = np.float32(0)
    for i in range(len(wld4)):
        e = np.float32(e + np.float32(d2[i, 0] + d2[i, 1]))
    if not (np.isfinite(e) and np.isfinite(rvec).all() and np.isfinite(tvec).all()):
        return np.float32(np.inf)
    return e


def hypotheses(wld, img, K, force_nonfinite=()):
    """EPnP on every four-point subset: (poses [H,6], errors [H] f32).  force_nonfinite: subset
    indices whose pose is replaced by NaN (what a failed solve would hand back)."""
    key = (wld.tobytes(), img.tobytes(), np.asarray(K, np.float64).tobytes(), tuple(sorted(force_nonfinite)))
    if key in _hyp_cache:
        return _hyp_cache[key]
    S = subsets(len(wld))
    poses = np.zeros((len(S), 6))
    errs = np.zeros(len(S), np.float32)
    for h, idx in enumerate(S):
        idx = list(idx)
        r, t = pnp_ref.epnp(wld[idx], img[idx], K)
        if h in force_nonfinite:
            r = np.full(3, np.nan)
        poses[h, :3], poses[h, 3:] = r, t
        errs[h] = four_point_error(wld[idx], img[idx], r, t, K)
    _hyp_cache[key] = (poses, errs)
    return poses, errs


def stable_topk(errs, topk):
    """The topk smallest finite errors, ties to the lower index."""
    order = np.argsort(errs, kind="stable")
    return [int(h) for h in order[:topk] if np.isfinite(errs[h])]


def refine(wld, img, sig, inl, rvec, tvec, K):
    """ceres_pnp (:172-243) on the inliers: normalised float32 observations, float32 weights
    normalised over the inliers, Huber 0.001."""
    xn = np.stack([((img[inl, 0].astype(np.float64) - K[0, 2]) * (1.0 / K[0, 0])).astype(np.float32),
                   ((img[inl, 1].astype(np.float64) - K[1, 2]) * (1.0 / K[1, 1])).astype(np.float32)], 1)
    w = pnp_ref.sigma_weights_f32(sig[inl])
    return pnp_ref.sigma_lm_core(wld[inl].astype(np.float64), xn.astype(np.float64), w.astype(np.float64), 0.001,
                                 rvec, tvec)


def exhaustive_pnp(wld, img, sig, K, th0, topk, force_nonfinite=(), max_steps=1_000_000):
    """exhausive_pnp on selected correspondences wld [n,3] f32, img [n,2] f32, sig [n,2] f32 (n >= 4).
    Returns dict(status, rvec, tvec, cand_index, inlier_mask, repro_final, errors, candidates, trace);
    trace lists (subset index, threshold, n_inliers, reverted or None) per visited candidate."""
    th0 = float(np.float32(th0))
    poses, errs = hypotheses(wld, img, K, force_nonfinite)
    cand = stable_topk(errs, topk)
    out = dict(status=pnp_ref.ST_UNPINNED, rvec=np.zeros(3), tvec=np.zeros(3), cand_index=-1, inlier_mask=0,
               repro_final=np.float32(th0), errors=errs, candidates=cand, trace=[])
    if not cand:
        return out
    tabs = [repro_errors(wld, img, poses[h, :3], poses[h, 3:], K) for h in cand]
    # a candidate whose 4th smallest error is not finite never has 4 inliers: the walk would not end
    if not any(np.isfinite(np.sort(np.where(np.isnan(t), np.inf, t))[3]) for t in tabs):
        return out
    fails, err_opt, qualified, best = 0, 100000, False, None
    while not qualified:
        for h, tab in zip(cand, tabs):
            th = th0 + 5.0 * fails
            inl = np.where(tab.astype(np.float64) < th)[0]
            if len(inl) < 4:
                fails += 1
                assert fails < max_steps
                out["trace"].append((h, th, len(inl), None))
                continue
            qualified = True
            before = np_sum_f32(tab)
            r2, t2 = refine(wld, img, sig, inl, poses[h, :3], poses[h, 3:], K)
            after = np_sum_f32(repro_errors(wld, img, r2, t2, K))
            worse = bool(after > before)
            rep = before if worse else after
            out["trace"].append((h, th, len(inl), worse))
            if err_opt > rep:
                err_opt = rep
                best = (h, (poses[h, :3], poses[h, 3:]) if worse else (r2, t2), inl)
    out["repro_final"] = np.float32(th0 + 5.0 * fails)
    if best is None:
        return out
    h, (r, t), inl = best
    out.update(status=pnp_ref.ST_OK, rvec=np.asarray(r, np.float64), tvec=np.asarray(t, np.float64), cand_index=h,
               inlier_mask=int(sum(1 << int(i) for i in inl)))
    return out


def first_pass_bound(e4, th0, K):
    """The device kernel's bound on the walk: no candidate of a pass below the returned one can have 4
    inliers (e4: every candidate's 4th smallest error, th0 the starting threshold)."""
    E = float(np.min(e4))
    x = np.floor(((E - th0) / 5.0 - (K - 1)) / K) - 1.0
    return max(int(x), 0)


def solve_one(points, probs, sigmas, K, world, th0, topk):
    """The front (:473-522) + exhausive_pnp for one image: points [Q,2], probs [Q,C], sigmas [Q,2] or None."""
    C = probs.shape[1]
    labs, img = pnp_ref.select_correspondences(points, probs)
    n = len(labs)
    res = dict(status=pnp_ref.ST_OK, quat=np.zeros(4, np.float32), tvec=np.zeros(3), rvec=np.zeros(3), n_corr=n,
               corr_label=np.array(labs + [-1] * (MAXN - n), np.int32), inlier_mask=0, cand_index=-1,
               repro_final=np.float32(th0), errors=np.zeros(0, np.float32), candidates=[])
    if n == 0:
        res["status"] = pnp_ref.ST_NO_FG
        return res
    if n < 4:
        res["status"] = pnp_ref.ST_CV_ERROR
        return res
    wld = np.asarray(world, np.float64)[labs].astype(np.float32)
    if sigmas is None:
        sig = np.ones((n, 2), np.float32)
    else:
        # the sigma of the best-score query per label (the first on ties), as the selection takes the point
        best = [max((q for q in range(len(probs)) if probs[q].argmax() == l), key=lambda q: (probs[q, l], -q))
                for l in labs]
        sig = np.asarray(sigmas, np.float32)[best]
    o = exhaustive_pnp(wld, img, sig, np.asarray(K, np.float64), th0, topk)
    for k in ("status", "cand_index", "inlier_mask", "repro_final", "errors", "candidates"):
        res[k] = o[k]
    if o["status"] == pnp_ref.ST_OK:
        res["rvec"], res["tvec"] = o["rvec"], o["tvec"]
        res["quat"] = pnp_ref.blender_quat(pnp_ref.rodrigues(o["rvec"]))
    _ = C
    return res


def solve_batch(points, probs, sigmas, K, world, th, topk):
    """th: one threshold or one per image.  Returns dict of stacked fields + `errors` / `candidates` lists."""
    B = len(points)
    th = np.broadcast_to(np.asarray(th, np.float32), (B,))
    rs = [solve_one(points[b], probs[b], None if sigmas is None else sigmas[b], K, world, th[b], topk)
          for b in range(B)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in
           ("status", "quat", "tvec", "rvec", "n_corr", "corr_label", "inlier_mask", "cand_index", "repro_final")}
    out["errors"] = [r["errors"] for r in rs]
    out["candidates"] = [r["candidates"] for r in rs]
    return out


def near_tie(errors, topk, rel=1e-6):
    """True when the K-th and (K+1)-th smallest finite errors differ by less than `rel` relative: the
    only images a parity test may leave out (which of the two is kept hangs on the last bits)."""
    e = np.sort(errors[np.isfinite(errors)].astype(np.float64))
    return len(e) > topk and abs(e[topk] - e[topk - 1]) < rel * abs(e[topk])


def synthetic_case(seed, noise=0.0, nout=0, n=11, K=None, world=None):
    """n landmarks under a seeded pose: projections + N(0, noise) px, the first `nout` moved 100-300 px
    away.  Returns wld [n,3] f32, img [n,2] f32, rvec, tvec."""
    rng = np.random.default_rng(seed)
    r = rng.normal(size=3)
    r *= rng.uniform(0.3, 2.5) / np.linalg.norm(r)
    t = np.array([rng.normal(0, .3), rng.normal(0, .3), rng.uniform(5, 15)])
    wld = np.asarray(world, np.float64)[:n].astype(np.float32)
    img = pnp_ref.project(wld, r, t, K).astype(np.float32)
    if noise:
        img = (img + rng.normal(0, noise, img.shape)).astype(np.float32)
    if nout:
        img[:nout] += rng.uniform(100, 300, (nout, 2)).astype(np.float32)
    return wld, img, r, t
