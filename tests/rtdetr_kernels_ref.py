"""fp64 restatements of the five kernels of csrc/rtdetr.hip, and the input generator of the msdeform tests
(tests/test_gpu_rtdetr_kernels.py runs the kernels against them; tests/test_rtdetr_kernels_ref.py ties them to
the model's own operations on the CPU).  Test infrastructure only.

Memory is level-major (rtdetr.hip): token t of level l of image b is row B * lvl_start[l] + b * hw_l +
(t - lvl_start[l]).
"""
import numpy as np
import torch

import rtdetr_ref

HEADS = 8


# ---------------------------------------------------------------- query_select
def level_major_rows(lvl_start, B):
    """[B][L] int64: the level-major row of token t of image b."""
    L = lvl_start[-1]
    rows = np.empty((B, L), np.int64)
    for s, e in zip(lvl_start[:-1], lvl_start[1:]):
        rows[:, s:e] = B * s + np.arange(B)[:, None] * (e - s) + np.arange(e - s)[None]
    return rows


def select_ref(score, Q):
    """score [B][L] (max over classes): the Q best tokens per image, descending, the lower token index first
    among equal scores (a stable sort; torch.topk promises no order among ties, the kernel documents this one)."""
    return np.argsort(-np.asarray(score, np.float64), axis=1, kind="stable")[:, :Q]


# ---------------------------------------------------------------- head_finish
def head_finish_ref(h2, box_w2, box_b2, pt_add, invsig, Q, hs=None, cls_w=None, cls_b=None, sig_w2=None, sig_b2=None,
                    clip_bbox=None):
    """The kernel's header comment on fp64 tensors: h2 [rows][>= 256 (512 with a sigma head)], pt_add [rows][2]."""
    o = {}
    if cls_w is not None:
        o["logits"] = hs @ cls_w.t() + cls_b
        o["probs"] = torch.softmax(o["logits"], -1)
    add = rtdetr_ref.inverse_sigmoid(pt_add) if invsig else pt_add
    o["points"] = torch.sigmoid(h2[:, :256] @ box_w2.t() + box_b2 + add)
    if clip_bbox is not None:
        bb = clip_bbox[torch.arange(h2.shape[0]) // Q]
        o["points_px"] = o["points"] * (bb[:, 2:4] - bb[:, 0:2]) + bb[:, 0:2]
    if sig_w2 is not None:
        o["log_sigmas"] = (h2[:, 256:512] @ sig_w2.reshape(256, 1) + sig_b2).repeat(1, 2)
        o["sigmas"] = torch.exp(o["log_sigmas"])
    return o


# ---------------------------------------------------------------- msdeform
def msdeform_ref(value, shapes, ref, off, logits, dtype=torch.float64):
    """value [B][L][256] image-major (levels concatenated), shapes [(H_l, W_l)], ref [B][Q][2], off
    [B][Q][8][nl][np][2], logits [B][Q][8][nl * np] -> [B][Q][256], every step in `dtype`."""
    B, L, _ = value.shape
    Q, nl, npt = ref.shape[1], len(shapes), off.shape[4]
    aw = torch.softmax(logits.to(dtype), -1).reshape(B, Q, HEADS, nl, npt)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=dtype).reshape(1, 1, 1, nl, 1, 2)
    loc = ref.to(dtype)[:, :, None, None, None, :] + off.to(dtype) / norm
    return rtdetr_ref.deformable_core(value.to(dtype).reshape(B, L, HEADS, 32), shapes, loc, aw)


# (levels as (H_l, W_l), points, B, Q): non-square maps of unequal sizes / 4 x 4 = the 128-sample LDS boundary,
# a 1-high map / 3 points
MSDEFORM_CASES = [
    ([(5, 8), (3, 4), (2, 2)], 4, 3, 5),
    ([(6, 4), (4, 6), (2, 3), (1, 2)], 4, 2, 3),
    ([(4, 2), (2, 4)], 3, 2, 2),
]
MSDEFORM_SINGLE = ([(3, 5)], 1, 1, 1)
CLASSES = ["inside", "left", "right", "top", "bottom", "outside", "far"]
# share of the sampling points drawn into each class; the rest is uniform over the map and a margin
DRAW = {"inside": 0.30, "left": 0.07, "right": 0.07, "top": 0.07, "bottom": 0.07, "outside": 0.15, "far": 0.03}


def _draw_pixel(cls, H, W, g):
    """a pixel coordinate (ix, iy) of a sampling point of class `cls` on an H x W map, 0.02 off every edge"""
    u = lambda a, b: a + 0.02 + (b - a - 0.04) * torch.rand((), generator=g, dtype=torch.float64).item()
    if cls == "inside" and (H < 2 or W < 2):
        cls = "top" if H < 2 else "left"              # a 1-wide map has no point with four corners inside
    if cls == "inside":
        return u(0, W - 1), u(0, H - 1)
    if cls in ("left", "right"):
        return (u(-1, 0) if cls == "left" else u(W - 1, W)), u(-1, H)
    if cls in ("top", "bottom"):
        return u(-1, W), (u(-1, 0) if cls == "top" else u(H - 1, H))
    side = int(torch.randint(0, 4, (), generator=g))
    lo, hi = (1.0, 4.0) if cls == "outside" else (1e6, 4e6)
    d = u(lo, hi)
    if side < 2:
        return (-d if side == 0 else W - 1 + d), u(-4, H + 3)
    return u(-4, W + 3), (-d if side == 2 else H - 1 + d)


def msdeform_inputs(case, seed=0, classes=None):
    """Inputs of one case, fp32 (the kernel's formats) except `value` (fp32, rounded to the kernel's dtype by the
    caller).  Every sampling point is drawn into a class of DRAW (or `classes`: a list cycled over the points), as
    a pixel coordinate; its offset is what puts it there: off = (ix + 0.5, iy + 0.5) - ref * (W_l, H_l).
    Reference points of rows 0 / 1 are exactly (0, 1) / (1, 0) (one row: (1, 0)); one (row, head) has attention
    logits spread over 60."""
    shapes, npt, B, Q = case
    nl = len(shapes)
    g = torch.Generator().manual_seed(seed)
    L = sum(h * w for h, w in shapes)
    value = torch.randn(B, L, 256, generator=g)
    ref = (0.05 + 0.9 * torch.rand(B, Q, 2, generator=g))
    flat = ref.reshape(-1, 2)
    flat[0] = torch.tensor([1.0, 0.0])
    if flat.shape[0] > 1:
        flat[0], flat[1] = torch.tensor([0.0, 1.0]), torch.tensor([1.0, 0.0])
    n = B * Q * HEADS * nl * npt
    if classes is None:
        plan = []
        for c, share in DRAW.items():
            plan += [c] * max(1, int(round(share * n)))
        plan += ["any"] * (n - len(plan))
        plan = [plan[i] for i in torch.randperm(n, generator=g).tolist()]
    else:
        plan = [classes[i % len(classes)] for i in range(n)]
    off = torch.empty(B, Q, HEADS, nl, npt, 2, dtype=torch.float64)
    i = 0
    for b in range(B):
        for q in range(Q):
            for h in range(HEADS):
                for l, (Hl, Wl) in enumerate(shapes):
                    for p in range(npt):
                        if plan[i] == "any":
                            r = torch.rand(2, generator=g, dtype=torch.float64)
                            ix, iy = -1.5 + (Wl + 2) * r[0].item(), -1.5 + (Hl + 2) * r[1].item()
                        else:
                            ix, iy = _draw_pixel(plan[i], Hl, Wl, g)
                        off[b, q, h, l, p, 0] = ix + 0.5 - ref[b, q, 0].double().item() * Wl
                        off[b, q, h, l, p, 1] = iy + 0.5 - ref[b, q, 1].double().item() * Hl
                        i += 1
    logits = torch.randn(B, Q, HEADS, nl * npt, generator=g) * 2.0
    logits[0, 0, HEADS - 1] = torch.linspace(-30.0, 30.0, nl * npt)[torch.randperm(nl * npt, generator=g)]
    return dict(value=value, shapes=shapes, ref=ref, off=off.float(), logits=logits, B=B, Q=Q, points=npt)


def msdeform_coverage(inp):
    """Share of the sampling points in each class of CLASSES, from the fp32 inputs in fp64: pixel coordinate
    ix = (ref_x + off_x / W_l) * W_l - 0.5 (align_corners=False), corners floor(ix), floor(ix) + 1 (same in y).
    inside: four corners on the map; left / right / top / bottom: the corner pair beyond that border off the map
    and at least one corner on it; outside: no corner on the map; far: |ix| or |iy| > 1e6."""
    shapes = inp["shapes"]
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).reshape(1, 1, 1, len(shapes), 1, 2)
    pix = (inp["ref"].double()[:, :, None, None, None, :] + inp["off"].double() / wh) * wh - 0.5
    c0 = torch.floor(pix)
    on0, on1 = (c0 >= 0) & (c0 < wh), (c0 + 1 >= 0) & (c0 + 1 < wh)
    x0, y0, x1, y1 = on0[..., 0], on0[..., 1], on1[..., 0], on1[..., 1]
    anyx, anyy = x0 | x1, y0 | y1
    cls = {"inside": x0 & x1 & y0 & y1,
           "left": ~x0 & x1 & anyy, "right": x0 & ~x1 & anyy,
           "top": ~y0 & y1 & anyx, "bottom": y0 & ~y1 & anyx,
           "outside": ~(anyx & anyy),
           "far": (pix.abs() > 1e6).any(-1)}
    return {k: v.double().mean().item() for k, v in cls.items()}, {k: int(v.sum()) for k, v in cls.items()}


# what the issue asks of the inputs of every multi-point case
REQUIRED_SHARE = {"inside": 0.10, "left": 0.02, "right": 0.02, "top": 0.02, "bottom": 0.02, "outside": 0.05}


def check_msdeform_coverage(inp):
    share, count = msdeform_coverage(inp)
    for k, s in REQUIRED_SHARE.items():
        assert share[k] >= s, (k, share)
    assert count["far"] >= 1, count
    assert (inp["ref"] == 0).any() and (inp["ref"] == 1).any()
    lg = inp["logits"]
    assert (lg.max(-1).values - lg.min(-1).values).max().item() >= 60.0
    return share
