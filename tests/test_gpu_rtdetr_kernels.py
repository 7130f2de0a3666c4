"""The five kernels of csrc/rtdetr.hip (resample2x, query_select, qpos_hidden, head_finish, msdeform) one by one,
through their spe_debug_rt_* hooks, against fp64 restatements (tests/rtdetr_kernels_ref.py, torch's own
interpolate / grid_sample in fp64) of the same dtype-rounded operands.  Every output buffer is NaN-filled first, so
an unwritten element fails, and what a kernel must not write (pad columns, absent heads) must still be NaN after.

Gates.  tests/test_gpu_rtdetr_ghostv2.py's, relative to max(1, max |ref|): 1e-5 fp32, 2e-2 bf16; outputs the kernel
writes as fp32 (all of head_finish, sel_logits, sel_anchors) take 1e-5 in the bf16 variant too.  Exact: nearest
resampling, bicubic of a spatially constant map (the taps -3/32, 19/32 are exact and sum to 1), everything
query_select writes, msdeform of points with no corner on the map (0).

msdeform, fp32: the pixel coordinate is computed in fp32, and its error times the local slope of a random value
map is what the output loses, so the gate is max(1e-5 max(1, max |ref|), 4 x what the same restatement evaluated in
torch fp32 on the CPU loses against fp64), computed in the test.  Measured on an MI355X (CPU fp32 vs fp64 / kernel
vs fp64 / gate; max |ref| 1.0 .. 2.9):
  3 levels x 4 points   6.466e-07 / 6.466e-07 / 1.955e-05        one point, inside   4.046e-07 / 4.046e-07 / 2.861e-05
  4 levels x 4 points   5.217e-07 / 5.014e-07 / 1.695e-05        left / right        2.522e-07, 6.533e-07 (kernel the same)
  2 levels x 3 points   2.642e-07 / 2.642e-07 / 1.840e-05        top / bottom        3.394e-07, 8.519e-07 (kernel the same)
                                                                 outside / far       0 / 0 / 1.000e-05
so the kernel loses what torch's own fp32 grid_sample loses, the 1e-5 term is the gate in every case, and four times
the CPU figure (<= 3.4e-06) would hold as well.  bf16: 3.4e-03 .. 3.6e-03 (one point: up to 6.9e-03) against gates
of 3.4e-02 .. 5.7e-02.
A swapped axis, the other align_corners convention or a missing zero pad gives errors of order 1.

Ties: torch.topk promises no order among equal scores; the kernel documents "lower token index first" (what
torch's CPU topk gives for the all-NaN case of tests/test_rtdetr.py), and that is what is pinned here.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spe import _lib
import rtdetr_kernels_ref as kr

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32, 1e-5), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16, 2e-2)}
NAN = float("nan")
REFUSED = -5


def _p(t):
    return _lib.ptr(t)


def _ints(xs):
    return (ctypes.c_int * len(xs))(*xs)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _close(got, ref, tol, what=""):
    scale = max(1.0, ref.abs().max().item())
    err = (got.double().cpu() - ref.double().cpu()).abs().max().item()
    print(f"{what} max |d| {err:.3e} (gate {tol * scale:.3e})")
    assert err <= tol * scale, (what, err, scale)          # (NaN fails)


# ---------------------------------------------------------------- resample2x
# (B, H, W, C, ldi, ldo, input channel offset, output channel offset): non-square / every bicubic tap clamped on
# both sides / the concat-slice use / a production-like width / one fp32 chunk
RS_CASES = [(3, 6, 4, 16, 16, 16, 0, 0), (1, 2, 2, 8, 8, 8, 0, 0), (2, 4, 10, 8, 24, 40, 8, 16),
            (2, 16, 16, 256, 256, 512, 0, 0)]
RS_FP32_ONLY = [(2, 6, 4, 4, 4, 4, 0, 0)]
RS_PARAMS = [(d, c) for d in ("fp32", "bf16") for c in RS_CASES] + [("fp32", c) for c in RS_FP32_ONLY]
_rs_id = lambda v: v if isinstance(v, str) else "x".join(map(str, v))


def _resample(dev, dtype, case, mode, xin=None):
    """-> (the output buffer, the written slice, the input slice as fp64 NCHW on the CPU)"""
    B, H, W, C, ldi, ldo, ioff, ooff = case
    code, tdt, _ = DT[dtype]
    if xin is None:
        xin = torch.randn(B, H, W, ldi, generator=torch.Generator().manual_seed(H * W + C)) * 2.0
    xin = xin.to(tdt).to(dev)
    Ho, Wo = (2 * H, 2 * W) if mode == 0 else (H // 2, W // 2)
    out = _nan((B, Ho, Wo, ldo), dev, tdt)
    rc = _lib.lib().spe_debug_rt_resample2x(None, code, _p(xin[..., ioff:]), ldi, _p(out[..., ooff:]), ldo, B, H, W, C, mode)
    assert rc == 0, rc
    torch.cuda.synchronize()
    rest = torch.ones(ldo, dtype=torch.bool)
    rest[ooff:ooff + C] = False
    assert torch.isnan(out[..., rest.to(dev)]).all()        # the other columns of the concat buffer: untouched
    return out, out[..., ooff:ooff + C], xin[..., ioff:ioff + C].double().cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype,case", RS_PARAMS, ids=_rs_id)
def test_resample2x_nearest_is_exact(gpu_device, dtype, case):
    _, got, x64 = _resample(gpu_device, dtype, case, 0)
    ref = F.interpolate(x64, scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(got.double().cpu(), ref)


@pytest.mark.parametrize("dtype,case", RS_PARAMS, ids=_rs_id)
def test_resample2x_bicubic_matches_fp64(gpu_device, dtype, case):
    _, got, x64 = _resample(gpu_device, dtype, case, 1)
    ref = F.interpolate(x64, scale_factor=0.5, mode="bicubic", align_corners=False).permute(0, 2, 3, 1)
    assert got.shape == ref.shape
    _close(got, ref, DT[dtype][2])


@pytest.mark.parametrize("dtype,case", RS_PARAMS, ids=_rs_id)
def test_resample2x_bicubic_of_a_constant_map_is_exact(gpu_device, dtype, case):
    """Per channel a constant with few mantissa bits: every product with -3/32 and 19/32 and every partial sum is
    exact, clamped taps included."""
    B, H, W, C, ldi = case[:5]
    const = ((torch.arange(ldi) % 7) - 3).float() * 0.25
    _, got, x64 = _resample(gpu_device, dtype, case, 1, const.expand(B, H, W, ldi).contiguous())
    assert torch.equal(got.double().cpu(), x64.permute(0, 2, 3, 1)[:, :H // 2, :W // 2].contiguous())


def test_resample2x_grid_stride_second_pass(gpu_device):
    """fp32 nearest, B = 66, 32 x 32 x 256: 66 * 64 * 64 * 64 = 17 301 504 output chunks against the launch's cap of
    65535 * 256 = 16 776 960 threads, so the last 524 544 chunks (two images) are written by the grid-stride loop's
    second pass (production: B = 64 at 80 x 80 x 256 runs it too).  About 70 MB in, 277 MB out."""
    dev, B, H, C = gpu_device, 66, 32, 256
    assert B * 4 * H * H * (C // 4) - 65535 * 256 == 524544
    x = torch.randn(B, H, H, C, device=dev)
    out = _nan((B, 2 * H, 2 * H, C), dev)
    assert _lib.lib().spe_debug_rt_resample2x(None, _lib.SPE_DTYPE_F32, _p(x), C, _p(out), C, B, H, H, C, 0) == 0
    torch.cuda.synchronize()
    idx = torch.arange(2 * H, device=dev) // 2
    assert torch.equal(out, x[:, idx][:, :, idx])


def test_resample2x_refuses_shapes_outside_its_contract(gpu_device):
    """C, ldi, ldo multiples of the 16-byte chunk (8 bf16, 4 fp32), even H and W under the bicubic mode: -5 before
    any launch, output untouched; an empty batch is 0."""
    L, f32, b16 = _lib.lib(), _lib.SPE_DTYPE_F32, _lib.SPE_DTYPE_BF16
    z = torch.zeros(4096, device=gpu_device)
    y = torch.full((4096,), 7.0, device=gpu_device)
    assert L.spe_debug_rt_resample2x(None, b16, _p(z), 16, _p(y), 16, 1, 4, 4, 12, 0) == REFUSED     # C = 12 in bf16
    assert L.spe_debug_rt_resample2x(None, b16, _p(z), 16, _p(y), 12, 1, 4, 4, 8, 0) == REFUSED      # ldo = 12
    assert L.spe_debug_rt_resample2x(None, f32, _p(z), 8, _p(y), 8, 1, 5, 4, 8, 1) == REFUSED        # odd H
    assert L.spe_debug_rt_resample2x(None, f32, _p(z), 8, _p(y), 8, 1, 4, 5, 8, 1) == REFUSED        # odd W
    assert L.spe_debug_rt_resample2x(None, f32, _p(z), 8, _p(y), 8, 0, 4, 4, 8, 1) == 0              # B = 0
    torch.cuda.synchronize()
    assert (y == 7.0).all()


# ---------------------------------------------------------------- query_select
def _select(dev, dtype, lvl_start, B, Q, logits, D=256, ldm=None, ldt=None):
    """logits [B][L][C] fp32 per image (token order); the kernel gets them, and the memory, level-major.
    Checks everything the kernel writes, exactly; -> (topk as the reference gives it, level of each token)."""
    code, tdt, _ = DT[dtype]
    ldm, ldt = ldm or D, ldt or D
    L, C = lvl_start[-1], logits.shape[2]
    assert logits.shape == (B, L, C)
    g = torch.Generator().manual_seed(L + Q)
    rows = torch.from_numpy(kr.level_major_rows(lvl_start, B))             # [B][L]
    lm = torch.empty(B * L, C)
    lm[rows.reshape(-1)] = logits.reshape(B * L, C)
    memory = torch.randn(B * L, ldm, generator=g).to(tdt)
    anchors = torch.randn(L, 2, generator=g) * 3.0
    anchors[::5] = float("inf")                                            # (invalid anchors are +inf)
    topk = torch.full((B, Q), -1, dtype=torch.int32, device=dev)
    target = _nan((B * Q, ldt), dev, tdt)
    sel_logits, sel_anchors = _nan((B * Q, C), dev), _nan((B * Q, 2), dev)
    lm_d, memory_d, anchors_d = lm.to(dev), memory.to(dev), anchors.to(dev)
    rc = _lib.lib().spe_debug_rt_query_select(None, code, _p(lm_d), C, _p(memory_d), ldm, _p(anchors_d), B, Q, D,
                                              len(lvl_start) - 1, _ints(lvl_start), _p(topk), _p(target), ldt,
                                              _p(sel_logits), _p(sel_anchors))
    assert rc == 0, rc
    torch.cuda.synchronize()
    want = torch.from_numpy(kr.select_ref(logits.max(-1).values.numpy(), Q))
    np.testing.assert_array_equal(topk.cpu().numpy(), want.numpy())
    src = rows.gather(1, want).reshape(-1)
    target = target.cpu()
    assert torch.equal(target[:, :D], memory[src, :D])                     # bit-equal rows
    assert torch.isnan(target[:, D:]).all()                                # pad columns untouched
    assert torch.equal(sel_logits.cpu(), lm[src])
    assert torch.equal(sel_anchors.cpu(), anchors[want.reshape(-1)])
    level = np.searchsorted(np.asarray(lvl_start[1:]), np.arange(L), side="right")
    return want.numpy(), level


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_unequal_levels(gpu_device, dtype):
    """Levels of 20, 6 and 3 tokens, B = 3: per image two tokens of each level are raised, so each image's top 5
    span all three levels and every level's row block is read at an image offset."""
    lvl_start, B, Q, C = [0, 20, 26, 29], 3, 5, 11
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, 29, C, generator=g)
    for b in range(B):
        for s, e in zip(lvl_start[:-1], lvl_start[1:]):
            t = s + torch.randperm(e - s, generator=g)[:2]
            logits[b, t, int(torch.randint(0, C, (), generator=g))] += 10.0
    want, level = _select(gpu_device, dtype, lvl_start, B, Q, logits)
    for b in range(B):
        assert set(level[want[b]]) == {0, 1, 2}
    assert len({tuple(r) for r in want}) == B                              # the images differ


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_more_tokens_than_threads(gpu_device, dtype):
    """L = 400 > 256 threads, Q = 64 (the most), C = 1."""
    logits = torch.randn(2, 400, 1, generator=torch.Generator().manual_seed(2))
    want, _ = _select(gpu_device, dtype, [0, 300, 380, 400], 2, 64, logits)
    assert (want >= 256).any() and (want < 256).any()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_every_token(gpu_device, dtype):
    """One level, Q = L = 7: a permutation, in score order."""
    logits = torch.randn(2, 7, 3, generator=torch.Generator().manual_seed(3))
    want, _ = _select(gpu_device, dtype, [0, 7], 2, 7, logits)
    assert all(sorted(r) == list(range(7)) for r in want.tolist())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_ties_take_the_lower_token(gpu_device, dtype):
    """L = 600, four distinct scores (about 3 % / 5 % / 32 % / 60 % of the tokens): the 64 selected take every
    token of the two highest and the first of the third, so equal scores meet within a thread's stride (t, t +
    256), across the four waves and across the three levels."""
    lvl_start, B, Q, L = [0, 400, 520, 600], 2, 64, 600
    g = torch.Generator().manual_seed(4)
    u = torch.rand(B, L, generator=g)
    score = (u > 0.60).float() + (u > 0.92).float() + (u > 0.97).float()
    logits = torch.stack([score, score - torch.randint(0, 3, (B, L), generator=g).float()], -1)
    want, level = _select(gpu_device, dtype, lvl_start, B, Q, logits)
    for b in range(B):
        s = score[b].numpy()[want[b]]
        top = want[b][s == 3.0]
        assert set(level[top]) == {0, 1, 2} and len(set((top % 256) // 64)) == 4 and (top >= 256).any()
        assert (s == 1.0).any() and (s == 2.0).any()                       # cut inside the third value's ties
        assert (np.diff(want[b][s == 1.0]) > 0).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_all_minus_inf_image(gpu_device, dtype):
    """Image 1 scores -inf everywhere: tokens 0 .. Q - 1; the other images are not disturbed."""
    logits = torch.randn(3, 29, 4, generator=torch.Generator().manual_seed(5))
    logits[1] = float("-inf")
    want, _ = _select(gpu_device, dtype, [0, 20, 26, 29], 3, 5, logits)
    np.testing.assert_array_equal(want[1], np.arange(5))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_query_select_strides_wider_than_d(gpu_device, dtype):
    logits = torch.randn(2, 29, 4, generator=torch.Generator().manual_seed(6))
    _select(gpu_device, dtype, [0, 20, 26, 29], 2, 5, logits, D=264, ldm=272, ldt=280)


@pytest.mark.parametrize("bad", [dict(Q=65), dict(Q=8, lvl=[0, 7]), dict(lvl=[0, 20, 40, 60, 80, 100]), dict(lvl=[0, 12289]),
                                 dict(C=257)], ids=["Q=65", "Q>L", "levels=5", "L=12289", "C=257"])
def test_query_select_refuses_shapes_outside_its_contract(gpu_device, bad):
    """1 <= Q <= min(64, L), levels <= 4, L <= 12288 (the LDS score table), C <= 256: -5 before any launch."""
    a = dict(Q=5, lvl=[0, 60, 90, 100], C=4)
    a.update(bad)
    z = torch.zeros(1 << 16, device=gpu_device)
    y = torch.full((4096,), 7.0, device=gpu_device)
    rc = _lib.lib().spe_debug_rt_query_select(None, _lib.SPE_DTYPE_F32, _p(z), a["C"], _p(z), 256, _p(z), 1, a["Q"], 256,
                                              len(a["lvl"]) - 1, _ints(a["lvl"]), _p(y), _p(y), 256, _p(y), _p(y))
    torch.cuda.synchronize()
    assert rc == REFUSED and (y == 7.0).all()


# ---------------------------------------------------------------- qpos_hidden
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows", [1, 7])
def test_qpos_hidden_matches_fp64(gpu_device, rows, dtype):
    code, tdt, tol = DT[dtype]
    dev, H, g = gpu_device, 512, torch.Generator().manual_seed(rows)
    ref, w0, b0 = torch.rand(rows, 2, generator=g), torch.randn(H, 2, generator=g), torch.randn(H, generator=g) * 0.5
    out = _nan((rows, H), dev, tdt)
    ref_d, w0_d, b0_d = ref.to(dev), w0.to(dev), b0.to(dev)
    rc = _lib.lib().spe_debug_rt_qpos_hidden(None, code, _p(ref_d), _p(w0_d), _p(b0_d), _p(out), rows, H)
    assert rc == 0, rc
    torch.cuda.synchronize()
    pre = ref.double() @ w0.double().t() + b0.double()
    assert (pre > 0.1).any() and (pre < -0.1).any()
    _close(out, F.relu(pre), tol)
    assert (out.cpu()[pre < 0] == 0).all()


# ---------------------------------------------------------------- head_finish
HEAD_OUT = ["logits", "probs", "points", "points_px", "log_sigmas", "sigmas"]


def _heads(dev, dtype, rows, Q, C, score=True, sigma=True, invsig=1, probs=True, clip=True, ld_h2=512, tweak=None, seed=0):
    """Runs the kernel on random heads (`tweak` edits the CPU inputs first) and compares every output with the
    fp64 restatement at the fp32 gate; what the case leaves out must keep its NaN fill."""
    code, tdt, _ = DT[dtype]
    g = torch.Generator().manual_seed(seed + rows * C)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(hs=rn(rows, 256), cls_w=rn(C, 256) / 16, cls_b=rn(C), h2=F.relu(rn(rows, ld_h2)), box_w2=rn(2, 256) / 16,
             box_b2=rn(2) * 0.5, sig_w2=rn(256) / 16, sig_b2=rn(1) * 0.5,
             pt_add=torch.rand(rows, 2, generator=g) if invsig else rn(rows, 2) * 2.0,
             clip_bbox=torch.rand((rows + Q - 1) // Q, 4, generator=g) * 500.0)
    d["clip_bbox"][:, 2:] += d["clip_bbox"][:, :2] + 100.0
    if tweak:
        tweak(d)
    d["h2"] = d["h2"].to(tdt)
    if not score:
        d["hs"] = d["cls_w"] = d["cls_b"] = None
    if not sigma:
        d["sig_w2"] = d["sig_b2"] = None
    if not clip:
        d["clip_bbox"] = None
    dv = {k: (v.to(dev) if v is not None else None) for k, v in d.items()}
    width = {"logits": C, "probs": C}
    out = {k: _nan((rows, width.get(k, 2)), dev) for k in HEAD_OUT}
    rc = _lib.lib().spe_debug_rt_head_finish(
        None, code, rows, Q, C, _p(dv["hs"]), _p(dv["cls_w"]), _p(dv["cls_b"]), _p(dv["h2"]), ld_h2, _p(dv["box_w2"]),
        _p(dv["box_b2"]), _p(dv["sig_w2"]), _p(dv["sig_b2"]), _p(dv["pt_add"]), invsig, _p(out["logits"]),
        _p(out["probs"]) if probs else None, _p(out["points"]), _p(dv["clip_bbox"]), _p(out["points_px"]),
        _p(out["log_sigmas"]), _p(out["sigmas"]))
    assert rc == 0, rc
    torch.cuda.synchronize()
    f64 = {k: (v.double() if v is not None else None) for k, v in d.items()}
    ref = kr.head_finish_ref(f64["h2"], f64["box_w2"], f64["box_b2"], f64["pt_add"], invsig, Q, hs=f64["hs"], cls_w=f64["cls_w"],
                             cls_b=f64["cls_b"], sig_w2=f64["sig_w2"], sig_b2=f64["sig_b2"], clip_bbox=f64["clip_bbox"])
    if not probs:
        ref.pop("probs", None)
    for k in HEAD_OUT:
        if k in ref:
            _close(out[k], ref[k], 1e-5, k)
        else:
            assert torch.isnan(out[k]).all(), k
    if sigma:
        assert ref["log_sigmas"].abs().max().item() <= 5.0                # so that the relative gate on exp means something
        assert torch.equal(out["log_sigmas"][:, 0], out["log_sigmas"][:, 1])
        assert torch.equal(out["sigmas"][:, 0], out["sigmas"][:, 1])
    return {k: v.cpu() for k, v in out.items()}, ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_finish_every_head(gpu_device, dtype):
    """rows = 10, Q = 5, C = 11: two images with different crop boxes (points_px takes the box of row // Q)."""
    seen = {}
    _heads(gpu_device, dtype, 10, 5, 11, tweak=seen.update)
    assert (seen["clip_bbox"][0] - seen["clip_bbox"][1]).abs().min().item() > 1.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_finish_encoder_call(gpu_device, dtype):
    """The encoder selection's call: anchors added as they are (one of them +inf: the point is 1), no sigma head,
    no probabilities, no crop box; rows = 5 is no multiple of the 4 rows of a block; h2 only 256 wide."""
    def tweak(d):
        d["pt_add"][2, 0] = float("inf")
    out, ref = _heads(gpu_device, dtype, 5, 5, 16, sigma=False, invsig=0, probs=False, clip=False, ld_h2=256, tweak=tweak)
    assert out["points"][2, 0].item() == 1.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_finish_without_score_head(gpu_device, dtype):
    """rows = Q = C = 1 and a null score head: logits and probs keep their NaN fill (checked in _heads)."""
    _heads(gpu_device, dtype, 1, 1, 1, score=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_finish_inverse_sigmoid_clamps(gpu_device, dtype):
    """Reference points 0, 1e-7 / 1, 1 - 1e-7 / 0.5 / -0.01, 1.01: inverse_sigmoid clamps to [0, 1], then both
    ratios' terms to 1e-5, so the addend is -+ln(1e5) = -+11.51 at the ends.  The box hidden rows are solved so
    that the pre-activation cancels it and the points sit near 0.5, where a missing clamp (-inf, ln(1e-7) = -16.1,
    NaN from a negative ratio) moves the result by 0.4 or more."""
    pts = torch.tensor([[0.0, 1e-7], [1.0, 1.0 - 1e-7], [0.5, 0.5], [-0.01, 1.01]])
    assert pts[1, 1].item() < 1.0
    cancel = torch.tensor([[11.5, 11.5], [-11.5, -11.5], [0.3, -0.3], [11.5, -11.5]])

    def tweak(d):
        W = d["box_w2"].double()
        d["h2"][:, :256] = ((cancel.double() - d["box_b2"].double()) @ torch.linalg.inv(W @ W.t()) @ W).float()
        d["pt_add"] = pts.clone()
    out, ref = _heads(gpu_device, dtype, 4, 2, 3, tweak=tweak)
    assert ((ref["points"] > 0.2) & (ref["points"] < 0.8)).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_head_finish_saturated_sigmoid_and_softmax(gpu_device, dtype):
    """Box pre-activations near +-90 on either coordinate (exp(90) overflows fp32) and logits spread over +-80:
    every output finite, points 0 or 1 within the gate, probabilities a one-hot within the gate."""
    def tweak(d):
        d["cls_w"] *= 0.05
        d["cls_b"] = torch.linspace(-80.0, 80.0, 16)[torch.randperm(16, generator=torch.Generator().manual_seed(7))]
        d["box_w2"] *= 0.05
        d["box_b2"] = torch.tensor([90.0, -90.0])
        d["pt_add"] = torch.tensor([[0.0, 0.0], [-180.0, 180.0], [0.0, 180.0], [-180.0, 0.0]])
    out, ref = _heads(gpu_device, dtype, 4, 2, 16, invsig=0, tweak=tweak)
    assert all(torch.isfinite(v).all() for v in out.values())
    assert (ref["logits"].max() - ref["logits"].min()).item() > 150.0
    assert ((ref["points"] < 1e-30) | (ref["points"] > 1 - 1e-12)).all()
    assert ((ref["points"] < 0.5).any(0) & (ref["points"] > 0.5).any(0)).all()


@pytest.mark.parametrize("bad", ["C=17", "points", "pt_add", "h2", "hs"])
def test_head_finish_refuses_arguments_outside_its_contract(gpu_device, bad):
    """C <= 16 (the per-lane logit registers); points, pt_add and h2 required; a score head needs hs: -5 before any
    launch, output untouched."""
    z = torch.zeros(4096, device=gpu_device)
    y = torch.full((4096,), 7.0, device=gpu_device)
    a = dict(hs=z, h2=z, pt_add=z, points=y)
    if bad != "C=17":
        a[bad] = None
    rc = _lib.lib().spe_debug_rt_head_finish(None, _lib.SPE_DTYPE_F32, 2, 2, 17 if bad == "C=17" else 4, _p(a["hs"]), _p(z), _p(z),
                                             _p(a["h2"]), 512, _p(z), _p(z), _p(z), _p(z), _p(a["pt_add"]), 1, _p(y), _p(y),
                                             _p(a["points"]), _p(z), _p(y), _p(y), _p(y))
    torch.cuda.synchronize()
    assert rc == REFUSED and (y == 7.0).all()


# ---------------------------------------------------------------- msdeform
@functools.lru_cache(maxsize=None)
def _ms_inputs(case_index, cls=None):
    if cls is None:
        inp = kr.msdeform_inputs(kr.MSDEFORM_CASES[case_index])
        kr.check_msdeform_coverage(inp)                       # the inputs, not the kernel, guarantee the coverage
        return inp
    inp = kr.msdeform_inputs(kr.MSDEFORM_SINGLE, classes=[cls])
    assert kr.msdeform_coverage(inp)[0][cls] == 1.0
    return inp


def _msdeform(dev, dtype, inp):
    """value: level-major rows of 512 columns, the kernel reads 256..511 (columns 0..255 hold other numbers);
    so_aw rows 8 wider than the offsets and logits, out rows 8 wider than 256: both pads NaN."""
    code, tdt, tol = DT[dtype]
    shapes, B, Q, npt = inp["shapes"], inp["B"], inp["Q"], inp["points"]
    nl, rows, n = len(shapes), B * Q, kr.HEADS * len(shapes) * npt
    val = inp["value"].to(tdt)
    start = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).tolist()
    buf = torch.randn(B * start[-1], 512, generator=torch.Generator().manual_seed(11)).to(tdt)
    for s, e in zip(start[:-1], start[1:]):
        buf[B * s:B * e, 256:] = val[:, s:e].reshape(B * (e - s), 256)
    so = torch.full((rows, 3 * n + 8), NAN)
    so[:, :2 * n] = inp["off"].reshape(rows, 2 * n)
    so[:, 2 * n:3 * n] = inp["logits"].reshape(rows, n)
    buf, so, ref_d, out = buf.to(dev), so.to(dev), inp["ref"].reshape(rows, 2).to(dev), _nan((rows, 264), dev, tdt)
    rc = _lib.lib().spe_debug_rt_msdeform(None, code, _p(buf[:, 256:]), 512, _p(so), 3 * n + 8, _p(ref_d),
                                          _p(out), 264, rows, Q, kr.HEADS, nl, npt, _ints([h for h, _ in shapes]),
                                          _ints([w for _, w in shapes]), _ints([B * s for s in start[:-1]]))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[:, 256:]).all()
    got = out[:, :256].double()
    ref = kr.msdeform_ref(val.double(), shapes, inp["ref"], inp["off"], inp["logits"]).reshape(rows, 256)
    assert torch.isfinite(ref).all()
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    if dtype == "fp32":
        own = (kr.msdeform_ref(val.float(), shapes, inp["ref"], inp["off"], inp["logits"], torch.float32).reshape(rows, 256).double()
               - ref).abs().max().item()
        gate = max(1e-5 * scale, 4.0 * own)
        print(f"msdeform fp32: CPU fp32 vs fp64 {own:.3e}, kernel vs fp64 {err:.3e}, gate {gate:.3e}, max |ref| {scale:.2f}")
    else:
        gate = tol * scale
        print(f"msdeform bf16: kernel vs fp64 {err:.3e}, gate {gate:.3e}")
    assert err <= gate, (err, gate)                            # (NaN fails)
    return got, ref


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case_index", range(len(kr.MSDEFORM_CASES)), ids=["3lv-4pt", "4lv-4pt", "2lv-3pt"])
def test_msdeform_matches_fp64(gpu_device, case_index, dtype):
    """Non-square levels of unequal sizes (W and H, the row stride and the level's row block all differ), 128 samples
    a row at the LDS boundary, 3 points; B > 1 with different values per image; reference points exactly 0 and 1; a
    logit row spread over 60; points of every corner class in the shares rtdetr_kernels_ref asserts."""
    _msdeform(gpu_device, dtype, _ms_inputs(case_index))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cls", kr.CLASSES)
def test_msdeform_single_point(gpu_device, cls, dtype):
    """One 3 x 5 level, one point, one row: the 8 heads' points placed in one class each run.  With no corner on the
    map (outside, and far outside at |pixel| > 1e6) the output is exactly 0."""
    got, ref = _msdeform(gpu_device, dtype, _ms_inputs(0, cls))
    if cls in ("outside", "far"):
        assert (ref == 0).all() and (got == 0).all()
    else:
        assert (ref.reshape(8, 32).abs().max(1).values > 0).all()


def test_msdeform_refuses_shapes_outside_its_contract(gpu_device):
    """8 heads of 32 channels, levels <= 4, points <= 4 (the LDS tables hold 8 x 4 x 4 samples): -5 before any
    launch, output untouched; no rows is 0."""
    L, f32 = _lib.lib(), _lib.SPE_DTYPE_F32
    z = torch.zeros(1 << 16, device=gpu_device)
    y = torch.full((4096,), 7.0, device=gpu_device)
    five = _ints([2, 2, 2, 2, 2])
    rows0 = _ints([0, 4, 8, 12, 16])
    call = lambda rows, heads, levels, points: L.spe_debug_rt_msdeform(None, f32, _p(z), 256, _p(z), 512, _p(z), _p(y), 256, rows, 1,
                                                                      heads, levels, points, five, five, rows0)
    assert call(2, 4, 3, 4) == REFUSED
    assert call(2, 8, 5, 1) == REFUSED and call(2, 8, 5, 4) == REFUSED
    assert call(2, 8, 3, 5) == REFUSED
    assert call(0, 8, 3, 4) == 0
    torch.cuda.synchronize()
    assert (y == 7.0).all()
