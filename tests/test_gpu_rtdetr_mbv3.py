"""UNC RT-DETR behind the MobileNetV3_Large backbone, GPU side: the new gfx950 kernels (mbv3.hip) one by
one against fp64 torch on the same dtype-rounded operands, the backbone stage against the torch-fp32
restatement (tests/rtdetr_mbv3_ref.py), and the whole model against the reference's golden
(tests/golden/rtdetr_mbv3l_s256.npz).

Gates.  Kernels: tests/test_gpu_kernels.py's for the same operand types, relative to max(1, max |ref|):
1e-5 fp32, 2e-2 bf16.  Whole model, fp32: the RT-DETR contract of tests/test_rtdetr.py (pred_pts 1e-4,
logits / sigmas 2e-3, top-k exact; the golden's topk_min_gap is 1.908e-3 against a restatement-vs-reference
encoder score difference of 3.576e-6).  bf16: test_hip_bf16_close_to_reference's gates (points 3e-2, logits
0.3 on queries selected in the same rank, selected sets overlapping >= 80 %) were the starting point and do not
hold through 15 SE / Hardswish blocks (measured on the MI355X: points 3.26e-2, logits 0.332 on image 1), so the
gate is twice what the torch-CPU restatement loses against the fp32 golden with its weights and stage outputs
rounded to bf16 where the kernels round (tools/measure_bf16_rtdetr_mbv3.py: points 1.851e-2, logits 0.2910,
overlap 29 / 30): points <= 3.70e-2, logits <= 0.582; the 80 % overlap stays.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from spe import _lib
from spe.config import SpeConfig
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
from spe.synthetic import synthetic_batch
import rtdetr_ref
import rtdetr_mbv3_ref
from test_rtdetr_mbv3 import golden, reference_run

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32, 1e-5), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16, 2e-2)}
ACTS = {"none": 0, "relu": 1, "hswish": 4}


def _p(t):
    return _lib.ptr(t)


def _act64(x, act):
    if act == "relu":
        return F.relu(x)
    if act == "hswish":
        return x * F.relu6(x + 3.0) / 6.0
    return x


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.double() - ref.double()).abs().max().item()
    print(f"max |d| {err:.3e} (gate {tol * scale:.3e})")
    assert err <= tol * scale, (err, scale)


def _dwconv(dev, dtype, B, C, H, k, stride, act, pool=False, seed=0):
    code, tdt, _ = DT[dtype]
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, H, H, C, generator=g) * 2.0).to(tdt).to(dev)          # NHWC, values past +-3
    w = (torch.randn(k * k, C, generator=g) * (1.5 / k)).to(dev)
    bias = (torch.randn(C, generator=g) * 0.5).to(dev)
    Ho = H // stride
    y = torch.empty(B, Ho, Ho, C, dtype=tdt, device=dev)
    tiles = _lib.lib().spe_debug_dwconv_tiles(Ho, Ho)
    part = torch.full((B, tiles, C), float("nan"), device=dev) if pool else None
    rc = _lib.lib().spe_debug_dwconv(None, code, _p(x), _p(w), _p(bias), _p(y), _p(part), B, H, H, C, k, stride, ACTS[act])
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    w64 = w.double().t().reshape(C, 1, k, k)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w64, bias.double(), stride, k // 2, 1, C)
    return y, _act64(ref, act).permute(0, 2, 3, 1), part


DW_CASES = [(2, 24, 8, 5, 2), (1, 184, 16, 3, 1), (3, 72, 64, 5, 2), (2, 16, 128, 3, 1), (1, 960, 8, 5, 1)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["relu", "hswish"])
@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv_matches_fp64(gpu_device, case, act, dtype):
    y, ref, _ = _dwconv(gpu_device, dtype, *case, act)
    _close(y, ref, DT[dtype][2])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 72, 64, 5, 2), (2, 120, 32, 5, 1), (1, 960, 8, 5, 1), (2, 24, 8, 5, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_dwconv_pooled_sums(gpu_device, case, dtype):
    """The pool partials add up to the fp64 sum of the kernel's own stored outputs (1e-5 relative), every
    partial is written, and two runs give identical bits (fixed-order reduction, no float atomics)."""
    y, _, part = _dwconv(gpu_device, dtype, *case, "hswish", pool=True)
    y2, _, part2 = _dwconv(gpu_device, dtype, *case, "hswish", pool=True)
    assert torch.isfinite(part).all()
    assert torch.equal(part, part2) and torch.equal(y, y2)
    got = part.double().sum(1)
    want = y.double().sum((1, 2))
    scale = y.double().abs().sum((1, 2)).clamp_min(1.0)       # relative to the summed magnitudes
    err = ((got - want).abs() / scale).max().item()
    print(f"pooled sums max relative |d| {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("bad", [dict(k=4), dict(k=7), dict(stride=3), dict(C=12), dict(H=9, stride=2), dict(act=2)])
def test_dwconv_refuses_shapes_outside_its_contract(gpu_device, bad):
    """k in {3, 5}; stride 1, or 2 with even H and W; C % 8 == 0; act in {0, 1, 4}: SPE_E_ARG, output untouched."""
    a = dict(B=1, H=8, C=16, k=3, stride=1, act=1)
    a.update(bad)
    x = torch.zeros(1, 16, 16, 16, device=gpu_device)
    w = torch.zeros(49, 16, device=gpu_device)
    y = torch.full((1, 16, 16, 16), 7.0, device=gpu_device)
    rc = _lib.lib().spe_debug_dwconv(None, _lib.SPE_DTYPE_F32, _p(x), _p(w), _p(w), _p(y), None, a["B"], a["H"], a["H"],
                                     a["C"], a["k"], a["stride"], a["act"])
    torch.cuda.synchronize()
    assert rc == -1 and (y == 7.0).all()


@pytest.mark.parametrize("C,hidden", [(72, 18), (480, 120), (960, 240), (24, 8)])
def test_se_gate_matches_fp64(gpu_device, C, hidden):
    """pooled mean -> fc1 (+ folded BN) -> ReLU -> fc2 -> Hardsigmoid; (24, 8): the max(C / 4, 8) clamp.
    The gate is fp32 in both model dtypes (its inputs are the fp32 pool partials), so the fp32 gate 1e-5
    holds for bf16 models too (the issue's 2e-2 is the looser one)."""
    dev, B, tiles, hw = gpu_device, 3, 4, 256
    g = torch.Generator().manual_seed(C)
    part = (torch.randn(B, tiles, C, generator=g) * 20.0 + 30.0).to(dev)
    w1 = (torch.randn(hidden, C, generator=g) * (2.0 / C) ** 0.5).to(dev)
    b1 = (torch.randn(hidden, generator=g) * 0.3).to(dev)
    w2 = (torch.randn(C, hidden, generator=g) * 3.0 * (2.0 / hidden) ** 0.5).to(dev)
    scale = torch.empty(B, C, device=dev)
    rc = _lib.lib().spe_debug_se_gate(None, _p(part), tiles, 1.0 / hw, _p(w1), _p(b1), _p(w2.t().contiguous()), _p(scale),
                                      B, C, hidden)
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    mean = part.double().sum(1) / hw
    pre = F.relu(mean @ w1.double().t() + b1.double()) @ w2.double().t()
    ref = F.relu6(pre + 3.0) / 6.0
    assert (pre.abs() > 3).any() and (pre.abs() < 3).any()       # both the linear part and the clamps
    _close(scale, ref, 1e-5)


def _pwconv(dev, dtype, M, K, N, use_scale, use_res, act, rows_per_image=None, res_sign=None, seed=0):
    code, tdt, _ = DT[dtype]
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(tdt).to(dev)
    w = (torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5).to(tdt).to(dev)
    bias = (torch.randn(N, generator=g) * 0.5).to(dev)
    hw = rows_per_image or M
    scale = torch.rand(M // hw, K, generator=g).to(dev) if use_scale else None
    c = torch.empty(M, N, dtype=tdt, device=dev)
    a64 = a.double()
    if use_scale:      # the kernel rounds the scaled operand to the storage type
        a64 = (a.float() * scale.repeat_interleave(hw, 0)).to(tdt).double()
    lin = a64 @ w.double().t() + bias.double()
    r = None
    if use_res:
        r = (torch.randn(M, N, generator=g) * 2.0)
        if res_sign is not None:           # a residual that flips the sign of the sum
            r = -2.0 * lin.float().cpu()
        r = r.to(tdt).to(dev)
        lin = lin + r.double()
    rc = _lib.lib().spe_debug_pwconv(None, code, _p(a), K, _p(w), K, _p(bias), _p(scale), hw, _p(r), N, _p(c), N, M, N, K,
                                     ACTS[act])
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    return c, _act64(lin, act), lin


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("opts", [(False, False, "none"), (True, True, "hswish"), (False, True, "relu"), (True, False, "hswish")],
                         ids=["plain", "scale+res+hswish", "res+relu", "scale+hswish"])
@pytest.mark.parametrize("KN", [(72, 24), (960, 160), (16, 64)], ids=lambda kn: f"K{kn[0]}N{kn[1]}")
@pytest.mark.parametrize("M", [128, 1000])
def test_pwconv_matches_fp64(gpu_device, M, KN, opts, dtype):
    """M = 64 * 2 rows and the ragged M = 1000 (two images of 500 rows for the SE scale)."""
    c, ref, _ = _pwconv(gpu_device, dtype, M, KN[0], KN[1], opts[0], opts[1], opts[2], rows_per_image=M // 2)
    _close(c, ref, DT[dtype][2])


@pytest.mark.parametrize("act", ["relu", "hswish"])
def test_pwconv_activation_follows_the_residual(gpu_device, act):
    """Block.forward is act3(bn3(conv3(.)) + skip).  With r = -2 * (a . w^T + bias) the sum has the opposite sign of
    the product, so act(product) + r and act(product + r) differ wherever the product is positive."""
    c, ref, lin = _pwconv(gpu_device, "fp32", 128, 72, 24, False, True, act, res_sign=-1)
    wrong = _act64(-lin, act) + 2.0 * lin           # act before the residual: (-lin is the product)
    assert (wrong - ref).abs().max().item() > 0.5
    _close(c, ref, 1e-5)


def test_pwconv_refuses_unaligned_shapes(gpu_device):
    t = torch.zeros(64, 64, device=gpu_device)
    L = _lib.lib()
    assert L.spe_debug_pwconv(None, _lib.SPE_DTYPE_F32, _p(t), 60, _p(t), 60, None, None, 64, None, 0, _p(t), 64, 64, 64, 60, 0) == -1
    assert L.spe_debug_pwconv(None, _lib.SPE_DTYPE_F32, _p(t), 64, _p(t), 64, None, None, 64, None, 0, _p(t), 64, 64, 64, 64, 2) == -1


# ---------------------------------------------------------------- the model
_models = {}


def _model(dtype):
    from spe.rtdetr import RTDETR
    if dtype not in _models:
        r = reference_run()
        m = RTDETR(r["cfg"], dtype)
        missing, unexpected = m.load_state_dict(r["w"])
        assert not missing and not unexpected
        _models[dtype] = m
    return _models[dtype]


def _feat_err(dev, dtype):
    r = reference_run()
    feats = _model(dtype).backbone_features(torch.from_numpy(r["batch"]["images"]).to(dev))
    torch.cuda.synchronize()
    errs = []
    for f, t in zip(feats, r["trace"]["feats"]):
        assert f.shape == t.shape
        errs.append((f.cpu() - t).abs().max().item())
    print(dtype, "backbone maps max |d| vs the fp32 restatement:", ["%.3e" % e for e in errs],
          "max |ref|", ["%.2f" % t.abs().max().item() for t in r["trace"]["feats"]])
    return errs


def test_backbone_fp32_matches_restatement(gpu_device):
    """The three maps within 1e-4 (max abs, activations O(1): |ref| up to ~12) of tests/rtdetr_mbv3_ref.py."""
    assert max(_feat_err(gpu_device, "fp32")) <= 1e-4


_bf16_bound = {}


def _bf16_restatement():
    """The CPU restatement with weights and stage outputs rounded to bf16 where the kernels round."""
    if not _bf16_bound:
        r = reference_run()
        rnd = lambda t: t.to(torch.bfloat16).float()
        with torch.no_grad():
            x = torch.from_numpy(r["batch"]["images"])
            feats = rtdetr_mbv3_ref.mobilenetv3_large_rounded(x, r["w"], rnd)
        _bf16_bound["feats"] = feats
        _bf16_bound["err"] = [(a - b).abs().max().item() for a, b in zip(feats, r["trace"]["feats"])]
    return _bf16_bound


def test_backbone_bf16_close_to_restatement(gpu_device):
    """bf16 through 15 SE / Hardswish blocks: gated at twice what the torch-CPU restatement loses against the
    fp32 golden when its weights and stage outputs are rounded to bf16 at the kernels' storage points
    (printed; measured figures in DESIGN.md)."""
    bound = _bf16_restatement()["err"]
    errs = _feat_err(gpu_device, "bf16")
    print("bf16-rounded CPU restatement vs fp32:", ["%.3e" % e for e in bound])
    for e, b in zip(errs, bound):
        assert e <= 2.0 * b


def test_backbone_hook_on_r18_matches_presnet(gpu_device):
    """The same entry point on an r18 handle: the PResNet launches moved into their own function unchanged."""
    from spe.rtdetr import RTDETR
    g = np.load(os.path.join(GOLDEN, "rtdetr_r18_s128.npz"))
    cfg = RtdetrConfig(**json.loads(str(g["config"])))
    w = random_rtdetr_weights(cfg, int(g["weight_seed"]))
    b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
    m = RTDETR(cfg, "fp32")
    m.load_state_dict(w)
    feats = m.backbone_features(torch.from_numpy(b["images"]).to(gpu_device))
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = rtdetr_ref.presnet(torch.from_numpy(b["images"]), w, cfg)
    for i, (f, t) in enumerate(zip(feats, ref)):
        np.testing.assert_allclose(rtdetr_mbv3_chk(f.cpu().numpy()), g[f"chk_feat{i}"], rtol=1e-4)
        assert (f.cpu() - t).abs().max().item() <= 1e-4


def rtdetr_mbv3_chk(a):
    a = np.asarray(a, np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.ravel()[:: max(1, a.size // 97)].sum()])


def _forward(dtype, dev):
    r = reference_run()
    g = r["g"]
    o = _model(dtype)(torch.from_numpy(r["batch"]["images"]).to(dev), clip_bbox=torch.from_numpy(g["clip_bbox"]).float().to(dev))
    torch.cuda.synchronize()
    return g, r["cfg"], o


def test_hip_fp32_matches_reference(gpu_device):
    g, cfg, o = _forward("fp32", gpu_device)
    c = lambda t: t.cpu().numpy()
    aux = o["aux_outputs"]
    fig = {"pred_pts": np.abs(c(o["pred_pts"]) - g["pred_pts"]).max(),
           "pred_logits": np.abs(c(o["pred_logits"]) - g["pred_logits"]).max(),
           "pred_sigmas": np.abs(c(o["pred_sigmas"]) - g["pred_sigmas"]).max(),
           "enc_logits": np.abs(c(aux[-1]["pred_logits"]) - g["enc_topk_logits"]).max()}
    print({k: "%.3e" % v for k, v in fig.items()})
    np.testing.assert_array_equal(c(o["topk"]), g["topk_ind"])
    assert fig["pred_pts"] <= 1e-4 and fig["pred_logits"] <= 2e-3 and fig["pred_sigmas"] <= 2e-3
    assert np.abs(np.stack([c(a["pred_pts"]) for a in aux[:-1]]) - g["aux_pts"]).max() <= 1e-4
    assert np.abs(np.stack([c(a["pred_logits"]) for a in aux[:-1]]) - g["aux_logits"]).max() <= 2e-3
    assert np.abs(np.stack([c(a["pred_sigmas"]) for a in aux[:-1]]) - g["aux_sigmas"]).max() <= 2e-3
    assert np.abs(c(aux[-1]["pred_pts"]) - g["enc_topk_bboxes"]).max() <= 1e-4
    assert fig["enc_logits"] <= 2e-3
    ref = rtdetr_ref.postprocess({k: torch.from_numpy(g[k]) for k in ("pred_logits", "pred_pts", "pred_sigmas")},
                                 g["clip_bbox"])
    assert np.abs(c(o["points_px"]) - ref["points"].numpy()).max() <= 0.05
    assert np.abs(c(o["probs"]) - ref["probs"].numpy()).max() <= 1e-3
    assert np.abs(c(o["sigmas"]) - ref["sigmas"].numpy()).max() <= 5e-3 * max(1.0, float(ref["sigmas"].max()))


def test_hip_bf16_close_to_reference(gpu_device):
    """On queries selected in the same rank: points <= 3.70e-2 and logits <= 0.582 = twice the figures of the
    bf16-rounded torch-CPU restatement against the fp32 golden (1.851e-2, 0.2910;
    tools/measure_bf16_rtdetr_mbv3.py); selected sets overlapping >= 80 %.  The r18 / r50 gates (3e-2, 0.3) do
    not hold here: the HIP model measured 3.26e-2 and 0.332 on image 1 (overlap 30 / 30 and 29 / 30)."""
    g, cfg, o = _forward("bf16", gpu_device)
    sel, ref_sel = o["topk"].cpu().numpy(), g["topk_ind"]
    for b in range(sel.shape[0]):
        overlap = len(set(sel[b]) & set(ref_sel[b]))
        same = sel[b] == ref_sel[b]
        dp = np.abs(o["pred_pts"][b].cpu().numpy()[same] - g["pred_pts"][b][same]).max() if same.any() else 0.0
        dl = np.abs(o["pred_logits"][b].cpu().numpy()[same] - g["pred_logits"][b][same]).max() if same.any() else 0.0
        print(f"image {b}: overlap {overlap}/{cfg.num_queries}, same rank {int(same.sum())}, points {dp:.3e}, logits {dl:.3e}")
        assert overlap >= 0.8 * cfg.num_queries
        assert dp <= 2 * 1.851e-2 and dl <= 2 * 0.2910


def test_hip_batch_independence(gpu_device):
    """Images 1..2 of a batch of 4 give the same top-k and pred_pts (1e-5) as alone: catches pooled sums or
    SE scales that leak across images."""
    r = reference_run()
    m = _model("fp32")
    b = synthetic_batch(SpeConfig(input_size=r["cfg"].input_size), 4, 9)
    x = torch.from_numpy(b["images"]).to(gpu_device)
    full = m(x)
    part = m(x[1:3].contiguous())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(full["topk"][1:3].cpu().numpy(), part["topk"].cpu().numpy())
    assert (full["pred_pts"][1:3] - part["pred_pts"]).abs().max().item() <= 1e-5


def test_postprocessor_and_evaluate_loop(gpu_device):
    """RTDETRPostProcessor and one batch through evaluate_rtdetr produce the log keys they produce for r18."""
    from spe.engine import evaluate_rtdetr
    from spe.rtdetr import RTDETRPostProcessor, build_rtdetr_criterion
    from spe.solver import SimplePoseSolverSigma
    r = reference_run()
    g, cfg = r["g"], r["cfg"]
    m = _model("fp32")
    images = torch.from_numpy(r["batch"]["images"])
    clip = torch.from_numpy(g["clip_bbox"]).float()
    o = m(images.to(gpu_device))
    res = RTDETRPostProcessor()(o, clip)
    assert len(res) == 2 and set(res[0]) == {"logits", "points", "sigmas"}
    assert res[0]["points"].shape == (cfg.num_queries, 2) and res[0]["logits"].shape == (cfg.num_queries, 12)
    names = ["img000000.jpg", "img000001.jpg"]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.1 * i, -0.2, 8.0 + i]} for i, n in enumerate(names)}
    rng = np.random.default_rng(0)
    tg = [{"filename": names[b], "clip_bbox": clip[b], "labels": torch.arange(11),
           "landmarks": torch.from_numpy(rng.uniform(0.1, 0.9, (11, 2)).astype(np.float32))} for b in range(2)]
    crit = build_rtdetr_criterion(cfg)
    stats, ev = evaluate_rtdetr(m, crit, {"bbox": RTDETRPostProcessor()}, [(images, tg)], gt, SimplePoseSolverSigma(),
                                gpu_device)
    keys = ["class_error", "loss_ce", "loss_bbox"] + [f"{k}_aux_{i}" for i in range(3) for k in ("loss_ce", "loss_bbox")]
    assert set(stats) == {"loss", "class_error", "loss_ce", "loss_bbox", "speed_eval_pose"} | {k + "_unscaled" for k in keys}
    assert list(ev.log) == names
    for n in names:
        assert {"points", "logits", "quat_pr", "tvec_pr", "score", "sigma", "aux_points_0", "aux_points_1",
                "aux_points_2"} <= set(ev.log[n])
