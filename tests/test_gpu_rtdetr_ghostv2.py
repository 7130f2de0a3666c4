"""UNC RT-DETR behind the GhostNetV2 backbone, GPU side: the new gfx950 kernels (ghostv2.hip, the biased SE
gate) one by one against fp64 torch on the same dtype-rounded operands, the backbone stage against the
torch-fp32 restatement (tests/rtdetr_ghostv2_ref.py), and the whole model against the reference's golden
(tests/golden/rtdetr_ghostv2_s256.npz).

Gates.  Kernels: tests/test_gpu_rtdetr_mbv3.py's, relative to max(1, max |ref|): 1e-5 fp32, 2e-2 bf16.
Backbone: fp32 within 1e-4 of the restatement; bf16 within twice what the bf16-rounded CPU restatement loses
against the fp32 one (computed here).  Whole model, fp32: the RT-DETR contract of tests/test_rtdetr.py
(pred_pts 1e-4, logits / sigmas 2e-3, top-k exact; the golden's topk_min_gap is 3.781e-4 against a
restatement-vs-reference encoder score difference of 3.815e-6).  bf16, on queries selected in the same rank:
twice what tools/measure_bf16_rtdetr_ghostv2.py prints for the bf16-rounded CPU restatement against the fp32
golden (points 8.258e-3, logits 0.1817, overlap 29 / 30 and 30 / 30): points <= 1.652e-2, logits <= 0.3633;
selected sets overlapping >= 80 %.

A ghost half that is not a multiple of 8 (12, 20, 36, 60, 92, 100) is stored padded to 8 with zero weights and
bias; the kernels take the padded width, and the tests check that the pad lanes come out exactly 0.
"""
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
import rtdetr_ghostv2_ref
from test_rtdetr_ghostv2 import reference_run

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32, 1e-5), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16, 2e-2)}
POST = {"none": 0, "gate": 1, "resid": 2}


def _p(t):
    return _lib.ptr(t)


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.double() - ref.double()).abs().max().item()
    print(f"max |d| {err:.3e} (gate {tol * scale:.3e})")
    assert err <= tol * scale, (err, scale)


def _pad8(n):
    return (n + 7) // 8 * 8


def _lanes(half):
    """mask [2 hp] of the real lanes of a padded ghost tensor"""
    hp = _pad8(half)
    m = torch.zeros(2 * hp, dtype=torch.bool)
    m[:half] = True
    m[hp:hp + half] = True
    return m


def _cheap(dev, dtype, B, half, H, post, act, pool, seed=0):
    """x1 is channels [8, 8 + hp) of a [B][H][H][hp + 16] tensor; pad lanes of x1, w, bias, resid are zero."""
    code, tdt, _ = DT[dtype]
    hp, g = _pad8(half), torch.Generator().manual_seed(seed)
    real = _lanes(half)[:hp].float()
    wide = (torch.randn(B, H, H, hp + 16, generator=g) * 2.0)
    wide[..., 8:8 + hp] *= real
    wide = wide.to(tdt).to(dev)
    w = (torch.randn(9, hp, generator=g) * 0.5 * real).to(dev)
    bias = (torch.randn(hp, generator=g) * 0.5 * real).to(dev)
    gate = torch.rand(B, H // 2, H // 2, 2 * hp, generator=g).to(tdt).to(dev) if post == "gate" else None
    resid = (torch.randn(B, H, H, 2 * hp, generator=g) * 2.0 * _lanes(half).float()).to(tdt).to(dev) if post == "resid" else None
    y = torch.full((B, H, H, 2 * hp), float("nan"), dtype=tdt, device=dev)
    tiles = _lib.lib().spe_debug_dwconv_tiles(H, H)
    part = torch.full((B, tiles, 2 * hp), float("nan"), device=dev) if pool else None
    rc = _lib.lib().spe_debug_ghost_cheap(None, code, _p(wide), hp + 16, 8, _p(w), _p(bias), _p(y), _p(gate), _p(resid),
                                          _p(part), B, H, H, hp, 1 if act == "relu" else 0, POST[post])
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    x1 = wide[..., 8:8 + hp].double().permute(0, 3, 1, 2)
    w64 = w.double().t().reshape(hp, 1, 3, 3)

    def cheap_of(x):
        x2 = F.conv2d(x, w64, bias.double(), 1, 1, 1, hp)
        return F.relu(x2) if act == "relu" else x2
    ref = torch.cat([x1, cheap_of(x1)], 1)
    extra = {}
    if post == "gate":
        up = F.interpolate(gate.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        ref = ref * up
        extra["gated_first"] = torch.cat([x1 * up[:, :hp], cheap_of(x1 * up[:, :hp]) * up[:, hp:]], 1).permute(0, 2, 3, 1)
    elif post == "resid":
        ref = ref + resid.double().permute(0, 3, 1, 2)
    return y, ref.permute(0, 2, 3, 1), part, extra


# (B, half, H): one aligned vector / a pad (12 -> 16) / a pad at width (92 -> 96) / wide; maps 8, 16, 64 and a
# map that is no multiple of the 8 x 8 tile
CHEAP_CASES = [(2, 8, 64), (3, 12, 16), (1, 92, 16), (2, 480, 8), (1, 12, 8), (2, 20, 12)]
CHEAP_MODES = [("none", "relu"), ("gate", "relu"), ("resid", "none")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("mode", CHEAP_MODES, ids=lambda m: "+".join(m))
@pytest.mark.parametrize("case", CHEAP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_ghost_cheap_matches_fp64(gpu_device, case, mode, pool, dtype):
    B, half, H = case
    y, ref, part, _ = _cheap(gpu_device, dtype, B, half, H, mode[0], mode[1], pool)
    _close(y, ref, DT[dtype][2])
    pad = ~_lanes(half)
    assert (y[..., pad.to(y.device)] == 0).all()           # pad lanes: exactly 0 through act, gate, residual
    if pool:
        y2, _, part2, _ = _cheap(gpu_device, dtype, B, half, H, mode[0], mode[1], pool)
        assert torch.isfinite(part).all()                   # every partial written
        assert torch.equal(part, part2) and torch.equal(y, y2)
        got, want = part.double().sum(1), y.double().sum((1, 2))
        scale = y.double().abs().sum((1, 2)).clamp_min(1.0)
        err = ((got - want).abs() / scale).max().item()
        print(f"pooled sums max relative |d| {err:.3e}")
        assert err <= 1e-5
        assert (part[..., pad.to(part.device)] == 0).all()


def test_ghost_cheap_gate_follows_the_cheap_operation(gpu_device):
    """GhostModuleV2.forward gates cat(x1, cheap(x1)): the depthwise conv reads the UNGATED x1.  Gating x1
    first gives a visibly different second half."""
    y, ref, _, extra = _cheap(gpu_device, "fp32", 2, 12, 16, "gate", "relu", False)
    assert (extra["gated_first"] - ref).abs().max().item() > 0.5
    _close(y, ref, 1e-5)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [(2, 4, 16), (1, 8, 200), (2, 32, 960), (3, 4, 960), (1, 32, 16), (2, 8, 960)],
                         ids=lambda c: "x".join(map(str, c)))
def test_dfc_gate_matches_fp64(gpu_device, case, dtype):
    """(B, pooled edge, C): 4 x 4 is narrower than the 5-tap window (both pads overlap); the whole 32 x 32 map."""
    B, H, C = case
    code, tdt, tol = DT[dtype]
    dev, g = gpu_device, torch.Generator().manual_seed(H * C)
    x = (torch.randn(B, H, H, C, generator=g) * 2.0).to(tdt).to(dev)
    w1, w2 = ((torch.randn(5, C, generator=g) * 0.7).to(dev) for _ in range(2))
    b1, b2 = ((torch.randn(C, generator=g) * 0.5).to(dev) for _ in range(2))
    gate = torch.full((B, H, H, C), float("nan"), dtype=tdt, device=dev)
    rc = _lib.lib().spe_debug_dfc_gate(None, code, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(gate), B, H, H, C)
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    t = F.conv2d(x.double().permute(0, 3, 1, 2), w1.double().t().reshape(C, 1, 1, 5), b1.double(), 1, (0, 2), 1, C)
    pre = F.conv2d(t, w2.double().t().reshape(C, 1, 5, 1), b2.double(), 1, (2, 0), 1, C)
    ref = torch.sigmoid(pre).permute(0, 2, 3, 1)
    assert (pre < -8).any() and (pre > 8).any() and (pre.abs() < 1).any()       # both saturated ends, both sides of 0.5
    _close(gate, ref, tol)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("HKN", [(8, 160, 960), (64, 24, 72)], ids=lambda c: "x".join(map(str, c)))
def test_pool2_then_pwconv_matches_fp64(gpu_device, HKN, dtype):
    """The DFC branch's front: 2 x 2 mean (stored in dtype), then the 1x1 conv."""
    H, K, N = HKN
    code, tdt, tol = DT[dtype]
    dev, B, g = gpu_device, 2, torch.Generator().manual_seed(K)
    x = (torch.randn(B, H, H, K, generator=g) * 2.0).to(tdt).to(dev)
    w = (torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5).to(tdt).to(dev)
    bias = (torch.randn(N, generator=g) * 0.5).to(dev)
    xp = torch.full((B, H // 2, H // 2, K), float("nan"), dtype=tdt, device=dev)
    M = B * (H // 2) ** 2
    c = torch.empty(M, N, dtype=tdt, device=dev)
    L = _lib.lib()
    assert L.spe_debug_pool2(None, code, _p(x), _p(xp), B, H, H, K) == 0, L.spe_last_error()
    assert L.spe_debug_pwconv(None, code, _p(xp), K, _p(w), K, _p(bias), None, M, None, 0, _p(c), N, M, N, K, 0) == 0
    torch.cuda.synchronize()
    p64 = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    _close(xp, p64, tol)
    ref = p64.to(tdt).double().reshape(M, K) @ w.double().t() + bias.double()
    _close(c, ref, tol)


@pytest.mark.parametrize("C,hidden", [(72, 20), (672, 168), (960, 240)])
def test_se_gate_bias_matches_fp64(gpu_device, C, hidden):
    """SqueezeExcite with both conv biases: pooled mean -> fc1 + b1 -> ReLU -> fc2 + b2 -> Hardsigmoid (fp32 in
    both model dtypes: gate 1e-5)."""
    dev, B, tiles, hw = gpu_device, 3, 4, 256
    g = torch.Generator().manual_seed(C)
    part = (torch.randn(B, tiles, C, generator=g) * 20.0 + 30.0).to(dev)
    w1 = (torch.randn(hidden, C, generator=g) * (2.0 / C) ** 0.5).to(dev)
    b1 = (torch.randn(hidden, generator=g) * 0.3).to(dev)
    w2 = (torch.randn(C, hidden, generator=g) * 2.0 * (2.0 / hidden) ** 0.5).to(dev)
    b2 = (torch.randn(C, generator=g) * 1.5).to(dev)
    scale = torch.full((B, C), float("nan"), device=dev)
    w2t = w2.t().contiguous()
    L = _lib.lib()
    rc = L.spe_debug_se_gate_bias(None, _p(part), tiles, 1.0 / hw, _p(w1), _p(b1), _p(w2t), _p(b2), _p(scale), B, C, hidden)
    assert rc == 0, L.spe_last_error()
    plain = torch.empty(B, C, device=dev)
    assert L.spe_debug_se_gate(None, _p(part), tiles, 1.0 / hw, _p(w1), _p(b1), _p(w2t), _p(plain), B, C, hidden) == 0
    torch.cuda.synchronize()
    mean = part.double().sum(1) / hw
    lin = F.relu(mean @ w1.double().t() + b1.double()) @ w2.double().t()
    pre = lin + b2.double()
    assert (pre > 3).any() and (pre < -3).any() and ((pre > -3) & (pre < 0)).any() and ((pre > 0) & (pre < 3)).any()
    _close(scale, F.relu6(pre + 3.0) / 6.0, 1e-5)
    _close(plain, F.relu6(lin + 3.0) / 6.0, 1e-5)          # the unbiased entry is what it was


@pytest.mark.parametrize("bad", [dict(half=12), dict(half=0), dict(post=3), dict(act=4), dict(act=2), dict(post=1, H=9),
                                 dict(ldx=20), dict(xoff=4)], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_ghost_cheap_refuses_shapes_outside_its_contract(gpu_device, bad):
    """half, ldx, xoff multiples of 8 (a narrower half is stored padded); act 0 / 1; post 0 / 1 / 2; even map
    under the gate: -1 before any launch, output untouched."""
    a = dict(H=8, half=16, act=1, post=0, ldx=16, xoff=0)
    a.update(bad)
    z = torch.zeros(1, 16, 16, 32, device=gpu_device)
    y = torch.full((1, 16, 16, 32), 7.0, device=gpu_device)
    rc = _lib.lib().spe_debug_ghost_cheap(None, _lib.SPE_DTYPE_F32, _p(z), a["ldx"], a["xoff"], _p(z), _p(z), _p(y), _p(z), _p(z),
                                          None, 1, a["H"], a["H"], a["half"], a["act"], a["post"])
    torch.cuda.synchronize()
    assert rc == -1 and (y == 7.0).all()


def test_pool2_and_dfc_gate_refuse_shapes_outside_their_contracts(gpu_device):
    """pool2: odd H or W, C % 8; dfc_gate: a map wider than 32, C % 8: -1 before any launch, output untouched."""
    L = _lib.lib()
    z = torch.zeros(1, 40, 40, 16, device=gpu_device)
    y = torch.full((1, 40, 40, 16), 7.0, device=gpu_device)
    f32 = _lib.SPE_DTYPE_F32
    assert L.spe_debug_pool2(None, f32, _p(z), _p(y), 1, 9, 8, 16) == -1
    assert L.spe_debug_pool2(None, f32, _p(z), _p(y), 1, 8, 7, 16) == -1
    assert L.spe_debug_pool2(None, f32, _p(z), _p(y), 1, 8, 8, 12) == -1
    assert L.spe_debug_dfc_gate(None, f32, _p(z), _p(z), _p(z), _p(z), _p(z), _p(y), 1, 33, 8, 16) == -1
    assert L.spe_debug_dfc_gate(None, f32, _p(z), _p(z), _p(z), _p(z), _p(z), _p(y), 1, 8, 8, 12) == -1
    assert L.spe_debug_se_gate_bias(None, _p(z), 1, 1.0, _p(z), _p(z), _p(z), None, _p(y), 1, 16, 8) == -1
    torch.cuda.synchronize()
    assert (y == 7.0).all()


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
    """The three maps within 1e-4 (max abs; |ref| up to ~13) of tests/rtdetr_ghostv2_ref.py."""
    assert max(_feat_err(gpu_device, "fp32")) <= 1e-4


def test_backbone_bf16_close_to_restatement(gpu_device):
    """bf16 through 16 ghost bottlenecks: gated at twice what the torch-CPU restatement loses against the fp32
    one when the MFMA weights and every stage output are rounded to bf16 at the kernels' storage points
    (computed here and printed: 3.70e-2, 6.03e-2, 7.98e-2; measured figures in DESIGN.md)."""
    r = reference_run()
    rnd = lambda t: t.to(torch.bfloat16).float()
    with torch.no_grad():
        feats = rtdetr_ghostv2_ref.ghostnetv2_rounded(torch.from_numpy(r["batch"]["images"]), r["w"], rnd)
    bound = [(a - b).abs().max().item() for a, b in zip(feats, r["trace"]["feats"])]
    errs = _feat_err(gpu_device, "bf16")
    print("bf16-rounded CPU restatement vs fp32:", ["%.3e" % e for e in bound])
    for e, b in zip(errs, bound):
        assert e <= 2.0 * b


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
    """On queries selected in the same rank: points <= 1.652e-2 and logits <= 0.3633 = twice the figures of the
    bf16-rounded torch-CPU restatement against the fp32 golden (8.258e-3, 0.1817;
    tools/measure_bf16_rtdetr_ghostv2.py); selected sets overlapping >= 80 %.  The HIP model measured points
    5.58e-3 / 6.84e-3 and logits 0.101 / 0.094 on the two images (overlap 29 / 30 and 30 / 30), so the r18 gates
    (3e-2, 0.3) would hold as well; the figures are in DESIGN.md 3n."""
    g, cfg, o = _forward("bf16", gpu_device)
    sel, ref_sel = o["topk"].cpu().numpy(), g["topk_ind"]
    for b in range(sel.shape[0]):
        overlap = len(set(sel[b]) & set(ref_sel[b]))
        same = sel[b] == ref_sel[b]
        dp = np.abs(o["pred_pts"][b].cpu().numpy()[same] - g["pred_pts"][b][same]).max() if same.any() else 0.0
        dl = np.abs(o["pred_logits"][b].cpu().numpy()[same] - g["pred_logits"][b][same]).max() if same.any() else 0.0
        print(f"image {b}: overlap {overlap}/{cfg.num_queries}, same rank {int(same.sum())}, points {dp:.3e}, logits {dl:.3e}")
        assert overlap >= 0.8 * cfg.num_queries
        assert dp <= 2 * 8.258e-3 and dl <= 2 * 0.1817


def test_hip_batch_independence(gpu_device):
    """Images 1..2 of a batch of 4 give the same top-k and pred_pts (1e-5) as alone: catches pool partials, SE
    scales or DFC gates that leak across images."""
    r = reference_run()
    m = _model("fp32")
    b = synthetic_batch(SpeConfig(input_size=r["cfg"].input_size), 4, 9)
    x = torch.from_numpy(b["images"]).to(gpu_device)
    full = m(x)
    part = m(x[1:3].contiguous())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(full["topk"][1:3].cpu().numpy(), part["topk"].cpu().numpy())
    assert (full["pred_pts"][1:3] - part["pred_pts"]).abs().max().item() <= 1e-5


def test_backbone_hook_on_the_other_families_unchanged(gpu_device):
    """spe_debug_rtdetr_backbone on an r18 and on a MobileNetV3_Large handle still gives their restatements
    within 1e-4: nothing moved."""
    from spe.rtdetr import RTDETR
    import test_rtdetr_mbv3
    g = np.load(os.path.join(GOLDEN, "rtdetr_r18_s128.npz"))
    cfg = RtdetrConfig(**json.loads(str(g["config"])))
    w = random_rtdetr_weights(cfg, int(g["weight_seed"]))
    b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
    with torch.no_grad():
        runs = [(cfg, w, b["images"], rtdetr_ref.presnet(torch.from_numpy(b["images"]), w, cfg))]
    r = test_rtdetr_mbv3.reference_run()
    runs.append((r["cfg"], r["w"], r["batch"]["images"], r["trace"]["feats"]))
    for cfg, w, images, ref in runs:
        m = RTDETR(cfg, "fp32")
        m.load_state_dict(w)
        feats = m.backbone_features(torch.from_numpy(images).to(gpu_device))
        torch.cuda.synchronize()
        for f, t in zip(feats, ref):
            assert (f.cpu() - t).abs().max().item() <= 1e-4
