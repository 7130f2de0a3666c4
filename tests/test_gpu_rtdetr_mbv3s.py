"""UNC RT-DETR behind the MobileNetV3_Small backbone, GPU side: the fused entry kernel (csrc/mbv3s.hip) against
fp64 (tests/rtdetr_mbv3s_ref.py) next to the launch-per-layer sequence of the existing kernels on the same
inputs, the backbone stage against the torch-fp32 restatement and the whole model against the reference's golden
(tests/golden/rtdetr_mbv3s_s256.npz) -- through the fused entry and through the unfused path, each in a child
process of its own (the library reads SPE_MBS_ENTRY once per process).

Gates.  Entry kernel: per output, max |fused - fp64| <= 2 x max |unfused - fp64| (same precision class, another
summation order; in bf16 the fused path rounds once where the unfused one rounds the stem map and the expanded
map too).  Pool partials: 1e-5 of the summed magnitudes (fp32 summation of 64 values), as test_dwconv_pooled_sums.
Model: tests/test_gpu_rtdetr_mbv3.py's -- backbone fp32 1e-4 against the restatement; bf16 backbone twice what
the CPU restatement loses with bf16 storage points; whole model fp32 pred_pts 1e-4, logits / sigmas 2e-3, top-k
exact; bf16 points 3.70e-2, logits 0.582 on queries selected in the same rank, selected sets overlapping >= 80 %.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from spe import _lib
from spe.config import SpeConfig
from spe.synthetic import synthetic_batch
import rtdetr_ref
import rtdetr_mbv3s_ref as R
from test_rtdetr_mbv3s import reference_run

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16)}
OUTS = ("pooled", "skip", "t2")
_p = _lib.ptr


# ---------------------------------------------------------------- the entry kernel
def _source(kind, B, S, seed):
    """(fp32 batch on the CPU, crops or None): a normal batch, or random 8-bit crops with 0 / 255 borders."""
    g = torch.Generator().manual_seed(seed)
    if kind == "f32":
        return torch.randn(B, 3, S, S, generator=g) * 1.5, None
    c = torch.randint(0, 256, (B, S, S) + ((3,) if kind == "rgb" else ()), dtype=torch.uint8, generator=g)
    c[:, 0], c[:, -1] = 0, 255
    c[:, :, 0], c[:, :, -1] = 255, 0
    return R.normalise_crops(c), c


def _fused(dev, dtype, x, crops, wbuf):
    code, tdt = DT[dtype]
    B, S = x.shape[0], x.shape[-1]
    G = S // 4
    tiles = _lib.lib().spe_debug_mbs_entry_tiles(S)
    assert tiles == ((G + 7) // 8) ** 2
    o = {k: torch.full((B, G, G, 16), float("nan"), dtype=tdt, device=dev) for k in OUTS}
    part = torch.full((B, tiles, 16), float("nan"), device=dev)
    xd = x.to(dev).contiguous() if crops is None else None
    cd = crops.to(dev).contiguous() if crops is not None else None
    ch = 0 if crops is None else (3 if crops.dim() == 4 else 1)
    rc = _lib.lib().spe_debug_mbs_entry(None, code, _p(xd), _p(cd), ch, _p(wbuf.to(dev)), _p(o["pooled"]), _p(o["skip"]),
                                        _p(o["t2"]), _p(part), B, S)
    assert rc == 0, _lib.lib().spe_last_error()
    torch.cuda.synchronize()
    return o, part


def _unfused(dev, dtype, x, crops, wbuf):
    """The launch-per-layer sequence of the kernels the model had before: mb_stem -> {pool2, skip dwconv,
    expand pwconv -> dwconv}, every intermediate stored in the storage type."""
    code, tdt = DT[dtype]
    L = _lib.lib()
    B, S = x.shape[0], x.shape[-1]
    H1, G = S // 2, S // 4
    wd = wbuf.to(dev)
    sl = lambda a, n: wd[a:a + n].contiguous()
    stem = torch.empty(B, H1, H1, 16, dtype=tdt, device=dev)
    xd = x.to(dev).contiguous() if crops is None else None
    cd = crops.to(dev).contiguous() if crops is not None else None
    ch = 0 if crops is None else (3 if crops.dim() == 4 else 1)
    assert L.spe_debug_mb_stem(None, code, _p(xd), _p(cd), ch, _p(sl(R.W_STEM, 432)), _p(sl(R.W_STEM_B, 16)), _p(stem), B, S) == 0
    o = {k: torch.empty(B, G, G, 16, dtype=tdt, device=dev) for k in OUTS}
    assert L.spe_debug_pool2(None, code, _p(stem), _p(o["pooled"]), B, H1, H1, 16) == 0
    assert L.spe_debug_dwconv(None, code, _p(stem), _p(sl(R.W_SKIP, 144)), _p(sl(R.W_SKIP_B, 16)), _p(o["skip"]), None,
                              B, H1, H1, 16, 3, 2, 0) == 0
    we = sl(R.W_EXP, 256).reshape(16, 16).t().contiguous().to(tdt)           # rows [co][ci]
    exp = torch.empty(B, H1, H1, 16, dtype=tdt, device=dev)
    M = B * H1 * H1
    assert L.spe_debug_pwconv(None, code, _p(stem), 16, _p(we), 16, _p(sl(R.W_EXP_B, 16)), None, M, None, 0, _p(exp), 16,
                              M, 16, 16, 1) == 0, L.spe_last_error()
    part = torch.empty(B, L.spe_debug_dwconv_tiles(G, G), 16, device=dev)
    assert L.spe_debug_dwconv(None, code, _p(exp), _p(sl(R.W_DW, 144)), _p(sl(R.W_DW_B, 16)), _p(o["t2"]), _p(part),
                              B, H1, H1, 16, 3, 2, 1) == 0
    torch.cuda.synchronize()
    return o, part


_cases = {}


def _case(dev, dtype, kind, S, B):
    key = (dtype, kind, S, B)
    if key not in _cases:
        x, crops = _source(kind, B, S, 17 * S + B)
        wbuf = R.entry_random_weights(S)
        ref = R.entry_ref64(x, wbuf)
        _cases[key] = dict(x=x, crops=crops, wbuf=wbuf, ref=ref, fused=_fused(dev, dtype, x, crops, wbuf),
                           unfused=_unfused(dev, dtype, x, crops, wbuf))
    return _cases[key]


SIZES = [(64, 3), (96, 2)]       # a 16 x 16 grid: 4 tiles, each on two borders; 24 x 24: 9 tiles, one interior


@pytest.mark.parametrize("S,B", SIZES)
@pytest.mark.parametrize("kind", ["f32", "gray", "rgb"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_entry_matches_fp64_like_the_unfused_sequence(gpu_device, dtype, kind, S, B):
    c = _case(gpu_device, dtype, kind, S, B)
    # a border padded with act(bias) instead of zero would move the border outputs by far more than any gate
    sb = c["wbuf"][R.W_STEM_B:R.W_STEM_B + 16].double()
    assert (sb * torch.clamp(sb + 3, 0, 6) / 6).abs().min().item() > 0.05
    fig = {}
    for k in OUTS:
        ref = c["ref"][k]
        ef = (c["fused"][0][k].double().cpu() - ref).abs().max().item()
        eu = (c["unfused"][0][k].double().cpu() - ref).abs().max().item()
        print(f"{dtype} {kind} S={S} {k}: fused {ef:.3e} unfused {eu:.3e} (max |ref| {ref.abs().max().item():.2f})")
        assert torch.isfinite(c["fused"][0][k]).all()
        fig[k] = (ef, eu)
    for k, (ef, eu) in fig.items():
        assert ef <= 2.0 * eu, (k, ef, eu)


@pytest.mark.parametrize("S,B", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_entry_pool_partials(gpu_device, dtype, S, B):
    """Every [b][tile][c] is the fp64 sum of that tile's stored t2 values; the total is the whole stored map's."""
    c = _case(gpu_device, dtype, "f32", S, B)
    o, part = c["fused"]
    G, T = S // 4, (S // 4 + 7) // 8
    t2 = o["t2"].double().cpu()
    pad = T * 8 - G
    t2p = torch.nn.functional.pad(t2, (0, 0, 0, pad, 0, pad))
    want = t2p.reshape(B, T, 8, T, 8, 16).sum((2, 4)).reshape(B, T * T, 16)
    mag = t2p.abs().reshape(B, T, 8, T, 8, 16).sum((2, 4)).reshape(B, T * T, 16).clamp_min(1.0)
    got = part.double().cpu()
    assert torch.isfinite(got).all()
    err = ((got - want).abs() / mag).max().item()
    tot = ((got.sum(1) - t2.sum((1, 2))).abs() / t2.abs().sum((1, 2)).clamp_min(1.0)).max().item()
    print(f"pool partials max relative |d| {err:.3e}, totals {tot:.3e}")
    assert err <= 1e-5 and tot <= 1e-5
    o2, part2 = _fused(gpu_device, dtype, c["x"], None, c["wbuf"])
    assert torch.equal(part, part2) and all(torch.equal(o[k], o2[k]) for k in OUTS)     # fixed-order reduction


@pytest.mark.parametrize("kind", ["gray", "rgb"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_entry_u8_equals_the_normalised_batch_bit_for_bit(gpu_device, dtype, kind):
    c = _case(gpu_device, dtype, kind, 96, 2)
    o, part = c["fused"]                                   # from the crops
    o2, part2 = _fused(gpu_device, dtype, c["x"], None, c["wbuf"])   # from the batch normalised from them
    for k in OUTS:
        assert torch.equal(o[k], o2[k]), k
    assert torch.equal(part, part2)


@pytest.mark.parametrize("S", [40, 16])
def test_entry_refuses_other_sizes(gpu_device, S):
    t = torch.full((1, 16, 16, 16), 7.0, device=gpu_device)
    x = torch.zeros(1, 3, 64, 64, device=gpu_device)
    w = torch.zeros(_lib.MBS_W_FLOATS, device=gpu_device)
    rc = _lib.lib().spe_debug_mbs_entry(None, _lib.SPE_DTYPE_F32, _p(x), None, 0, _p(w), _p(t), _p(t), _p(t), None, 1, S)
    torch.cuda.synchronize()
    assert rc == -1 and (t == 7.0).all()
    assert _lib.lib().spe_debug_mbs_entry_tiles(S) == 0


# ---------------------------------------------------------------- the model, one child process a path
_child = {}


def _run_child(entry):
    """The golden batch through the fp32 and bf16 models with SPE_MBS_ENTRY = 1 (fused) / 0 (unfused)."""
    if entry not in _child:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "out.npz")
            env = dict(os.environ, SPE_MBS_ENTRY="1" if entry == "fused" else "0")
            script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rtdetr_mbv3s_child.py")
            r = subprocess.run([sys.executable, script, out], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            with np.load(out) as z:
                _child[entry] = {k: z[k] for k in z.files}
        assert int(_child[entry]["entry"]) == (1 if entry == "fused" else 0)
    return _child[entry]


PATHS = ["fused", "unfused"]


@pytest.mark.parametrize("entry", PATHS)
def test_backbone_fp32_matches_restatement(gpu_device, entry):
    z, r = _run_child(entry), reference_run()
    errs = [np.abs(z[f"fp32_feat{i}"] - t.numpy()).max() for i, t in enumerate(r["trace"]["feats"])]
    print(entry, "fp32 backbone maps max |d| vs the restatement:", ["%.3e" % e for e in errs])
    assert max(errs) <= 1e-4


_bf16_bound = {}


@pytest.mark.parametrize("entry", PATHS)
def test_backbone_bf16_close_to_restatement(gpu_device, entry):
    """Twice what the torch-CPU restatement loses against fp32 with its weights and stage outputs rounded to bf16
    at this path's storage points (printed; measured figures in DESIGN.md)."""
    z, r = _run_child(entry), reference_run()
    if entry not in _bf16_bound:
        rnd = lambda t: t.to(torch.bfloat16).float()
        with torch.no_grad():
            feats = R.mobilenetv3_small_rounded(torch.from_numpy(r["batch"]["images"]), r["w"], rnd, fused=entry == "fused")
        _bf16_bound[entry] = [(a - b).abs().max().item() for a, b in zip(feats, r["trace"]["feats"])]
    errs = [np.abs(z[f"bf16_feat{i}"] - t.numpy()).max() for i, t in enumerate(r["trace"]["feats"])]
    print(entry, "bf16 backbone maps max |d|:", ["%.3e" % e for e in errs], "bf16-rounded CPU restatement:",
          ["%.3e" % e for e in _bf16_bound[entry]])
    for e, b in zip(errs, _bf16_bound[entry]):
        assert e <= 2.0 * b


@pytest.mark.parametrize("entry", PATHS)
def test_hip_fp32_matches_reference(gpu_device, entry):
    z, g = _run_child(entry), reference_run()["g"]
    d = lambda a, b: float(np.abs(z["fp32_" + a] - g[b]).max())
    fig = {k: d(k, k) for k in ("pred_pts", "pred_logits", "pred_sigmas")}
    fig["enc_logits"] = d("enc_logits", "enc_topk_logits")
    print(entry, {k: "%.3e" % v for k, v in fig.items()})
    np.testing.assert_array_equal(z["fp32_topk"], g["topk_ind"])
    assert fig["pred_pts"] <= 1e-4 and fig["pred_logits"] <= 2e-3 and fig["pred_sigmas"] <= 2e-3
    assert d("aux_pred_pts", "aux_pts") <= 1e-4 and d("aux_pred_logits", "aux_logits") <= 2e-3
    assert d("aux_pred_sigmas", "aux_sigmas") <= 2e-3
    assert d("enc_pts", "enc_topk_bboxes") <= 1e-4 and fig["enc_logits"] <= 2e-3
    ref = rtdetr_ref.postprocess({k: torch.from_numpy(g[k]) for k in ("pred_logits", "pred_pts", "pred_sigmas")},
                                 g["clip_bbox"])
    assert np.abs(z["fp32_points_px"] - ref["points"].numpy()).max() <= 0.05
    assert np.abs(z["fp32_probs"] - ref["probs"].numpy()).max() <= 1e-3
    assert np.abs(z["fp32_sigmas"] - ref["sigmas"].numpy()).max() <= 5e-3 * max(1.0, float(ref["sigmas"].max()))


@pytest.mark.parametrize("entry", PATHS)
def test_hip_bf16_close_to_reference(gpu_device, entry):
    """The Large test's gates: on queries selected in the same rank points <= 3.70e-2, logits <= 0.582; selected
    sets overlapping >= 80 %."""
    z, r = _run_child(entry), reference_run()
    g, Q = r["g"], r["cfg"].num_queries
    sel, ref_sel = z["bf16_topk"], g["topk_ind"]
    for b in range(sel.shape[0]):
        overlap = len(set(sel[b]) & set(ref_sel[b]))
        same = sel[b] == ref_sel[b]
        dp = np.abs(z["bf16_pred_pts"][b][same] - g["pred_pts"][b][same]).max() if same.any() else 0.0
        dl = np.abs(z["bf16_pred_logits"][b][same] - g["pred_logits"][b][same]).max() if same.any() else 0.0
        print(f"{entry} image {b}: overlap {overlap}/{Q}, same rank {int(same.sum())}, points {dp:.3e}, logits {dl:.3e}")
        assert overlap >= 0.8 * Q
        assert dp <= 3.70e-2 and dl <= 0.582


# ---------------------------------------------------------------- the model in this process (the default path)
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


def test_hip_batch_independence(gpu_device):
    """Image 0 of a batch of 3 gives the same top-k and pred_pts (1e-5) as alone: catches image strides, pool
    partials or SE scales that leak across images."""
    m = _model("fp32")
    b = synthetic_batch(SpeConfig(input_size=256), 3, 9)
    x = torch.from_numpy(b["images"]).to(gpu_device)
    full, one = m(x), m(x[:1].contiguous())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(full["topk"][:1].cpu().numpy(), one["topk"].cpu().numpy())
    assert (full["pred_pts"][:1] - one["pred_pts"]).abs().max().item() <= 1e-5


def _flat(o, prefix=""):
    for k, v in (o.items() if isinstance(o, dict) else enumerate(o)):
        if torch.is_tensor(v):
            yield f"{prefix}{k}", v
        else:
            yield from _flat(v, f"{prefix}{k}.")


def _same(got, ref, what):
    got, ref = dict(_flat(got)), dict(_flat(ref))
    assert list(got) == list(ref) and "aux_outputs.0.pred_sigmas" in got, what
    for k in ref:
        assert torch.equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stages_and_u8_equal_the_one_call_forward(gpu_device, dtype):
    """fp32 batch: encode + decode and backbone + transformer + decode are bit-identical to forward; 8-bit crops
    (gray and RGB) are bit-identical to the batch normalised from them, in one call and in stages."""
    m, B, dev = _model(dtype), 3, gpu_device
    clip = torch.tensor([[100.0, 80.0, 700.0, 640.0]] * B, device=dev)
    for kind in ("gray", "rgb"):
        x, crops = _source(kind, B, 256, 5)
        x, crops = x.to(dev), crops.to(dev)
        ref = m(x, clip_bbox=clip)
        ws = m.new_workspace(B, dev)
        m.encode(x, ws)
        _same(m.decode(B, ws, clip_bbox=clip), ref, (kind, "encode + decode"))
        for src in (x, crops):
            ws3 = m.new_workspace(B, dev)
            m.encode(src, ws3, part="backbone")
            m.encode(None, ws3, part="transformer", B=B)
            _same(m.decode(B, ws3, clip_bbox=clip), ref, (kind, str(src.dtype), "three stages"))
        _same(m(crops, clip_bbox=clip), ref, (kind, "u8 forward"))
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for _, t in _flat(ref))


def test_evaluate_loop_runs_one_batch(gpu_device):
    from spe.engine import evaluate_rtdetr
    from spe.rtdetr import RTDETRPostProcessor, build_rtdetr_criterion
    from spe.solver import SimplePoseSolverSigma
    r = reference_run()
    g, cfg = r["g"], r["cfg"]
    images, clip = torch.from_numpy(r["batch"]["images"]), torch.from_numpy(g["clip_bbox"]).float()
    names = ["img000000.jpg", "img000001.jpg"]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.1 * i, -0.2, 8.0 + i]} for i, n in enumerate(names)}
    rng = np.random.default_rng(0)
    tg = [{"filename": names[b], "clip_bbox": clip[b], "labels": torch.arange(11),
           "landmarks": torch.from_numpy(rng.uniform(0.1, 0.9, (11, 2)).astype(np.float32))} for b in range(2)]
    stats, ev = evaluate_rtdetr(_model("fp32"), build_rtdetr_criterion(cfg), {"bbox": RTDETRPostProcessor()},
                                [(images, tg)], gt, SimplePoseSolverSigma(), gpu_device)
    assert {"loss", "class_error", "loss_ce", "loss_bbox", "speed_eval_pose"} <= set(stats) and list(ev.log) == names
    assert np.isfinite(stats["loss"])
    for n in names:
        assert {"points", "logits", "quat_pr", "tvec_pr", "score", "sigma"} <= set(ev.log[n])


def test_pose_pipeline_eager_mode_gives_finite_poses(gpu_device):
    """PosePipeline(overlap_backbone=True) over the bf16 model and the sigma solver: two batches, finite poses."""
    import argparse
    from spe.pipeline import PosePipeline
    from spe.solver import build_solver
    dev, B = gpu_device, 2
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    p = PosePipeline(_model("bf16"), solver, B, device=dev, overlap_backbone=True)
    g = torch.Generator().manual_seed(3)
    outs = []
    for k in range(2):
        x, _ = _source("gray", B, 256, 30 + k)
        clip = torch.tensor([[100.0, 80.0, 700.0, 640.0]] * B, device=dev)
        quat = torch.nn.functional.normalize(torch.randn(B, 4, generator=g, dtype=torch.float64), dim=1)
        tvec = torch.tensor([0.0, 0.0, 8.0], dtype=torch.float64) + torch.randn(B, 3, generator=g, dtype=torch.float64)
        p.load(x.to(dev), clip, quat.to(dev), tvec.to(dev))
        outs.append(p.run())
    for o in outs:
        p.wait(o)
    torch.cuda.synchronize()
    for o in outs:
        assert torch.isfinite(o["forward"]["points_px"]).all()
        assert torch.isfinite(o["poses"]["quat"]).all() and torch.isfinite(o["poses"]["tvec"]).all()
