"""GPU: the DETR keypoint model with the reference's GroupNorm backbone (`--bn group_bn`, SpeConfig.norm,
SPE_MODEL_GROUP_NORM) against the reference's golden outputs (tools/gen_golden_groupnorm.py).

Tolerances are tests/test_gpu_prenorm.py's / tests/test_gpu_parity.py's:
  fp32 parity modes  pred_points |d| <= 1e-4, pred_logits |d| <= 2e-3, hs <= 2e-3, PostProcess px <= 0.05, probs <= 1e-3
  bf16 throughput    finite, pred_points |d| <= 2e-2, logits |d| <= 0.25 (also with fp16 attention operands)
fp32x3 / fp32x6 run the bare convolutions through the same generic launches and are held to the fp32 bounds; fp32h3
is refused at create.
"""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import launch_table
from spe import _lib
from spe.config import SpeConfig
from spe.synthetic import random_weights, synthetic_batch

pytestmark = pytest.mark.gpu

TAGS = ["s8_s128_q11_l1", "s16_s224_q30_l2", "prenorm_s8_s128_q11_l1"]
_models = {}


def _model(cfg, dtype, wseed, attn_dtype=None, aux=False):
    from spe.models import DETR
    key = (cfg, dtype, wseed, attn_dtype, aux)
    if key not in _models:
        m = DETR(cfg, dtype=dtype, attn_dtype=attn_dtype, aux_loss=aux)
        m.load_state_dict(random_weights(cfg, wseed))
        _models[key] = m
    return _models[key]


def _golden(tag):
    g = np.load(os.path.join(GOLDEN, f"model_groupnorm_{tag}.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    assert cfg.norm == "group_bn"
    return g, cfg


def _run(tag, dtype, dev, attn_dtype=None):
    g, cfg = _golden(tag)
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    m = _model(cfg, dtype, int(g["weight_seed"]), attn_dtype, aux=True)
    o = m(torch.from_numpy(b["images"]).to(dev), clip_bbox=torch.from_numpy(b["clip_bbox"]).float().to(dev),
          return_hs=True)
    torch.cuda.synchronize()
    return g, cfg, o


@pytest.mark.parametrize("dtype", ["fp32", "fp32x3", "fp32x6"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_fp32_matches_reference(gpu_device, tag, dtype):
    g, cfg, o = _run(tag, dtype, gpu_device)
    d = {"points": np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max(),
         "logits": np.abs(o["pred_logits"].cpu().numpy() - g["pred_logits"]).max(),
         "px": np.abs(o["points_px"].cpu().numpy() - g["pp_points"]).max(),
         "probs": np.abs(o["probs"].cpu().numpy() - g["pp_probs"]).max(),
         "hs": np.abs(o["hs"].cpu().numpy() - g["hs"][-1]).max()}
    if cfg.dec_layers > 1:
        d["aux_points"] = max(np.abs(a["pred_points"].cpu().numpy() - g["aux_points"][i]).max()
                              for i, a in enumerate(o["aux_outputs"]))
        d["aux_logits"] = max(np.abs(a["pred_logits"].cpu().numpy() - g["aux_logits"][i]).max()
                              for i, a in enumerate(o["aux_outputs"]))
    print(f"groupnorm {tag} {dtype}: " + " ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert d["points"] <= 1e-4
    assert d["logits"] <= 2e-3
    assert d["px"] <= 0.05
    assert d["probs"] <= 1e-3
    assert d["hs"] <= 2e-3
    assert d.get("aux_points", 0.0) <= 1e-4 and d.get("aux_logits", 0.0) <= 2e-3


@pytest.mark.parametrize("attn_dtype", [None, "fp16"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_bf16_close_to_reference(gpu_device, tag, attn_dtype):
    g, cfg, o = _run(tag, "bf16", gpu_device, attn_dtype)
    for k in ("pred_points", "pred_logits", "points_px", "probs", "hs"):
        assert np.isfinite(o[k].cpu().numpy()).all(), k
    dp = np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max()
    dl = np.abs(o["pred_logits"].cpu().numpy() - g["pred_logits"]).max()
    ap = al = 0.0
    for i, a in enumerate(o.get("aux_outputs", [])):
        ap = max(ap, np.abs(a["pred_points"].cpu().numpy() - g["aux_points"][i]).max())
        al = max(al, np.abs(a["pred_logits"].cpu().numpy() - g["aux_logits"][i]).max())
    print(f"groupnorm {tag} bf16 attn {attn_dtype}: points {dp:.3e} logits {dl:.3e} aux points {ap:.3e} logits {al:.3e}"
          f" (reference arithmetic in bf16: {float(g['emu_bf16_points']):.3e} / {float(g['emu_bf16_logits']):.3e})")
    assert dp <= 2e-2 and ap <= 2e-2
    assert dl <= 0.25 and al <= 0.25


def test_keys_and_loading(gpu_device):
    """param_keys() is the reference's list; a reference-style Namespace goes through build_model ->
    load_state_dict of the 326-key-shaped dict -> forward; the two norms' state dicts do not cross-load."""
    from spe.models import DETR, build_model
    with open(os.path.join(GOLDEN, "model_keys_groupnorm.json")) as f:
        keys = json.load(f)
    for tag in TAGS:
        _, cfg = _golden(tag)
        assert DETR(cfg, dtype="fp32").param_keys() == [k for k, _ in keys[tag]]
    g, cfg = _golden("s8_s128_q11_l1")
    args = argparse.Namespace(bn="group_bn", backbone="resnet50s8", input_size=128, num_queries=11, enc_layers=1,
                              dec_layers=1, dtype="fp32")
    model, _, post = build_model(args)
    assert model.cfg == cfg
    w = random_weights(cfg, int(g["weight_seed"]))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    o = model(torch.from_numpy(b["images"]).to(gpu_device))
    assert np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max() <= 1e-4
    res = post["points"](o, b["clip_bbox"])
    assert np.abs(np.stack([r["points"] for r in res]) - g["pp_points"]).max() <= 0.05
    bn = SpeConfig(**dict(cfg.to_dict(), norm="frozen_bn"))
    with pytest.raises(RuntimeError, match="running_mean"):
        DETR(cfg, dtype="fp32").load_state_dict(random_weights(bn, 1), strict=True)
    with pytest.raises(RuntimeError, match="running_mean"):
        DETR(bn, dtype="fp32").load_state_dict(w, strict=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stages_and_u8_equal_forward(gpu_device, dtype):
    """BACKBONE, then TRANSFORMER, then DECODE in one workspace == forward(), bit for bit; the 8-bit crop entry ==
    the fp32 batch normalised the same way, bit for bit."""
    g, cfg = _golden("s8_s128_q11_l1")
    m = _model(cfg, dtype, int(g["weight_seed"]))
    B, dev = 4, gpu_device
    b = synthetic_batch(cfg, B, 77)
    clip = torch.from_numpy(b["clip_bbox"]).float().to(dev)
    mean = np.array([0.485, 0.456, 0.406], np.float32)
    std = np.array([0.229, 0.224, 0.225], np.float32)
    u = b["crops_u8"].astype(np.float32)[..., None].repeat(3, -1)
    x = torch.from_numpy(np.stack([(u[..., c] / np.float32(255) - mean[c]) / std[c] for c in range(3)], 1)).to(dev)
    ref = m(x, clip_bbox=clip)
    ws = m.new_workspace(B, dev)
    m.encode(x, ws, part="backbone")
    m.encode(None, ws, part="transformer", B=B)
    staged = m.decode(B, ws, clip_bbox=clip)
    u8 = m(torch.from_numpy(b["crops_u8"]).to(dev), clip_bbox=clip)
    torch.cuda.synchronize()
    for k in ("pred_logits", "pred_points", "probs", "points_px"):
        assert torch.equal(staged[k], ref[k]), ("stages", k)
        assert torch.equal(u8[k], ref[k]), ("u8", k)


def test_batch_independence(gpu_device):
    """An image's outputs do not depend on its neighbours in the batch (per-image statistics), in either storage."""
    g, cfg = _golden("s8_s128_q11_l1")
    b = synthetic_batch(cfg, 5, 123)
    img = torch.from_numpy(b["images"]).to(gpu_device)
    for dtype in ("fp32", "bf16"):
        m = _model(cfg, dtype, int(g["weight_seed"]))
        full = m(img)["pred_points"].cpu().numpy()
        part = m(img[2:4].contiguous())["pred_points"].cpu().numpy()
        np.testing.assert_array_equal(full[2:4], part)


def test_pipeline_graph_matches_eager(gpu_device):
    """PosePipeline(use_graph=True): every replay over new inputs equals the eager pipeline."""
    from spe.pipeline import PosePipeline
    from spe.solver import build_solver
    g, cfg = _golden("s8_s128_q11_l1")
    m = _model(cfg, "bf16", int(g["weight_seed"]))
    B, dev = 4, gpu_device
    solver = build_solver(argparse.Namespace(solver="ransac_p3p_lm", repro=20))
    eager = PosePipeline(m, solver, B, device=dev)
    graph = PosePipeline(m, solver, B, device=dev, use_graph=True)
    for k in range(2):
        b = synthetic_batch(cfg, B, 700 + k)
        res = []
        for p in (eager, graph):
            p.load(torch.from_numpy(b["images"]).to(dev), torch.from_numpy(b["clip_bbox"]).float().to(dev))
            o = p.run()
            torch.cuda.synchronize()
            res.append({"logits": o["forward"]["pred_logits"].clone(), "points": o["forward"]["pred_points"].clone(),
                        "status": o["poses"]["status"].clone(), "quat": o["poses"]["quat"].clone(),
                        "tvec": o["poses"]["tvec"].clone()})
        for key in res[0]:
            assert torch.equal(res[0][key], res[1][key]), (k, key)
    assert graph.graph is not None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_bn_model_unchanged(gpu_device, dtype):
    """A frozen-BN model of the same shape, built in the same process next to a GroupNorm one, still meets its own
    existing golden (model_s128_q11_l2) at the parity tests' bounds and takes its fused kinds."""
    g = np.load(os.path.join(GOLDEN, "model_s128_q11_l2.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    assert cfg.norm == "frozen_bn"
    gn = SpeConfig(**dict(cfg.to_dict(), norm="group_bn"))
    mg = _model(gn, dtype, 3)
    m = _model(cfg, dtype, int(g["weight_seed"]))
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    img = torch.from_numpy(b["images"]).to(gpu_device)
    mg(img)
    o = m(img)
    again = m(img)
    torch.cuda.synchronize()
    dp = np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max()
    dl = np.abs(o["pred_logits"].cpu().numpy() - g["pred_logits"]).max()
    print(f"frozen_bn beside group_bn, {dtype}: points {dp:.3e} logits {dl:.3e}")
    assert dp <= (1e-4 if dtype == "fp32" else 2e-2) and dl <= (2e-3 if dtype == "fp32" else 0.25)
    assert torch.equal(o["pred_points"], again["pred_points"])
    kinds = [r[0] for r in launch_table(m, lambda: m(img))]
    assert not any(k.startswith("norm.gn") for k in kinds)


def test_fp32h3_refused(gpu_device):
    """fp32h3 + group_bn fails at create with SPE_E_ARG, before anything is launched."""
    from spe.models import DETR
    with pytest.raises(_lib.SpeError) as e:
        DETR(SpeConfig(input_size=128, enc_layers=1, dec_layers=1, norm="group_bn"), dtype="fp32h3")
    assert "code -1" in str(e.value) and "fp32h3" in str(e.value)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_launch_table(gpu_device, dtype):
    """Stride 8: 43 norm.gn.stats / norm.gn.apply pairs, each behind its conv; one unfused stem conv + max-pool; 43
    body conv launches (no fused conv3 + conv1, no conv3 + downsample GEMM); everything after the backbone is the
    frozen-BN model's sequence."""
    g, cfg = _golden("s8_s128_q11_l1")
    bn_cfg = SpeConfig(**dict(cfg.to_dict(), norm="frozen_bn"))
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    img = torch.from_numpy(b["images"]).to(gpu_device)
    m = _model(cfg, dtype, int(g["weight_seed"]))
    mb = _model(bn_cfg, dtype, 3)
    kinds = [r[0] for r in launch_table(m, lambda: m(img))]
    kinds_bn = [r[0] for r in launch_table(mb, lambda: mb(img))]
    print("groupnorm launch table", dtype, kinds)
    assert kinds.count("norm.gn.apply") == 43 and kinds.count("norm.gn.stats") == 43
    assert not any("stempool" in k or "btail" in k for k in kinds)
    assert kinds[:5] == ["eltwise.pack", "conv.stem", "norm.gn.stats", "norm.gn.apply", "eltwise.maxpool"]
    body = [k for k in kinds if k in ("conv.1x1", "conv.3x3", "conv.1x1s2")]
    assert len(body) == 3 * 13 + 3                      # conv1-3 of 13 blocks + 3 downsample convs, one launch each
    for i, k in enumerate(kinds):
        if k == "norm.gn.stats":
            assert kinds[i - 1].startswith("conv.") and kinds[i + 1] == "norm.gn.apply"
    first_neck = kinds.index("conv.neck")
    assert kinds[first_neck:] == kinds_bn[kinds_bn.index("conv.neck"):]
