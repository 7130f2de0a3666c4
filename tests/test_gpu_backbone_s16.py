"""GPU: the DETR keypoint model behind the plain ResNet-50 stride-16 backbone (`--backbone resnet50`,
REV/models/backbone.py:57-102) against the reference's golden outputs (tools/gen_golden_s16.py).

Tolerances are tests/test_gpu_parity.py's:
  fp32 parity modes  pred_points |d| <= 1e-4, pred_logits |d| <= 2e-3, PostProcess px <= 0.05, probs <= 1e-3
  bf16 throughput    finite, pred_points |d| <= 2e-2, logits |d| <= 0.25 (also with fp16 attention operands)
The goldens: T = 64 tokens (the smallest map), T = 196 (no multiple of 8: the encoder attention's fallback
forms), T = 784 at 448 / Q40 / 3-3 (REV/train_backbone.sh's "resnet50s16" arm).
"""
import json
import os

import numpy as np
import pytest
import torch

import model_s16_ref
from conftest import GOLDEN
from spe.config import SpeConfig
from spe.synthetic import random_weights, synthetic_batch

pytestmark = pytest.mark.gpu

TAGS = ["s128_q11_l2", "s224_q30_l2", "s448_q40_l3"]
_models = {}


def _model(cfg, dtype, wseed, attn_dtype=None):
    from spe.models import DETR
    key = (cfg, dtype, wseed, attn_dtype)
    if key not in _models:
        m = DETR(cfg, dtype=dtype, attn_dtype=attn_dtype)
        m.load_state_dict(random_weights(cfg, wseed))
        _models[key] = m
    return _models[key]


def _golden(tag):
    g = np.load(os.path.join(GOLDEN, f"model_r50s16_{tag}.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    assert cfg.backbone == "resnet50"
    return g, cfg


def _small():
    return SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2, backbone="resnet50")


@pytest.mark.parametrize("dtype", ["fp32", "fp32x3", "fp32x6", "fp32h3"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_fp32_matches_reference(gpu_device, tag, dtype):
    g, cfg = _golden(tag)
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    m = _model(cfg, dtype, int(g["weight_seed"]))
    o = m(torch.from_numpy(b["images"]).to(gpu_device), clip_bbox=torch.from_numpy(b["clip_bbox"]).float().to(gpu_device))
    torch.cuda.synchronize()
    d = {"points": np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max(),
         "logits": np.abs(o["pred_logits"].cpu().numpy() - g["pred_logits"]).max(),
         "px": np.abs(o["points_px"].cpu().numpy() - g["pp_points"]).max(),
         "probs": np.abs(o["probs"].cpu().numpy() - g["pp_probs"]).max()}
    print(f"s16 {tag} {dtype}: " + " ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert d["points"] <= 1e-4
    assert d["logits"] <= 2e-3
    assert d["px"] <= 0.05
    assert d["probs"] <= 1e-3


@pytest.mark.parametrize("attn_dtype", [None, "fp16"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_bf16_close_to_reference(gpu_device, tag, attn_dtype):
    g, cfg = _golden(tag)
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    m = _model(cfg, "bf16", int(g["weight_seed"]), attn_dtype)
    o = m(torch.from_numpy(b["images"]).to(gpu_device), clip_bbox=torch.from_numpy(b["clip_bbox"]).float().to(gpu_device))
    torch.cuda.synchronize()
    for k in ("pred_points", "pred_logits", "points_px", "probs"):
        assert np.isfinite(o[k].cpu().numpy()).all(), k
    dp = np.abs(o["pred_points"].cpu().numpy() - g["pred_points"]).max()
    dl = np.abs(o["pred_logits"].cpu().numpy() - g["pred_logits"]).max()
    print(f"s16 {tag} bf16 attn {attn_dtype}: points {dp:.3e} logits {dl:.3e}")
    assert dp <= 2e-2
    assert dl <= 0.25


_TAIL_CHILD = """
import json, sys
import numpy as np, torch
sys.path[:0] = [%(tests)r, %(pkg)r, %(oracle)r]
from helpers import launch_table
from spe.config import SpeConfig
from spe.models import DETR
from spe.synthetic import random_weights, synthetic_batch
g = np.load(%(golden)r)
cfg = SpeConfig(**json.loads(str(g["config"])))
b = synthetic_batch(cfg, 1, int(g["image_seed"]))
img = torch.from_numpy(b["images"]).cuda().expand(64, -1, -1, -1).contiguous()
m = DETR(cfg, dtype="bf16")
m.load_state_dict(random_weights(cfg, int(g["weight_seed"])))
out = {}
rows = launch_table(m, lambda: out.update(m(img)))
pts, lg = out["pred_points"].cpu().numpy(), out["pred_logits"].cpu().numpy()
print(json.dumps({"launches": len(rows), "conv1x1": sum(r[0] == "conv.1x1" for r in rows),
                  "input_proj": sum(r[0] == "gemm.input_proj" for r in rows),
                  "finite": bool(np.isfinite(pts).all() and np.isfinite(lg).all()),
                  "same_image_equal": bool(np.array_equal(pts[0], pts[63]) and np.array_equal(lg[0], lg[63])),
                  "points": float(np.abs(pts[0] - g["pred_points"][0]).max()),
                  "logits": float(np.abs(lg[0] - g["pred_logits"][0]).max())}))
"""


@pytest.mark.parametrize("knob", ["0", "1"])
def test_forward_bf16_final_tail_knob(gpu_device, knob):
    """SPE_BTAIL_PROJ (read once per process, so each side runs in a child process): at B = 64 and 448^2 the last
    bottleneck has 262 row tiles, and with the knob on the model takes the fused final tail (conv3 + identity +
    relu + input_proj in one launch, no block output stored): one launch fewer, no input_proj GEMM.  Either way
    the first image stays within the bf16 bounds of the golden (its one image), and the same image in another
    row tile gives the same bits."""
    import subprocess
    import sys
    from conftest import ORACLE, PKG
    code = _TAIL_CHILD % {"tests": os.path.dirname(os.path.abspath(__file__)), "pkg": PKG, "oracle": ORACLE,
                          "golden": os.path.join(GOLDEN, "model_r50s16_s448_q40_l3.npz")}
    env = dict(os.environ, SPE_BTAIL_PROJ=knob)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"s16 final tail SPE_BTAIL_PROJ={knob}: {r}")
    assert r["finite"] and r["same_image_equal"]
    assert r["points"] <= 2e-2 and r["logits"] <= 0.25
    assert r["input_proj"] == (0 if knob == "1" else 1)
    _TAIL_LAUNCHES[knob] = r["launches"]
    if len(_TAIL_LAUNCHES) == 2:
        assert _TAIL_LAUNCHES["1"] == _TAIL_LAUNCHES["0"] - 1


_TAIL_LAUNCHES = {}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stages_equal_forward(gpu_device, dtype):
    """BACKBONE, then TRANSFORMER, then DECODE in one workspace == forward(), bit for bit."""
    cfg = _small()
    m = _model(cfg, dtype, 29)
    B = 4
    b = synthetic_batch(cfg, B, 77)
    x = torch.from_numpy(b["images"]).to(gpu_device)
    clip = torch.from_numpy(b["clip_bbox"]).float().to(gpu_device)
    ref = m(x, clip_bbox=clip)
    ws = m.new_workspace(B, gpu_device)
    m.encode(x, ws, part="backbone")
    m.encode(None, ws, part="transformer", B=B)
    out = m.decode(B, ws, clip_bbox=clip)
    torch.cuda.synchronize()
    for k in ("pred_logits", "pred_points", "probs", "points_px"):
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_u8_crops_equal_normalised_batch(gpu_device, dtype):
    """The 8-bit crop entry (grayscale and RGB) == the fp32 batch normalised the same way, bit for bit."""
    cfg = _small()
    m = _model(cfg, dtype, 29)
    b = synthetic_batch(cfg, 6, 77)
    dev = gpu_device
    clip = torch.from_numpy(b["clip_bbox"]).float().to(dev)
    mean = np.array([0.485, 0.456, 0.406], np.float32)
    std = np.array([0.229, 0.224, 0.225], np.float32)
    rgb = np.random.Generator(np.random.PCG64(5)).integers(0, 256, (6, cfg.input_size, cfg.input_size, 3), np.uint8)
    for crops in (b["crops_u8"], rgb):
        u = crops.astype(np.float32)
        if u.ndim == 3:
            u = u[..., None].repeat(3, -1)
        x = np.stack([(u[..., c] / np.float32(255) - mean[c]) / std[c] for c in range(3)], 1)
        ref = m(torch.from_numpy(x).to(dev), clip_bbox=clip)
        got = m(torch.from_numpy(crops).to(dev), clip_bbox=clip)
        torch.cuda.synchronize()
        for k in ("pred_logits", "pred_points", "points_px", "probs"):
            assert torch.equal(got[k], ref[k]), (dtype, crops.ndim, k)


def test_forward_batch_independence(gpu_device):
    cfg = _small()
    m = _model(cfg, "fp32", 29)
    b = synthetic_batch(cfg, 5, 123)
    img = torch.from_numpy(b["images"]).to(gpu_device)
    full = m(img)["pred_points"].cpu().numpy()
    part = m(img[2:4].contiguous())["pred_points"].cpu().numpy()
    np.testing.assert_array_equal(full[2:4], part)


_oracle = {}


def _maps_oracle():
    if not _oracle:
        cfg = _small()
        b = synthetic_batch(cfg, 2, 123)
        w = random_weights(cfg, 29)
        with torch.no_grad():
            o32 = model_s16_ref.forward(b["images"], w, cfg, return_maps=True)
            o64 = model_s16_ref.forward(b["images"], w, cfg, dtype=torch.float64, return_maps=True)
        _oracle.update(enc=(o32["enc_maps"], o64["enc_maps"]), dec=(o32["dec_maps"], o64["dec_maps"]))
    return _oracle


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_with_attention(gpu_device, dtype):
    """Maps [B,64,64] / [B,Q,64] over the (S/16)^2 grid; rows sum to 1 within tests/test_gpu_attention_map.py's
    bounds (1e-5 fp32, 1e-3 bf16); the fp32 model's maps against the restatement's attention weights
    (tests/attention_map_ref.py) within 4 x the fp32-vs-fp64 spread of that restatement, as that file does."""
    cfg = _small()
    m = _model(cfg, dtype, 29)
    b = synthetic_batch(cfg, 2, 123)
    img = torch.from_numpy(b["images"]).to(gpu_device)
    clip = torch.from_numpy(b["clip_bbox"]).float().to(gpu_device)
    ref = m(img, clip_bbox=clip)
    out, mp = m.forward_with_attention(img, enc_layer=-1, dec_layer=-2, clip_bbox=clip)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    T, Q = cfg.tokens, cfg.num_queries
    assert T == 64 and mp["enc"].shape == (2, T, T) and mp["dec"].shape == (2, Q, T)
    ora = _maps_oracle()
    for name, layer in (("enc", -1), ("dec", -2)):
        got = mp[name].cpu()
        assert torch.isfinite(got).all() and (got >= 0).all()
        assert (got.double().sum(-1) - 1).abs().max() <= (1e-5 if dtype == "fp32" else 1e-3)
        o32, o64 = ora[name][0][layer], ora[name][1][layer]
        spread = (o32.double() - o64).abs().max().item()
        err = (got.double() - o64).abs().max().item()
        print(f"s16 attn map {dtype} {name}: error vs fp64 restatement {err:.3e}, restatement spread {spread:.3e}")
        if dtype == "fp32":
            assert err <= 4 * spread
    from spe.attention_maps import decoder_heatmaps
    assert decoder_heatmaps(mp["dec"], cfg.feat_size).shape == (2, Q, 8, 8)


def test_state_dicts_do_not_cross_load(gpu_device):
    from spe.models import DETR
    s16 = _small()
    s8 = SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2)
    w16, w8 = random_weights(s16, 1), random_weights(s8, 1)
    with pytest.raises(Exception):
        DETR(s16, dtype="fp32").load_state_dict(w8, strict=True)
    with pytest.raises(Exception):
        DETR(s8, dtype="fp32").load_state_dict(w16, strict=True)
    assert DETR(s16, dtype="fp32").param_keys() == list(w16)
