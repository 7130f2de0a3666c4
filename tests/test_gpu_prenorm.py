"""GPU: the DETR keypoint model with the reference's pre-norm transformer (`--pre_norm`, SpeConfig.pre_norm,
SPE_MODEL_PRE_NORM) against the reference's golden outputs (tools/gen_golden_prenorm.py).

Tolerances are tests/test_gpu_parity.py's:
  fp32 parity modes  pred_points |d| <= 1e-4, pred_logits |d| <= 2e-3, PostProcess px <= 0.05, probs <= 1e-3
  bf16 throughput    finite, pred_points |d| <= 2e-2, logits |d| <= 0.25 (also with fp16 attention operands)
fp32x6 is served through the same generic launches as fp32x3 and held to the fp32 bounds; fp32h3 is refused.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import model_prenorm_ref
from conftest import GOLDEN
from helpers import launch_table
from spe import _lib
from spe.config import SpeConfig
from spe.synthetic import random_weights, synthetic_batch

pytestmark = pytest.mark.gpu

TAGS = ["s8_s128_q11_l1", "s8_s128_q11_l3", "s16_s224_q30_l2"]
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
    g = np.load(os.path.join(GOLDEN, f"model_prenorm_{tag}.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    assert cfg.pre_norm
    return g, cfg


def _small(backbone="resnet50s8"):
    return SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2, backbone=backbone, pre_norm=True)


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
    print(f"prenorm {tag} {dtype}: " + " ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert d["points"] <= 1e-4
    assert d["logits"] <= 2e-3
    assert d["px"] <= 0.05
    assert d["probs"] <= 1e-3
    assert d["hs"] <= 2e-3                      # (hs feeds cls_embed, |W| rows sum to O(1): the logits' bound)
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
    print(f"prenorm {tag} bf16 attn {attn_dtype}: points {dp:.3e} logits {dl:.3e} aux points {ap:.3e} logits {al:.3e}"
          f" (reference arithmetic in bf16: {float(g['emu_bf16_points']):.3e} / {float(g['emu_bf16_logits']):.3e})")
    assert dp <= 2e-2 and ap <= 2e-2
    assert dl <= 0.25 and al <= 0.25


def test_keys_and_loading(gpu_device):
    from spe.models import DETR
    with open(os.path.join(GOLDEN, "model_keys_prenorm.json")) as f:
        keys = json.load(f)
    for tag in TAGS:
        _, cfg = _golden(tag)
        assert DETR(cfg, dtype="fp32").param_keys() == [k for k, _ in keys[tag]]
    pre = _small()
    post = SpeConfig(**dict(pre.to_dict(), pre_norm=False))
    wpre, wpost = random_weights(pre, 1), random_weights(post, 1)
    assert len(wpre) == len(wpost) + 2
    with pytest.raises(Exception):
        DETR(pre, dtype="fp32").load_state_dict(wpost, strict=True)
    with pytest.raises(Exception):
        DETR(post, dtype="fp32").load_state_dict(wpre, strict=True)


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
    """The 8-bit crop entry == the fp32 batch normalised the same way, bit for bit."""
    cfg = _small()
    m = _model(cfg, dtype, 29)
    b = synthetic_batch(cfg, 6, 77)
    dev = gpu_device
    clip = torch.from_numpy(b["clip_bbox"]).float().to(dev)
    mean = np.array([0.485, 0.456, 0.406], np.float32)
    std = np.array([0.229, 0.224, 0.225], np.float32)
    u = b["crops_u8"].astype(np.float32)[..., None].repeat(3, -1)
    x = np.stack([(u[..., c] / np.float32(255) - mean[c]) / std[c] for c in range(3)], 1)
    ref = m(torch.from_numpy(x).to(dev), clip_bbox=clip)
    got = m(torch.from_numpy(b["crops_u8"]).to(dev), clip_bbox=clip)
    torch.cuda.synchronize()
    for k in ("pred_logits", "pred_points", "points_px", "probs"):
        assert torch.equal(got[k], ref[k]), (dtype, k)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_batch_independence(gpu_device, dtype):
    cfg = _small()
    m = _model(cfg, dtype, 29)
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
            o32 = model_prenorm_ref.forward(b["images"], w, cfg, return_maps=True)
            o64 = model_prenorm_ref.forward(b["images"], w, cfg, dtype=torch.float64, return_maps=True)
        _oracle.update(enc=(o32["enc_maps"], o64["enc_maps"]), dec=(o32["dec_maps"], o64["dec_maps"]))
    return _oracle


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_with_attention(gpu_device, dtype):
    """Rows sum to 1 (1e-5 fp32, 1e-3 bf16); the fp32 model's maps against the restatement's attention weights
    within 4 x the restatement's own fp32-vs-fp64 spread; the outputs are forward()'s bit for bit."""
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
    assert mp["enc"].shape == (2, T, T) and mp["dec"].shape == (2, Q, T)
    ora = _maps_oracle()
    for name, layer in (("enc", -1), ("dec", -2)):
        got = mp[name].cpu()
        assert torch.isfinite(got).all() and (got >= 0).all()
        assert (got.double().sum(-1) - 1).abs().max() <= (1e-5 if dtype == "fp32" else 1e-3)
        o32, o64 = ora[name][0][layer], ora[name][1][layer]
        spread = (o32.double() - o64).abs().max().item()
        err = (got.double() - o64).abs().max().item()
        print(f"prenorm attn map {dtype} {name}: error vs fp64 restatement {err:.3e}, restatement spread {spread:.3e}")
        if dtype == "fp32":
            assert err <= 4 * spread


def test_fp32h3_refused(gpu_device):
    """fp32h3 + pre-norm fails at create with SPE_E_ARG, before anything is launched."""
    from spe.models import DETR
    with pytest.raises(_lib.SpeError) as e:
        DETR(_small(), dtype="fp32h3")
    assert "code -1" in str(e.value) and "fp32h3" in str(e.value)


ENC_KINDS = ["gemm.enc.qk", "gemm.enc.v", "attn.enc", "gemm.enc.o", "ffn.enc"]


def test_launch_table_bf16(gpu_device):
    """bf16, s8_s128_q11_l3: per encoder layer the pre-norm model launches the post-norm model's kinds, and over
    the whole encoder at most one ln.enc more."""
    g, cfg = _golden("s8_s128_q11_l3")
    post_cfg = SpeConfig(**dict(cfg.to_dict(), pre_norm=False))
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    img = torch.from_numpy(b["images"]).to(gpu_device)
    tables = {}
    for name, c in (("pre", cfg), ("post", post_cfg)):
        m = _model(c, "bf16", int(g["weight_seed"]))
        rows = launch_table(m, lambda: m(img))
        tables[name] = [r[0] for r in rows if r[0].split(".")[1:2] == ["enc"]]
    print("prenorm launch table: pre", tables["pre"], "post", tables["post"])
    assert tables["post"] == ENC_KINDS * cfg.enc_layers
    assert tables["pre"] == ["ln.enc"] + ENC_KINDS * cfg.enc_layers
