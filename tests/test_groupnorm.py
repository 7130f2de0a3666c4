"""CPU: the GroupNorm backbone (`--bn group_bn`, SpeConfig.norm, SPE_MODEL_GROUP_NORM) on the host side -- the key
lists against the reference's, the config switch, cross-loading refusals, that a frozen_bn config's seeded weights
did not move, the restatement (tests/model_groupnorm_ref.py) against the reference's goldens
(tools/gen_golden_groupnorm.py), the create-time refusals, and the kernel contract's restatement
(tests/groupnorm_ref.py) against F.group_norm."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupnorm_ref as gr
import model_groupnorm_ref
from conftest import GOLDEN
from spe import _lib
from spe.config import SpeConfig
from spe.synthetic import param_shapes, random_weights, synthetic_batch, weights_checksum

TAGS = ["s8_s128_q11_l1", "s16_s224_q30_l2", "prenorm_s8_s128_q11_l1"]


def _golden(tag):
    g = np.load(os.path.join(GOLDEN, f"model_groupnorm_{tag}.npz"))
    return g, SpeConfig(**json.loads(str(g["config"])))


@pytest.mark.parametrize("tag", TAGS)
def test_key_list(tag):
    """The reference's group_bn key list == param_shapes(cfg), in order: the frozen_bn list of the same shape without
    its running statistics."""
    _, cfg = _golden(tag)
    assert cfg.norm == "group_bn"
    with open(os.path.join(GOLDEN, "model_keys_groupnorm.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)[tag]]
    ours = param_shapes(cfg)
    assert ours == ref
    bn = param_shapes(SpeConfig(**dict(cfg.to_dict(), norm="frozen_bn")))
    assert len(bn) == len(ours) + 86
    assert [kv for kv in bn if "running_" not in kv[0]] == ours
    assert list(random_weights(cfg, 3)) == [k for k, _ in ours]


def test_key_counts_full_depth():
    assert len(param_shapes(SpeConfig(norm="group_bn"))) == 326
    assert len(param_shapes(SpeConfig(norm="group_bn", backbone="resnet50"))) == 322
    assert len(param_shapes(SpeConfig())) == 412 and len(param_shapes(SpeConfig(backbone="resnet50"))) == 408


def test_c_abi_keys():
    """spe_model_create_flags(SPE_MODEL_GROUP_NORM): the reference's key order for both backbones, alone and with
    SPE_MODEL_PRE_NORM; a larger workspace than the frozen-BN model's (the partial statistics), whose own is unchanged
    by the flag's existence.  (No GPU: create only registers the spec.)"""
    L = _lib.lib()
    base = SpeConfig(input_size=128, enc_layers=1, dec_layers=1)
    c = _lib.ModelConfig(base.input_size, base.num_queries, base.enc_layers, base.dec_layers, base.hidden_dim,
                         base.nheads, base.dim_feedforward, 0, _lib.SPE_DTYPE_F32, 0)
    for bb, name in ((_lib.SPE_BACKBONE_RESNET50_S8, "resnet50s8"), (_lib.SPE_BACKBONE_RESNET50_S16, "resnet50")):
        for pre in (False, True):
            h, h0 = ctypes.c_void_p(), ctypes.c_void_p()
            flags = _lib.SPE_MODEL_GROUP_NORM | (_lib.SPE_MODEL_PRE_NORM if pre else 0)
            assert L.spe_model_create_flags(ctypes.byref(c), bb, flags, ctypes.byref(h)) == 0
            names = [L.spe_model_param_name(h, i).decode() for i in range(L.spe_model_num_params(h))]
            cfg = SpeConfig(**dict(base.to_dict(), backbone=name, pre_norm=pre, norm="group_bn"))
            assert names == [k for k, _ in param_shapes(cfg)]
            assert L.spe_model_create_flags(ctypes.byref(c), bb, flags & ~_lib.SPE_MODEL_GROUP_NORM, ctypes.byref(h0)) == 0
            assert L.spe_model_num_params(h0) == len(names) + 86
            assert L.spe_model_workspace_bytes(h0, 4) < L.spe_model_workspace_bytes(h, 4)
            L.spe_model_destroy(h)
            L.spe_model_destroy(h0)


def test_fp32h3_and_unknown_flags_refused():
    """fp32h3 + group_norm fails at create with SPE_E_ARG (-1) and a message, with and without pre_norm; a bit that
    is no flag is refused too; fp32x3 / fp32x6 / bf16 are created."""
    L = _lib.lib()
    cfg = SpeConfig(input_size=128, enc_layers=1, dec_layers=1)

    def conf(dt):
        return _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim,
                                cfg.nheads, cfg.dim_feedforward, 0, dt, 0)
    h = ctypes.c_void_p()
    c = conf(_lib.SPE_DTYPE_F32H3)
    for flags in (_lib.SPE_MODEL_GROUP_NORM, _lib.SPE_MODEL_GROUP_NORM | _lib.SPE_MODEL_PRE_NORM):
        assert L.spe_model_create_flags(ctypes.byref(c), 0, flags, ctypes.byref(h)) == -1
        assert b"fp32h3" in L.spe_last_error() and not h.value
    assert L.spe_model_create_flags(ctypes.byref(c), 0, 0, ctypes.byref(h)) == 0     # frozen-BN fp32h3 still served
    L.spe_model_destroy(h)
    for dt in (_lib.SPE_DTYPE_BF16, _lib.SPE_DTYPE_F32, _lib.SPE_DTYPE_F32X3, _lib.SPE_DTYPE_F32X6):
        c = conf(dt)
        assert L.spe_model_create_flags(ctypes.byref(c), 0, _lib.SPE_MODEL_GROUP_NORM, ctypes.byref(h)) == 0
        L.spe_model_destroy(h)
    c = conf(_lib.SPE_DTYPE_F32)
    assert L.spe_model_create_flags(ctypes.byref(c), 0, 2, ctypes.byref(h)) == -1
    assert L.spe_model_create_flags(ctypes.byref(c), 0, _lib.SPE_MODEL_GROUP_NORM | 8, ctypes.byref(h)) == -1


def test_from_args_maps_bn():
    ns = argparse.Namespace
    for name in ("frozen_bn", "bn", "sync_bn"):
        assert SpeConfig.from_args(ns(bn=name)).norm == "frozen_bn"
    assert SpeConfig.from_args(ns(bn="group_bn")).norm == "group_bn"
    assert SpeConfig.from_args(ns()).norm == "frozen_bn" and SpeConfig().norm == "frozen_bn"
    c = SpeConfig.from_args(ns(bn="group_bn", backbone="resnet50", pre_norm=True))
    assert (c.norm, c.backbone, c.pre_norm) == ("group_bn", "resnet50", True)
    with pytest.raises(ValueError):
        SpeConfig.from_args(ns(bn="layer_norm"))
    with pytest.raises(ValueError):
        SpeConfig(norm="bn")


def test_stored_configs_without_norm_still_load():
    """A golden written before SpeConfig.norm has no such key: it rebuilds as a frozen_bn config."""
    g = np.load(os.path.join(GOLDEN, "model_s128_q11_l2.npz"))
    d = json.loads(str(g["config"]))
    assert "norm" not in d
    cfg = SpeConfig(**d)
    assert cfg.norm == "frozen_bn" and SpeConfig(**cfg.to_dict()) == cfg


def test_cross_loading_is_refused():
    """A frozen_bn state dict does not load strictly into a group_bn model (86 unexpected running statistics), nor
    the reverse (86 missing); the error names keys of each kind.  (No GPU: the refusal comes before finalize.)"""
    from spe.models import DETR
    gn = SpeConfig(input_size=128, enc_layers=1, dec_layers=1, norm="group_bn")
    bn = SpeConfig(**dict(gn.to_dict(), norm="frozen_bn"))
    wgn, wbn = random_weights(gn, 1), random_weights(bn, 1)
    assert len(wbn) == len(wgn) + 86
    with pytest.raises(RuntimeError, match=r"unexpected=\['backbone\.0\.body\.bn1\.running_mean'"):
        DETR(gn, dtype="fp32").load_state_dict(wbn, strict=True)
    with pytest.raises(RuntimeError, match=r"missing=\['backbone\.0\.body\.bn1\.running_mean'"):
        DETR(bn, dtype="fp32").load_state_dict(wgn, strict=True)
    m = DETR(gn, dtype="fp32")
    missing, unexpected = m.load_state_dict({k: v for k, v in wbn.items() if "bn1" not in k}, strict=False)
    assert unexpected and all("running_" in k for k in unexpected) and all("bn1" in k for k in missing)


@pytest.mark.parametrize("kw,n,digest", [
    (dict(input_size=128, num_queries=11, enc_layers=3, dec_layers=3), 322, "bcbe8dc6fe07e4be"),
    (dict(input_size=224, num_queries=30, enc_layers=2, dec_layers=2, backbone="resnet50"), 288, "a23b70729300ae9f")])
def test_frozen_bn_weights_unchanged(kw, n, digest):
    """random_weights of a frozen_bn config, bit for bit: the checksums tests/test_prenorm.py recorded from the code
    before either option existed; and a group_bn config of the same shape shares no running statistic with it."""
    w = random_weights(SpeConfig(**kw), 7)
    assert len(w) == n and weights_checksum(w) == digest
    assert weights_checksum(random_weights(SpeConfig(norm="frozen_bn", **kw), 7)) == digest
    wg = random_weights(SpeConfig(norm="group_bn", **kw), 7)
    assert len(wg) == n - 86 and not any("running_" in k for k in wg)
    # (gamma like the BN affine: bn3 damped, every gain in [0.125, 1])
    g3 = wg["backbone.0.body.layer1.0.bn3.weight"]
    assert g3.min() >= 0.125 and g3.max() <= 0.25 and wg["backbone.0.body.bn1.weight"].max() <= 1.0


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference(tag):
    """The fp32 restatement == the reference's own model code within 1e-5 on every output; the stored seed rules hold."""
    g, cfg = _golden(tag)
    assert float(g["cond_points_f64_vs_f32"]) <= 2e-5
    assert float(g["emu_bf16_points"]) <= 1e-2 and float(g["emu_bf16_logits"]) <= 0.125
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    with torch.no_grad():
        o = model_groupnorm_ref.forward(b["images"], random_weights(cfg, int(g["weight_seed"])), cfg)
    d = {k: float(np.abs(o[k].numpy() - g[k]).max(initial=0.0))
         for k in ("pred_points", "pred_logits", "hs", "aux_points", "aux_logits")}
    print(f"groupnorm restatement {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert max(d.values()) <= 1e-5


# ---- the kernel contract's restatement

@pytest.mark.parametrize("shape", [(2, 5, 5, 64), (2, 13, 7, 1024), (2, 13, 7, 256), (1, 104, 104, 64)])
def test_welford_merge_is_group_norm(shape):
    """Per-tile (count, mean, M2) triples merged with Chan's update == F.group_norm's statistics in fp64, through
    ragged last tiles and more than one tile per group; the contract == F.group_norm + residual + ReLU."""
    rng = np.random.default_rng(sum(shape))
    B, H, W, C = shape
    x = rng.normal(0.3, 1.7, shape)
    gamma, beta, res = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.2, C), rng.normal(0, 1, shape)
    mean, var = gr.stats(x)
    wm, wv = gr.welford_tiles(x)
    assert np.abs(wm - mean).max() <= 1e-13 and np.abs(wv / var - 1).max() <= 1e-12
    if shape[1] == 104:
        assert gr.tiles(H, W, C) > 1
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    ref = F.group_norm(t, 32, torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5).permute(0, 2, 3, 1).numpy()
    assert np.abs(gr.group_norm(x, gamma, beta) - ref).max() <= 1e-12
    assert np.abs(gr.group_norm(x, gamma, beta, res, True) - np.maximum(ref + res, 0)).max() <= 1e-12


def test_one_pass_variance_loses_the_conditioning_case():
    """x = 100 + N(0, 1): the fp32 one-pass variance misses the normalised output by more than 1e-4; an fp32 Welford
    merge does not."""
    rng = np.random.default_rng(5)
    x = (100.0 + rng.normal(0, 1, (1, 26, 26, 256))).astype(np.float32)
    gamma, beta = np.ones(256), np.zeros(256)
    ref = gr.group_norm(x, gamma, beta)
    m1, v1 = gr.one_pass_f32(x)
    bad = gr._finish(x, m1, np.maximum(v1, 0), gamma, beta, None, False, np.float64)
    wm, wv = gr.welford_tiles(x, np.float32)
    good = gr._finish(x, wm, wv, gamma, beta, None, False, np.float64)
    assert np.abs(bad - ref).max() > 1e-4
    assert np.abs(good - ref).max() <= 1e-4


def test_bf16_emulation_rounds_once():
    rng = np.random.default_rng(9)
    x = gr.to_bf16(rng.normal(0, 2, (2, 5, 5, 64)))
    gamma, beta = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(0, 0.2, 64).astype(np.float32)
    y = gr.group_norm_bf16(x, gamma, beta, relu=True)
    assert np.array_equal(gr.to_bf16(y), y) and y.min() >= 0
    ref = gr.group_norm(x, gamma, beta, relu=True)
    assert np.abs(gr.bf16_bits(y) - gr.bf16_bits(gr.to_bf16(ref))).max() <= 1
