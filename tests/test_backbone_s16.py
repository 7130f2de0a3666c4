"""CPU: the DETR keypoint model's second backbone, `--backbone resnet50` (REV/models/backbone.py:57-102:
ResNet-50 cut after layer3, stride 16, no neck; input_proj 1024 -> 256): configuration, key space, the
untouched stride-8 weights, and tests/model_s16_ref.py against the goldens tools/gen_golden_s16.py recorded
from the reference's model code."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import model_s16_ref
from conftest import GOLDEN
from spe.config import SpeConfig
from spe.synthetic import param_shapes, random_weights, synthetic_batch, weights_checksum

TAGS = ["s128_q11_l2", "s224_q30_l2", "s448_q40_l3"]
TOKENS = {"s128_q11_l2": 64, "s224_q30_l2": 196, "s448_q40_l3": 784}


def _golden(tag):
    g = np.load(os.path.join(GOLDEN, f"model_r50s16_{tag}.npz"))
    return g, SpeConfig(**json.loads(str(g["config"])))


def _keys():
    with open(os.path.join(GOLDEN, "model_keys_r50s16.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("layers", [2, 3])
def test_param_shapes_are_the_reference_keys(layers):
    ref = [(k, tuple(s)) for k, s in _keys()[f"l{layers}"]]
    assert len(ref) == {2: 288, 3: 318}[layers]
    cfg = SpeConfig(input_size=128, num_queries=11 if layers == 2 else 40, enc_layers=layers, dec_layers=layers,
                    backbone="resnet50")
    ours = [(k, tuple(s)) for k, s in param_shapes(cfg)]
    ref = [(k, (cfg.num_queries, s[1]) if k == "query_embed.weight" else s) for k, s in ref]
    assert sorted(ours) == sorted(ref)
    names = [k for k, _ in ours]
    assert ("input_proj.weight", (256, 1024, 1, 1)) in ours
    assert not any("latern" in k or "output_conv" in k or ".layer4." in k or ".fc." in k for k in names)


@pytest.mark.parametrize("layers", [2, 3])
def test_library_registry_speaks_the_reference_keys(layers):
    """spe_model_create_backbone(SPE_BACKBONE_RESNET50_S16): the parameter registry (no GPU compute)."""
    from spe import _lib
    L = _lib.lib()
    cfg = SpeConfig(input_size=128, num_queries=11, enc_layers=layers, dec_layers=layers, backbone="resnet50")
    c = _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim, cfg.nheads,
                         cfg.dim_feedforward, 0, _lib.SPE_DTYPE_BF16)
    h = ctypes.c_void_p()
    assert L.spe_model_create_backbone(ctypes.byref(c), _lib.SPE_BACKBONE_RESNET50_S16, ctypes.byref(h)) == 0
    names = [L.spe_model_param_name(h, i).decode() for i in range(L.spe_model_num_params(h))]
    assert names == [k for k, _ in param_shapes(cfg)]
    assert sorted(names) == sorted(k for k, _ in _keys()[f"l{layers}"])
    a = np.zeros(256 * 1024, np.float32)
    assert L.spe_model_set_param(h, b"input_proj.weight", a.ctypes.data_as(ctypes.c_void_p), a.size) == 0
    assert L.spe_model_set_param(h, b"backbone.0.s8_latern.weight", a.ctypes.data_as(ctypes.c_void_p), 256 * 512) == -4
    # no xs8 keep and no neck regions, a quarter of the tokens: a smaller workspace than the stride-8 model's
    h8 = ctypes.c_void_p()
    assert L.spe_model_create(ctypes.byref(c), ctypes.byref(h8)) == 0
    assert 0 < L.spe_model_workspace_bytes(h, 4) < L.spe_model_workspace_bytes(h8, 4)
    assert L.spe_model_num_params(h8) == L.spe_model_num_params(h) + 4
    L.spe_model_destroy(h8)
    L.spe_model_destroy(h)
    assert L.spe_model_create_backbone(ctypes.byref(c), 2, ctypes.byref(h)) == -1


# weights_checksum(random_weights(cfg, seed)) of three stride-8 configurations, recorded from the commit before
# the backbone field existed: every stride-8 golden depends on these bytes
S8_CHECKSUMS = [
    (dict(input_size=128, num_queries=11, enc_layers=2, dec_layers=2), 7, "9176d25db188a5df"),
    (dict(input_size=224, num_queries=30, enc_layers=4, dec_layers=4), 3, "4d34a4a2edc5bed8"),
    (dict(input_size=416, num_queries=11, enc_layers=6, dec_layers=6, sigma_head=True), 19, "2f1a73fef8de1e19"),
]


@pytest.mark.parametrize("kw,seed,digest", S8_CHECKSUMS)
def test_stride8_random_weights_unchanged(kw, seed, digest):
    cfg = SpeConfig(**kw)
    assert cfg.backbone == "resnet50s8"
    assert weights_checksum(random_weights(cfg, seed)) == digest
    assert weights_checksum(random_weights(SpeConfig(backbone="resnet50s8", **kw), seed)) == digest


def test_from_args_follows_build_backbone():
    ns = argparse.Namespace
    assert SpeConfig.from_args(ns(backbone="resnet50")).backbone == "resnet50"
    for name in ("resnet50s8", "resnet101", "anything"):      # build_backbone's else branch: Backbone8s
        assert SpeConfig.from_args(ns(backbone=name)).backbone == "resnet50s8"
    assert SpeConfig.from_args(ns()).backbone == "resnet50s8"
    for name in ("resnet18", "resnet34"):
        with pytest.raises(ValueError, match="num_channels 512"):
            SpeConfig.from_args(ns(backbone=name))
    with pytest.raises(ValueError, match="backbone"):
        SpeConfig(backbone="resnet18")
    with pytest.raises(ValueError, match="backbone"):
        SpeConfig(backbone="resnet101")


def test_old_golden_configs_still_load():
    g = np.load(os.path.join(GOLDEN, "model_s128_q11_l2.npz"))
    d = json.loads(str(g["config"]))
    assert "backbone" not in d
    assert SpeConfig(**d).backbone == "resnet50s8"


@pytest.mark.parametrize("S", [128, 224, 448])
def test_feat_size_and_tokens(S):
    a, b = SpeConfig(input_size=S), SpeConfig(input_size=S, backbone="resnet50")
    assert (a.feat_size, a.tokens) == (S // 8, (S // 8) ** 2)
    assert (b.feat_size, b.tokens) == (S // 16, (S // 16) ** 2)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference(tag):
    """tests/model_s16_ref.py against the reference's own outputs: 2e-6 (the stride-8 restatement sits at
    <= 2e-7 of its goldens; the margin of ten allows for the thread count's summation order)."""
    g, cfg = _golden(tag)
    assert cfg.backbone == "resnet50" and cfg.tokens == TOKENS[tag]
    assert float(g["cond_points_f64_vs_f32"]) <= 2e-5
    w = random_weights(cfg, int(g["weight_seed"]))
    b = synthetic_batch(cfg, int(g["batch"]), int(g["image_seed"]))
    with torch.no_grad():
        o = model_s16_ref.forward(b["images"], w, cfg, return_stages=True)
    dp = np.abs(o["pred_points"].numpy() - g["pred_points"]).max()
    dl = np.abs(o["pred_logits"].numpy() - g["pred_logits"]).max()
    print(f"model_s16_ref {tag}: points {dp:.3e} logits {dl:.3e}")
    assert tuple(o["xs16"].shape) == (int(g["batch"]), 1024, cfg.feat_size, cfg.feat_size)
    assert dp <= 2e-6 and dl <= 2e-6
    assert np.abs(o["aux_points"].numpy() - g["aux_points"]).max() <= 2e-6
