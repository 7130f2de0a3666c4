"""Shared seeded cases for parity tests (SURVEY.md §8(d) solver stress set)."""
import numpy as np

from spe.config import world_points, project


def solver_stress_set(B, seed=0, Q=11, C=12, noise=2.0, outlier_frac=0.1, degenerate_frac=0.05, world=None):
    """Per image: labels a random permutation of 0..10 (+ duplicates / no-object queries), points
    = GT projection + N(0, noise px) + uniform outliers, a few images with <=3 or 0 foreground
    labels.  `world`: the C - 1 landmarks (default: the 11 real ones, C = 12).  Returns points [B,Q,2] f32
    px, probs [B,Q,C] f32, q [B,4], t [B,3], sigmas [B,Q,2]."""
    rng = np.random.default_rng(seed)
    W = world_points() if world is None else np.asarray(world, np.float64)
    pts = np.zeros((B, Q, 2), np.float32)
    probs = np.zeros((B, Q, C), np.float32)
    qs, ts = np.zeros((B, 4)), np.zeros((B, 3))
    sig = rng.uniform(0.5, 20.0, (B, Q, 2)).astype(np.float32)
    for b in range(B):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        t = np.array([rng.normal(0, .3), rng.normal(0, .3), rng.uniform(3, 30)])
        qs[b], ts[b] = q, t
        lm = project(W, q, t)
        labels = rng.permutation(Q) % (C - 1)
        r = rng.random()
        if r < degenerate_frac / 2:
            labels[:] = C - 1                             # no foreground
        elif r < degenerate_frac:
            keep = rng.integers(1, 4)                      # 1..3 foreground labels
            labels[keep:] = C - 1
        else:
            ndup = rng.integers(0, 3)
            for _ in range(ndup):                          # duplicated labels / dropped queries
                labels[rng.integers(Q)] = rng.integers(C)
        logits = rng.normal(0, 1, (Q, C)).astype(np.float32)
        logits[np.arange(Q), labels] += rng.uniform(3, 6, Q).astype(np.float32)
        e = np.exp(logits - logits.max(1, keepdims=True))
        probs[b] = e / e.sum(1, keepdims=True)
        p = lm[np.minimum(labels, C - 2)] + rng.normal(0, noise, (Q, 2))
        nout = rng.binomial(Q, outlier_frac)
        if nout:
            idx = rng.choice(Q, nout, replace=False)
            p[idx] += rng.uniform(-400, 400, (nout, 2))
        pts[b] = p.astype(np.float32)
    return pts, probs, qs, ts, sig


# ---- launch tables (tests/test_gpu_launch_table.py, scripts/gen_golden_launch_tables.py)
def launch_table(model, call):
    """Run `call()` with `model`'s per-launch profiler on (spe_model_profile_*): the launches it made,
    in issue order, as [[kind, flops, bytes], ...]."""
    import ctypes

    import torch

    from spe import _lib
    L = _lib.lib()
    _lib.check(L.spe_model_profile_begin(model._h, b""), "spe_model_profile_begin")
    try:
        call()
        torch.cuda.synchronize()
    finally:
        n = L.spe_model_profile_end(model._h)
    rows = []
    kb = ctypes.create_string_buffer(64)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(n):
        _lib.check(L.spe_model_profile_get(model._h, i, kb, 64, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                   "spe_model_profile_get")
        rows.append([kb.value.decode(), fl.value, by.value])
    return rows


# DETR cases: goldens whose configs the parity tests run in every mode (Q = 11: the xattn, xtail and
# fp32h3-xattn branches; Q = 30: the projected-K/V branch in fp32h3), crossed with every numeric mode
LAUNCH_TABLE_TAGS = ["s128_q11_l2", "s224_q30_l4"]
LAUNCH_TABLE_MODES = {"bf16": ("bf16", None), "bf16_attn_fp16": ("bf16", "fp16"), "fp32": ("fp32", None),
                      "fp32x3": ("fp32x3", None), "fp32x6": ("fp32x6", None), "fp32h3": ("fp32h3", None)}
# s128_q11_l2 in bf16 and fp32h3, also: encode then decode as two calls (their tables concatenated), the
# 8-bit crop entry, and a call that fills the aux outputs
LAUNCH_TABLE_VARIANTS = ["split", "u8", "aux"]
# the stride-16, pre-norm and GroupNorm models, "<golden>-<mode>[-<variant>]": the smallest configs that reach each
# of their branches (Q = 30: the projected-K/V cross-attention; l3 with aux: the pre-norm decoder's aux-head call)
LAUNCH_TABLE_MODEL_VARIANTS = [
    "prenorm_s8_s128_q11_l1-bf16", "prenorm_s8_s128_q11_l1-fp32",
    "prenorm_s16_s224_q30_l2-bf16", "prenorm_s16_s224_q30_l2-fp32",
    "prenorm_s8_s128_q11_l3-bf16", "prenorm_s8_s128_q11_l3-bf16-aux",
    "groupnorm_s8_s128_q11_l1-bf16", "groupnorm_s8_s128_q11_l1-fp32",
    "groupnorm_s16_s224_q30_l2-bf16",
    "groupnorm_prenorm_s8_s128_q11_l1-bf16",
    "r50s16_s128_q11_l2-bf16", "r50s16_s128_q11_l2-fp32", "r50s16_s128_q11_l2-fp32h3"]
# RT-DETR cases, "<golden>-<dtype>": BasicBlock and BottleNeck PResNet, then the three light backbones (the
# MobileNetV3_Small case takes the default fused entry)
LAUNCH_TABLE_RTDETR = ["rtdetr_r18_s128-fp32", "rtdetr_r50_s256-bf16", "rtdetr_mbv3l_s256-fp32", "rtdetr_mbv3s_s256-bf16",
                       "rtdetr_ghostv2_s256-fp32"]


def launch_table_cases():
    """Case names of tests/golden/launch_tables.json."""
    names = [f"{t}-{m}" for t in LAUNCH_TABLE_TAGS for m in LAUNCH_TABLE_MODES]
    names += [f"s128_q11_l2-{m}-{v}" for m in ("bf16", "fp32h3") for v in LAUNCH_TABLE_VARIANTS]
    return names + LAUNCH_TABLE_RTDETR + LAUNCH_TABLE_MODEL_VARIANTS


_lt_models = {}


def run_launch_table_case(name, dev):
    """The launch table of one case: weights, batch and seeds as the parity tests take them from the golden."""
    import json
    import os

    import torch

    from spe.config import SpeConfig
    from spe.synthetic import random_weights, synthetic_batch
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if name in LAUNCH_TABLE_RTDETR:
        from spe.rtdetr import RTDETR
        from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
        tag, dtype = name.split("-")
        g = np.load(os.path.join(golden, tag + ".npz"))
        cfg = RtdetrConfig(**json.loads(str(g["config"])))
        if name not in _lt_models:
            _lt_models[name] = RTDETR(cfg, dtype)
            _lt_models[name].load_state_dict(random_rtdetr_weights(cfg, int(g["weight_seed"])))
        m = _lt_models[name]
        b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
        img = torch.from_numpy(b["images"]).to(dev)
        clip = torch.from_numpy(g["clip_bbox"]).float().to(dev)
        return launch_table(m, lambda: m(img, clip_bbox=clip))
    tag, mode, variant = (name.split("-") + [None])[:3]
    from spe.models import DETR
    g = np.load(os.path.join(golden, f"model_{tag}.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    dtype, attn_dtype = LAUNCH_TABLE_MODES[mode]
    key = (tag, mode, variant == "aux")
    if key not in _lt_models:
        _lt_models[key] = DETR(cfg, dtype=dtype, aux_loss=variant == "aux", attn_dtype=attn_dtype)
        _lt_models[key].load_state_dict(random_weights(cfg, int(g["weight_seed"])))
    m = _lt_models[key]
    B = int(g["batch"])
    b = synthetic_batch(cfg, B, int(g["image_seed"]))
    img = torch.from_numpy(b["crops_u8"] if variant == "u8" else b["images"]).to(dev)
    clip = torch.from_numpy(b["clip_bbox"]).float().to(dev)
    if variant == "split":
        ws = m.workspace(B, dev)
        return launch_table(m, lambda: m.encode(img, ws)) + launch_table(m, lambda: m.decode(B, ws, clip_bbox=clip))
    if variant == "aux":
        assert cfg.dec_layers > 1
    return launch_table(m, lambda: m(img, clip_bbox=clip))
