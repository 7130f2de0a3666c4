"""The fp64 restatements that tests/test_gpu_rtdetr_kernels.py holds the kernels of csrc/rtdetr.hip against
(tests/rtdetr_kernels_ref.py), tied to the model's own operations without a GPU:

  query_select   the stable descending sort picks what torch.topk picks when no two scores are equal
  head_finish    on the decoder trace of oracle/rtdetr_ref.py for the r18_s128 golden (the last layer's output and
                 the points it refines) the restatement gives the reference's pred_pts / pred_sigmas within 1e-5
                 and pred_logits within 1e-4: tests/test_rtdetr.py's oracle-vs-reference gates (fp32 rounding)
  msdeform       the input generator meets the coverage the GPU test relies on, for every case it runs
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from spe.config import SpeConfig
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
from spe.synthetic import synthetic_batch
import rtdetr_ref
import rtdetr_kernels_ref as kr


def test_stable_sort_selection_is_topk_without_ties():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(4, 700, 5, generator=g)
    score = logits.max(-1).values
    assert all(len(set(r.tolist())) == r.numel() for r in score)          # tie-free
    for Q in (1, 64, 700):
        want = torch.topk(score, Q, dim=1).indices.numpy()
        np.testing.assert_array_equal(kr.select_ref(score.numpy(), Q), want)


def test_level_major_rows_is_a_permutation_per_level():
    """Unequal levels, B = 3: every row is used once, and level l's rows are the block [B * start_l, B * end_l)."""
    lvl_start, B = [0, 20, 26, 29], 3
    rows = kr.level_major_rows(lvl_start, B)
    assert sorted(rows.ravel().tolist()) == list(range(B * 29))
    for s, e in zip(lvl_start[:-1], lvl_start[1:]):
        blk = rows[:, s:e]
        assert blk.min() == B * s and blk.max() == B * e - 1
        np.testing.assert_array_equal(blk[1] - blk[0], e - s)


def test_head_finish_restatement_reproduces_the_golden_heads():
    g = np.load(os.path.join(GOLDEN, "rtdetr_r18_s128.npz"))
    cfg = RtdetrConfig(**json.loads(str(g["config"])))
    w = random_rtdetr_weights(cfg, int(g["weight_seed"]))
    b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
    trace = {}
    rtdetr_ref.forward(b["images"], w, cfg, trace)
    i = cfg.dec_layers - 1
    B, Q = trace["dec_hs"][i].shape[:2]
    t = lambda k: torch.from_numpy(w[k]).double()
    hs = trace["dec_hs"][i].double().reshape(B * Q, -1)

    def hidden(p):                                  # the two 256-wide layers that run as GEMMs before the kernel
        h = F.relu(hs @ t(f"{p}.layers.0.weight").t() + t(f"{p}.layers.0.bias"))
        return F.relu(h @ t(f"{p}.layers.1.weight").t() + t(f"{p}.layers.1.bias"))
    box, sig = f"decoder.dec_bbox_head.{i}", f"decoder.decoder.sigma_embed.{i}"
    o = kr.head_finish_ref(torch.cat([hidden(box), hidden(sig)], 1), t(f"{box}.layers.2.weight"), t(f"{box}.layers.2.bias"),
                           trace["dec_ref"][i].double().reshape(B * Q, 2), 1, Q, hs=hs,
                           cls_w=t(f"decoder.dec_score_head.{i}.weight"), cls_b=t(f"decoder.dec_score_head.{i}.bias"),
                           sig_w2=t(f"{sig}.layers.2.weight"), sig_b2=t(f"{sig}.layers.2.bias"),
                           clip_bbox=torch.from_numpy(g["clip_bbox"]).double())
    err = {k: np.abs(o[n].reshape(B, Q, -1).numpy() - g[k]).max()
           for k, n in (("pred_pts", "points"), ("pred_logits", "logits"), ("pred_sigmas", "log_sigmas"))}
    print({k: "%.3e" % v for k, v in err.items()})
    assert err["pred_pts"] <= 1e-5 and err["pred_sigmas"] <= 1e-5 and err["pred_logits"] <= 1e-4
    pp = rtdetr_ref.postprocess({k: torch.from_numpy(g[k]) for k in ("pred_logits", "pred_pts", "pred_sigmas")}, g["clip_bbox"])
    assert (o["points_px"].reshape(B, Q, 2) - pp["points"]).abs().max().item() <= 1e-5 * float(np.abs(g["clip_bbox"]).max())
    assert (o["probs"].reshape(B, Q, -1) - pp["probs"]).abs().max().item() <= 1e-5
    assert ((o["sigmas"].reshape(B, Q, 2) - pp["sigmas"]).abs() / pp["sigmas"]).max().item() <= 1e-4


@pytest.mark.parametrize("case", kr.MSDEFORM_CASES, ids=lambda c: "%dlv-%dpt" % (len(c[0]), c[1]))
def test_msdeform_inputs_cover_every_corner_class(case):
    share = kr.check_msdeform_coverage(kr.msdeform_inputs(case))
    print({k: "%.3f" % v for k, v in share.items()})


@pytest.mark.parametrize("cls", kr.CLASSES)
def test_msdeform_single_point_placement(cls):
    """One level, one point: the 8 heads' points all land in the class they were placed in."""
    inp = kr.msdeform_inputs(kr.MSDEFORM_SINGLE, classes=[cls])
    share, count = kr.msdeform_coverage(inp)
    assert share[cls] == 1.0, (cls, share)
    if cls == "far":
        assert share["outside"] == 1.0


def test_msdeform_restatement_is_the_models_cross_attention_core():
    """msdeform_ref on the projections rtdetr_ref.ms_deform_attn computes (its own weights of a decoder layer, square
    levels) followed by that layer's output_proj equals ms_deform_attn."""
    cfg = RtdetrConfig(depth=18, input_size=128)
    w = random_rtdetr_weights(cfg, 1)
    p = "decoder.decoder.layers.1.cross_attn"
    t = lambda k: torch.from_numpy(w[k])
    g = torch.Generator().manual_seed(5)
    B, Q, d = 2, 4, cfg.hidden_dim
    L = sum(s * s for s in cfg.level_sizes)
    query, mem = torch.randn(B, Q, d, generator=g), torch.randn(B, L, d, generator=g)
    ref = torch.rand(B, Q, 2, generator=g)
    want = rtdetr_ref.ms_deform_attn(query, ref.unsqueeze(2), mem, w, p, cfg)
    value = F.linear(mem, t(f"{p}.value_proj.weight"), t(f"{p}.value_proj.bias"))
    nl, npt = cfg.num_levels, cfg.num_points
    off = F.linear(query, t(f"{p}.sampling_offsets.weight"), t(f"{p}.sampling_offsets.bias")).reshape(B, Q, 8, nl, npt, 2)
    lg = F.linear(query, t(f"{p}.attention_weights.weight"), t(f"{p}.attention_weights.bias")).reshape(B, Q, 8, nl * npt)
    core = kr.msdeform_ref(value, [(s, s) for s in cfg.level_sizes], ref, off, lg, torch.float32)
    got = F.linear(core, t(f"{p}.output_proj.weight"), t(f"{p}.output_proj.bias"))
    assert (got - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
