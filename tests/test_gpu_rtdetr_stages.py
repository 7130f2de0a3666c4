"""UNC RT-DETR from 8-bit crops and in stages, GPU side (include/spe.h spe_rtdetr_forward_stages / _u8):

1. the u8 entry (PResNet input pack, MobileNetV3_Large / GhostNetV2 u8 stems of stem_u8.h) gives the bits
   of the fp32 entry fed the batch normalised from the same crops;
2. encode + decode over a fresh workspace, and backbone + transformer + decode, give the bits of forward;
3. two batches interleaved stage by stage over two workspaces on one stream give the bits of their own
   unsplit forwards (nothing writable is shared outside the workspaces);
4. PosePipeline runs an RT-DETR in every eager mode with the plain mode's bits, sigmas reaching the solver;
5. generate_submission with one MobileNetV3_Large RT-DETR equals the loop done by hand.

No tolerance anywhere: the same arithmetic in the same order, compared with torch.equal.  The fp32 batch is
built on the device as ((u8.float() / 255 - mean) / std) with the divisors as device TENSORS: torch turns a
division by a Python scalar into a multiplication by its reciprocal, which is not the to_tensor + Normalize
arithmetic (IEEE division) the u8 path restates.
"""
import argparse
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

from spe import _lib
from spe.rtdetr import RTDETR
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights

pytestmark = pytest.mark.gpu

CFGS = {"r18": RtdetrConfig(depth=18, input_size=128), "r50": RtdetrConfig(depth=50, input_size=128),
        "mobilenetv3_large": RtdetrConfig(backbone="mobilenetv3_large", input_size=256),
        "ghostnetv2": RtdetrConfig(backbone="ghostnetv2", input_size=256)}


@functools.lru_cache(maxsize=None)
def _weights(name):
    return random_rtdetr_weights(CFGS[name], 0)


@functools.lru_cache(maxsize=None)
def _model(name, dtype):
    m = RTDETR(CFGS[name], dtype=dtype)
    m.load_state_dict(_weights(name))
    return m


def _crops(B, S, ch, seed, dev):
    """Random 8-bit crops with the border rows / columns forced to 0 and 255: the padded taps of the stems
    and both extreme values are hit."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 256, (B, S, S) + ((3,) if ch == 3 else ()), dtype=torch.uint8, generator=g)
    c[:, 0], c[:, -1] = 0, 255
    c[:, :, 0], c[:, :, -1] = 255, 0
    return c.to(dev)


def _normalised(crops):
    dev = crops.device
    u = crops.float()
    if u.dim() == 3:
        u = u[..., None].expand(-1, -1, -1, 3)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev)
    return ((u / torch.tensor(255.0, device=dev) - mean) / std).permute(0, 3, 1, 2).contiguous()


def _clip(B, dev, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    xy = torch.rand(B, 2, generator=g) * 600
    wh = 200 + torch.rand(B, 1, generator=g) * 500
    return torch.cat([xy, xy + wh], 1).to(dev)


def _flat(o, prefix=""):
    """(name, tensor) of every tensor of a forward's dict, aux_outputs and topk included."""
    for k, v in (o.items() if isinstance(o, dict) else enumerate(o)):
        if torch.is_tensor(v):
            yield f"{prefix}{k}", v
        else:
            yield from _flat(v, f"{prefix}{k}.")


def _assert_same(got, ref, what):
    got, ref = dict(_flat(got)), dict(_flat(ref))
    assert list(got) == list(ref), what
    assert {"pred_logits", "pred_pts", "pred_sigmas", "probs", "points_px", "sigmas", "topk",
            "aux_outputs.0.pred_sigmas"} <= set(got)
    for k in ref:
        assert torch.equal(got[k], ref[k]), (what, k, (got[k].float() - ref[k].float()).abs().max().item())


def test_device_normalisation_is_the_reference_arithmetic(gpu_device):
    """The fp32 batch the comparisons below use is numpy's float32 (u / 255 - mean) / std, bit for bit."""
    c = _crops(2, 64, 3, 5, gpu_device)
    u = c.cpu().numpy().astype(np.float32)
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    x = np.stack([(u[..., k] / np.float32(255) - mean[k]) / std[k] for k in range(3)], 1)
    assert np.array_equal(_normalised(c).cpu().numpy(), x)


@pytest.mark.parametrize("name,dtype", [("r18", "bf16"), ("r18", "fp32"), ("mobilenetv3_large", "bf16"),
                                        ("mobilenetv3_large", "fp32"), ("ghostnetv2", "bf16"), ("ghostnetv2", "fp32"),
                                        ("r50", "bf16")])
def test_u8_crops_equal_normalised_batch(gpu_device, name, dtype):
    m, S = _model(name, dtype), CFGS[name].input_size
    for B in (1, 3):
        clip = _clip(B, gpu_device)
        for ch in (1, 3):
            crops = _crops(B, S, ch, 10 * B + ch, gpu_device)
            ref = m(_normalised(crops), clip_bbox=clip)
            got = m(crops, clip_bbox=clip)
            torch.cuda.synchronize()
            _assert_same(got, ref, (name, dtype, B, ch))
            assert all(torch.isfinite(t).all() for _, t in _flat(ref))


STAGED = [("r18", "bf16"), ("r18", "fp32"), ("mobilenetv3_large", "bf16"), ("ghostnetv2", "bf16")]


@pytest.mark.parametrize("name,dtype", STAGED)
def test_stages_equal_unsplit_forward(gpu_device, name, dtype):
    m, S, B = _model(name, dtype), CFGS[name].input_size, 3
    clip = _clip(B, gpu_device)
    crops = _crops(B, S, 1, 7, gpu_device)
    for x in (_normalised(crops), crops):
        ref = m(x, clip_bbox=clip)
        ws = m.new_workspace(B, gpu_device)
        m.encode(x, ws)
        two = m.decode(B, ws, clip_bbox=clip)
        ws3 = m.new_workspace(B, gpu_device)
        m.encode(x, ws3, part="backbone")
        m.encode(None, ws3, part="transformer", B=B)
        three = m.decode(B, ws3, clip_bbox=clip)
        torch.cuda.synchronize()
        _assert_same(two, ref, (name, dtype, str(x.dtype), "encode + decode"))
        _assert_same(three, ref, (name, dtype, str(x.dtype), "backbone + transformer + decode"))
    # decode's own switches, and the workspace check
    hs = m.decode(B, ws3, clip_bbox=clip, aux=False, return_hs=True)
    torch.cuda.synchronize()
    assert "aux_outputs" not in hs and "topk" not in hs and hs["hs"].shape == (B, CFGS[name].num_queries, 256)
    assert torch.equal(hs["points_px"], ref["points_px"]) and torch.equal(hs["sigmas"], ref["sigmas"])
    with pytest.raises(_lib.SpeError, match="workspace too small"):
        m.encode(crops, ws[:-256])


@pytest.mark.parametrize("name,dtype", [("r18", "bf16"), ("mobilenetv3_large", "bf16"), ("ghostnetv2", "bf16")])
def test_two_batches_in_flight_share_nothing(gpu_device, name, dtype):
    """A.backbone, B.backbone, A.transformer, B.transformer, A.decode, B.decode on ONE stream (deterministic:
    no race is sought): a scratch buffer left outside the workspace would carry B's data into A's later stage."""
    m, S, B = _model(name, dtype), CFGS[name].input_size, 3
    xa, xb = _crops(B, S, 1, 21, gpu_device), _normalised(_crops(B, S, 3, 22, gpu_device))
    ca, cb = _clip(B, gpu_device, 1), _clip(B, gpu_device, 2)
    ra, rb = m(xa, clip_bbox=ca), m(xb, clip_bbox=cb)
    wa, wb = m.new_workspace(B, gpu_device), m.new_workspace(B, gpu_device)
    m.encode(xa, wa, part="backbone")
    m.encode(xb, wb, part="backbone")
    m.encode(None, wa, part="transformer", B=B)
    m.encode(None, wb, part="transformer", B=B)
    oa = m.decode(B, wa, clip_bbox=ca)
    ob = m.decode(B, wb, clip_bbox=cb)
    torch.cuda.synchronize()
    _assert_same(oa, ra, (name, "A"))
    _assert_same(ob, rb, (name, "B"))
    assert not torch.equal(ra["pred_pts"], rb["pred_pts"])


def test_pose_pipeline_runs_an_rtdetr_in_every_eager_mode(gpu_device):
    """r18, S=128, B=4, the sigma solver, 5 run() calls over 2 batches: overlap_decode, overlap_backbone and
    host_input + overlap_backbone (u8 crops from pinned memory) against the plain pipeline on the same batch."""
    from spe.pipeline import PosePipeline
    from spe.solver import build_solver
    dev, B, S = gpu_device, 4, 128
    m = _model("r18", "bf16")
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    crops = [_crops(B, S, 1, 40 + k, dev) for k in range(2)]
    images = [_normalised(c) for c in crops]
    clips = [_clip(B, dev, 10 + k) for k in range(2)]
    g = torch.Generator().manual_seed(3)
    quat = [torch.nn.functional.normalize(torch.randn(B, 4, generator=g, dtype=torch.float64), dim=1) for _ in range(2)]
    tvec = [torch.tensor([0.0, 0.0, 8.0], dtype=torch.float64) + torch.randn(B, 3, generator=g, dtype=torch.float64)
            for _ in range(2)]
    order = [0, 1, 0, 1, 0]

    def run_loaded(**kw):
        p = PosePipeline(m, solver, B, device=dev, **kw)
        outs = []
        for k in order:
            p.load(images[k], clips[k], quat[k].to(dev), tvec[k].to(dev))
            outs.append(p.run())
        for o in outs:
            p.wait(o)
        torch.cuda.synchronize()
        return outs

    def check(outs, ref, what):
        for i, (o, r) in enumerate(zip(outs, ref)):
            _assert_same(o["forward"], r["forward"], (what, i))
            for k in ("status", "quat", "tvec"):
                assert torch.equal(o["poses"][k], r["poses"][k]), (what, i, k)
            assert torch.equal(o["s_t"], r["s_t"]) and torch.equal(o["s_q"], r["s_q"]), (what, i)
            assert set(o["assess"]) == {"mean_sigma", "n_confident", "reliable"}
            assert torch.equal(o["assess"]["mean_sigma"], r["assess"]["mean_sigma"]), (what, i)

    plain = run_loaded()
    check([plain[2], plain[3], plain[4]], [plain[0], plain[1], plain[0]], "plain, repeated batch")
    assert not torch.equal(plain[0]["forward"]["points_px"], plain[1]["forward"]["points_px"])
    check(run_loaded(overlap=True), plain, "overlap")
    check(run_loaded(overlap_decode=True), plain, "overlap_decode")
    check(run_loaded(overlap_backbone=True), plain, "overlap_backbone")
    for kw in (dict(overlap_backbone=True), {}):          # the staged slots, and the one-slot host mode
        host = PosePipeline(m, solver, B, device=dev, host_input=True, **kw)
        host.load_host(torch.cat(crops).cpu(), torch.cat(clips).cpu(), torch.cat(quat), torch.cat(tvec))
        outs = [host.run() for _ in order]
        for o in outs:
            host.wait(o)
        torch.cuda.synchronize()
        check(outs, plain, ("host_input", kw))
        assert host.h2d_bytes == B * S * S + B * 4 * 4 + B * 7 * 8


def _jpeg(a):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", quality=90)
    return bio.getvalue()


def test_generate_submission_with_one_rtdetr(gpu_device):
    """3 synthetic 1920 x 1200 gray JPEG files (one box sticking out of the frame), batch size 2 (a short last
    batch), a MobileNetV3_Large RT-DETR and the sigma solver == SpeedSubmissionTransform -> model ->
    solver.solve_batch by hand on the same crops."""
    from spe.datasets import JpegDecoder, SpeedSubmissionTransform
    from spe.engine import generate_submission
    from spe.solver import EPnPCeresSolver, build_solver
    dev = gpu_device
    m = _model("mobilenetv3_large", "bf16")
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 1200, 1920
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [np.clip(np.rint(100 + 70 * np.sin(xx / (40.0 + 9 * i)) * np.cos(yy / 57.0) + rng.normal(0, 12, (H, W))),
                      0, 255).astype(np.uint8) for i in range(3)]
    names = ["img3.jpg", "img1.jpg", "img2.jpg"]
    files = {n: _jpeg(f) for n, f in zip(names, frames)}
    boxes = [[700.0, 300.0, 1300.0, 900.0], [-60.5, 200.0, 500.0, 850.0], [900.2, 410.9, 1400.4, 700.1]]
    anns = {n: [b + [0.9], [0.0, 0.0, 10.0, 10.0, 0.1]] for n, b in zip(names, boxes)}
    dec = JpegDecoder(H, W, max_bytes=max(map(len, files.values())))
    log = generate_submission(m, None, anns, files.__getitem__, solver, dev, 2, 256, decoder=dec)

    d = dec(*JpegDecoder.pack([files[n] for n in names], dev))
    assert d["status"].cpu().tolist() == [0, 0, 0]
    tr = SpeedSubmissionTransform(256)
    want, clip_x1 = {}, []
    for i in range(0, 3, 2):
        t = tr(d["frames"][i:i + 2].contiguous(), np.asarray(boxes[i:i + 2], np.float64), crops=True, images=False)
        assert t["crops"].dtype == torch.uint8 and t["status"].cpu().tolist() == [0] * len(boxes[i:i + 2])
        clip_x1 += t["clip_bbox"][:, 0].cpu().tolist()
        o = m(t["crops"], clip_bbox=t["clip_bbox"])
        p = solver.solve_batch(o["points_px"], o["probs"], o["sigmas"])
        quat, tvec, status = p["quat"].double().cpu().numpy(), p["tvec"].cpu().numpy(), p["status"].cpu().numpy()
        for j, n in enumerate(names[i:i + 2]):
            ok = status[j] in (0, 3)
            want[n] = {"quat_pr": np.around(quat[j] if ok else np.zeros(4), 6).tolist(),
                       "tvec_pr": np.around(tvec[j] if ok else np.zeros(3), 6).tolist()}
    assert min(clip_x1) < 0                                     # the second box sticks out of the frame
    print("solved poses:", sum(any(r["tvec_pr"]) for r in want.values()), "of", len(want))
    assert list(log) == names and log == want
    with pytest.raises(ValueError, match="EPnPCeresSolver"):
        generate_submission(m, None, anns, files.__getitem__, EPnPCeresSolver(256), dev, 2, 256, decoder=dec)
