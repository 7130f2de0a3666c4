"""The restatements that tests/test_gpu_detr_helpers.py holds the DETR helper kernels against
(tests/detr_helpers_ref.py), tied to torch's own operators and to oracle/model_ref.py without a GPU:

  maxpool3s2   F.max_pool2d(3, 2, 1), exactly (a max picks one of its inputs)
  upsample2x   F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) in fp64, 1e-12
  layernorm    F.layer_norm in fp64, 1e-12
  softmax      torch.softmax in fp64, 1e-12
  normalize_u8 numpy float32 (u / 255 - mean) / std written out per channel, bit for bit, for every byte value
  pack         the layouts: channel order, the zero pad channels, the zero border
  heads        model_ref's cls_embed / point_embed / sigma_embed on its fp32 tensors and model_ref.postprocess: the
               fp64 restatement within 1e-5 of them (fp32 rounding of three 256-wide layers), the restatement run
               in fp32 within 2e-6
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detr_helpers_ref as hr
import model_ref

# the shapes of the GPU tests and a few more
MAPS = [(1, 1, 1, 8), (2, 7, 5, 16), (1, 2, 3, 8), (1, 1, 3, 8), (2, 3, 1, 8), (2, 5, 7, 16), (1, 26, 13, 32), (1, 16, 16, 64)]
_id = lambda c: "x".join(map(str, c))


def _map(case, seed=0):
    return torch.randn(*case, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("case", MAPS, ids=_id)
@pytest.mark.parametrize("negative", [False, True])
def test_maxpool_is_max_pool2d(case, negative):
    x = _map(case)
    if negative:
        x = -1 - x.abs()
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    got = hr.maxpool3s2(x)
    assert got.shape == want.shape and torch.equal(got, want)
    if negative:
        assert (got < 0).all()                                  # a zero pad would win every border window


@pytest.mark.parametrize("case", MAPS, ids=_id)
def test_upsample_is_interpolate_align_corners(case):
    x = _map(case, 1)
    want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    got = hr.upsample2x(x)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12
    B, H, W, C = case
    if H > 1 and W > 1:                                          # and not the other convention
        other = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert (got - other).abs().max().item() > 1e-2


def test_upsample_corners_are_the_input_corners():
    x = _map((2, 5, 7, 16), 2)
    got = hr.upsample2x(x)
    assert torch.equal(got[:, 0, 0], x[:, 0, 0]) and torch.equal(got[:, -1, -1], x[:, -1, -1])
    assert torch.equal(got[:, 0, -1], x[:, 0, -1]) and torch.equal(got[:, -1, 0], x[:, -1, 0])


@pytest.mark.parametrize("M", [1, 5])
def test_layernorm_is_layer_norm(M):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, 256, generator=g, dtype=torch.float64) * 3 + 1
    x[0] = 1e3 + 0.1 * torch.randn(256, generator=g, dtype=torch.float64)
    gam, bet = torch.randn(256, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64)
    want = F.layer_norm(x, (256,), gam, bet, 1e-5)
    assert (hr.layernorm(x, gam, bet) - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_softmax_is_torch_softmax():
    lg = torch.randn(7, 12, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 5
    got = hr.softmax(lg)
    assert (got - torch.softmax(lg, -1)).abs().max().item() <= 1e-12
    assert (got.sum(-1) - 1).abs().max().item() <= 1e-12


@pytest.mark.parametrize("channels", [1, 3])
def test_normalize_u8_is_to_tensor_then_normalize(channels):
    """Every byte value in every channel, against the formula written out channel by channel in numpy float32."""
    crops = np.stack([np.roll(np.arange(256, dtype=np.uint8), 7 * c) for c in range(channels)], -1).reshape(1, 16, 16, channels)
    got = hr.normalize_u8(crops)
    assert got.dtype == np.float32 and got.shape == (1, 16, 16, 3)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    for c in range(3):
        u = crops[..., c if channels == 3 else 0].astype(np.float32)
        want = (u / np.float32(255)) - np.float32(mean[c])
        want = want / np.float32(std[c])
        assert want.dtype == np.float32
        np.testing.assert_array_equal(got[..., c].view(np.uint32), want.view(np.uint32))
        assert set(crops[..., c if channels == 3 else 0].ravel().tolist()) == set(range(256))
    # and the same numbers as fp64 arithmetic rounds to, within an fp32 ulp or two of values up to 2.7
    f64 = (crops.astype(np.float64) / 255 - np.array(mean)) / np.array(std)
    assert np.abs(got - f64).max() <= 4e-7


def test_pack_layouts():
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 5, 5, generator=g)
    x3 = hr.nchw_to_nhwc(img)
    assert x3.shape == (2, 5, 5, 3) and x3[1, 2, 4, 1].item() == img[1, 1, 2, 4].item()
    for cpad, dt in ((8, torch.float32), (4, torch.float32), (8, torch.bfloat16)):
        p = hr.pack(x3, cpad, dt)
        assert p.shape == (2, 5, 5, cpad) and p.dtype == dt
        assert torch.equal(p[..., :3], x3.to(dt)) and (p[..., 3:] == 0).all() and not torch.signbit(p[..., 3:]).any()
    q = hr.pack_pad4(x3)
    assert q.shape == (2, 11, 11, 4) and q.dtype == torch.bfloat16
    assert torch.equal(q[:, 3:8, 3:8, :3], x3.to(torch.bfloat16))
    inner = torch.zeros(11, 11, dtype=torch.bool)
    inner[3:8, 3:8] = True
    assert (q[:, ~inner] == 0).all() and (q[..., 3] == 0).all()
    assert q.float().abs().sum().item() == x3.to(torch.bfloat16).float().abs().sum().item()


def _head_weights(g, sigma=True):
    rn = lambda *s: torch.randn(*s, generator=g)
    w = {"cls_w": rn(12, 256) / 16, "cls_b": 0.2 * rn(12)}
    for p in ("pt", "sg") if sigma else ("pt",):
        n = 2 if p == "pt" else 1
        w.update({p + "_w0": rn(256, 256) / 16, p + "_b0": 0.2 * rn(256), p + "_w1": rn(256, 256) / 16, p + "_b1": 0.2 * rn(256),
                  p + "_w2": rn(n, 256) / 16, p + "_b2": 0.2 * rn(n)})
    return w


def test_heads_restatement_is_model_refs_heads_and_postprocess():
    g = torch.Generator().manual_seed(6)
    B, Q = 3, 11
    w = _head_weights(g)
    hs = torch.randn(B, Q, 256, generator=g)
    clip = torch.tensor([[10.0 + 37 * b, 20.0 + 11 * b, 110.0 + 87 * b, 100.0 + 41 * b] for b in range(B)])
    sd = {"cls_embed.weight": w["cls_w"], "cls_embed.bias": w["cls_b"]}
    for p, name in (("pt", "point_embed"), ("sg", "sigma_embed")):
        for i in range(3):
            sd[f"{name}.layers.{i}.weight"], sd[f"{name}.layers.{i}.bias"] = w[f"{p}_w{i}"], w[f"{p}_b{i}"]
    logits = F.linear(hs, sd["cls_embed.weight"], sd["cls_embed.bias"])            # model_ref.forward's three lines
    points = model_ref._mlp3(hs, sd, "point_embed").sigmoid()
    log_sigmas = model_ref._mlp3(hs, sd, "sigma_embed").repeat(1, 1, 2)
    pp = model_ref.postprocess(logits, points, clip.numpy(), log_sigmas)
    want = {"logits": logits, "points": points, "log_sigmas": log_sigmas,
            "probs": torch.from_numpy(np.stack([r["logits"] for r in pp])),
            "points_px": torch.from_numpy(np.stack([r["points"] for r in pp])),
            "sigmas": torch.from_numpy(np.stack([r["sigmas"] for r in pp]))}
    for dtype, tol in ((torch.float64, 1e-5), (torch.float32, 2e-6)):
        o = hr.heads(hs.reshape(B * Q, 256).to(dtype), {k: v.to(dtype) for k, v in w.items()}, Q, clip.to(dtype))
        assert set(o) == set(want)
        for k, ref in want.items():
            ref = ref.reshape(B * Q, -1).double()
            err = (o[k].double() - ref).abs().max().item()
            assert err <= tol * max(1.0, ref.abs().max().item()), (k, dtype, err)
    # without a sigma head and without a crop box those outputs are absent
    o = hr.heads(hs.reshape(B * Q, 256), _head_weights(g, sigma=False), Q)
    assert set(o) == {"logits", "probs", "points"}
    # postprocess alone is the tail of heads
    p = hr.postprocess(logits.reshape(B * Q, 12).double(), points.reshape(B * Q, 2).double(), clip.double(), Q)
    assert (p["probs"] - want["probs"].reshape(B * Q, 12)).abs().max().item() <= 1e-6
    assert (p["points_px"] - want["points_px"].reshape(B * Q, 2)).abs().max().item() <= 1e-5 * clip.max().item()


def test_rescale_takes_each_images_own_box():
    """Q = 11 rows an image: rows 8 .. 11 (one 4-row workgroup of the kernel) straddle images 0 and 1."""
    Q = 11
    pts = torch.full((2 * Q, 2), 0.5, dtype=torch.float64)
    clip = torch.tensor([[0.0, 0.0, 100.0, 50.0], [1000.0, 2000.0, 1200.0, 2400.0]], dtype=torch.float64)
    px = hr.rescale(pts, clip, Q)
    assert torch.equal(px[:Q], torch.tensor([50.0, 25.0], dtype=torch.float64).expand(Q, 2))
    assert torch.equal(px[Q:], torch.tensor([1100.0, 2200.0], dtype=torch.float64).expand(Q, 2))
