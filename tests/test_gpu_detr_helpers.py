"""The DETR stem, neck and head helper kernels one by one, through their hooks (spe_debug_pack_input,
spe_debug_pack_input_pad4, spe_debug_maxpool3s2, spe_debug_upsample2x, spe_debug_heads, spe_debug_layernorm) and
spe_postprocess, against the plain restatements of tests/detr_helpers_ref.py (tied to torch's operators and to
oracle/model_ref.py by tests/test_detr_helpers_ref.py).  Every output buffer is NaN-filled first and allocated with
slack (rows or elements after the last, pad columns of a wider row stride): an unwritten element fails, and what a
kernel must not write must still be NaN afterwards.

Exact (bit for bit): everything pack_input and pack_input_pad4 write (a copy, a bf16 rounding, or the fp32
(u / 255 - mean) / std that numpy float32 gives); the amax slot; maxpool3s2 (a max returns one of the stored inputs);
upsample2x of a spatially constant map whose constants are 0 or +-2^k (the products with the weights are then exact
and hx + lx differs from 1 by at most 2^-25, so a (hx + lx) rounds back to a, with or without FMA contraction);
points_px against torch fp32 `points * (x1 - x0) + x0` as two rounded operations on the kernel's own points
(heads.hip is built without FMA contraction for this); spe_postprocess against the fused kernel on the same
logits and points; layernorm of a constant row (beta).

Gates, relative to max(1, max |ref|), g = 1e-5 for fp32 and 1e-2 for bf16 storage (tests/test_gpu_kernels.py's bf16
gate, which covers the output rounding only):

upsample2x: max(g max(1, max |ref|), 4 x what torch's own fp32 CPU interpolate loses against the fp64 restatement on
the same dtype-rounded input) -- the source coordinate is computed in fp32, so the loss grows with the map's slope
(the rule of tests/test_gpu_rtdetr_kernels.py's msdeform).  Measured on an MI355X (CPU fp32 vs fp64 / kernel vs
fp64 / gate):
  fp32  1x1x1x8     0         / 0         / 3.822e-05      bf16  1x1x1x8     0         / 0         / 3.828e-02
        1x1x3x8     2.623e-07 / 2.623e-07 / 3.823e-05            1x1x3x8     2.384e-07 / 7.813e-03 / 3.828e-02
        2x3x1x8     4.292e-07 / 2.980e-07 / 5.990e-05            2x3x1x8     4.768e-07 / 1.484e-02 / 6.000e-02
        2x5x7x16    1.462e-06 / 5.726e-07 / 6.686e-05            2x5x7x16    1.438e-06 / 1.563e-02 / 6.688e-02
        1x26x13x32  9.272e-06 / 2.333e-06 / 6.980e-05            1x26x13x32  9.302e-06 / 1.562e-02 / 6.969e-02
        2x5x7x4     9.353e-07 / 6.022e-07 / 5.497e-05
so in fp32 the kernel loses no more than torch's own fp32 interpolate and the g term is the gate in every case
(max |ref| 3.8 .. 7.0); in bf16 the error is the output rounding (2^-9 of values up to 7).
The other align_corners convention or swapped axes give errors of order 1.

heads, logits / points / log_sigmas: max(1e-5 max(1, max |ref|), 4 x what the same restatement run in torch fp32 on
the CPU loses against fp64).  Measured on an MI355X (CPU fp32 vs fp64 / kernel vs fp64 / gate):
  (B, Q)   logits                               points                               log_sigmas
  1 x 1    3.085e-07 / 2.297e-07 / 2.102e-05    7.499e-08 / 7.958e-08 / 1.000e-05    2.374e-07 / 3.587e-07 / 1.589e-05
  1 x 5    6.277e-07 / 2.205e-07 / 2.874e-05    6.207e-08 / 1.136e-07 / 1.000e-05    1.189e-07 / 5.228e-07 / 1.000e-05
  3 x 4    8.014e-07 / 2.417e-07 / 3.139e-05    7.626e-08 / 1.114e-07 / 1.000e-05    2.945e-07 / 4.118e-07 / 1.000e-05
  2 x 11   9.648e-07 / 2.612e-07 / 2.643e-05    8.894e-08 / 1.034e-07 / 1.000e-05    2.676e-07 / 5.531e-07 / 1.043e-05
(without the sigma head logits and points are the same numbers): the 1e-5 term is the gate in every case, max |ref|
1.0 .. 3.2.
probs against the fp64 softmax of the kernel's own logits: 1e-6 absolute; sigmas against exp of the kernel's own
log_sigmas: 1e-6 relative; both columns of log_sigmas and of sigmas equal.  spe_postprocess alone: the same 1e-6
(the same code).

layernorm: 1e-5 for the fp32 outputs, 1e-2 for the bf16 one.  The row of mean 1e3 and standard deviation 0.1 (fp32
only: bf16 stores every such value as 1000): max(that, 4 x what torch's fp32 CPU layer_norm loses against fp64); the
fp32 row sum of 256 values near 1000 is only good to about 1e-2, which moves every output by the same 1e-4 / 0.1.
Measured on an MI355X (CPU fp32 vs fp64 / kernel vs fp64 / gate):
  1.600e-03 / 2.263e-03 / 6.398e-03 (max |ref| 5.78)
A one-pass variance (E[x^2] - mean^2 at 1e6) is wrong by orders of magnitude more.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from spe import _lib
import detr_helpers_ref as hr

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32, 1e-5), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16, 1e-2)}
NAN = float("nan")
REFUSED, BAD_SHAPE = -5, -6
SLACK = 64                                                     # elements after the last one a kernel may write


def _p(t):
    return _lib.ptr(t)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _biteq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b.to(a.device)))


def _err(got, ref):
    return (got.double().cpu() - ref.double()).abs().max().item()


_id = lambda v: v if isinstance(v, str) else "x".join(map(str, v))


# ---------------------------------------------------------------- pack_input
# (B, S): one 2 x 2 image / odd sizes / two workgroups / 17 * 256 * 256 = 1 114 112 pixels, more than the fp32
# launcher's 4096 x 256 threads: the smallest batch of 256 x 256 crops that runs the grid-stride loop
PACK_CASES = [(1, 2), (3, 5), (2, 16), (17, 256)]
PACK_OUT = [("fp32", 8), ("fp32", 4), ("bf16", 8)]
assert 16 * 256 * 256 <= 4096 * 256 < 17 * 256 * 256


@functools.lru_cache(maxsize=None)
def _images(B, S):
    """fp32 [B][3][S][S] and the same as NHWC [B][S][S][3]"""
    img = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(B * S)) * 2.0
    return img, hr.nchw_to_nhwc(img)


@functools.lru_cache(maxsize=None)
def _crops(B, S, channels):
    """u8 [B][S][S][channels] and its normalised fp32 [B][S][S][3].  At S = 16 image 0 holds every byte value in
    every channel."""
    c = torch.randint(0, 256, (B, S, S, channels), generator=torch.Generator().manual_seed(B * S + channels), dtype=torch.uint8)
    if S == 16:
        for ch in range(channels):
            c[0, :, :, ch] = torch.roll(torch.arange(256), 7 * ch).reshape(16, 16).to(torch.uint8)
            assert len(set(c[0, :, :, ch].reshape(-1).tolist())) == 256
    return c, torch.from_numpy(hr.normalize_u8(c.numpy()))


def _source(dev, src, B, S):
    """src "f32" / "u8x3" / "u8x1" -> (images on the device or None, crops on the device or None, channels, the
    three channel values as fp32 NHWC on the CPU)"""
    if src == "f32":
        img, x3 = _images(B, S)
        return img.to(dev), None, 0, x3
    crops, x3 = _crops(B, S, int(src[-1]))
    return None, crops.to(dev), int(src[-1]), x3


def _pack(dev, dtype, cpad, B, S, f32, u8, channels, amax=None, want_rc=0):
    code, tdt, _ = DT[dtype]
    n = B * S * S * cpad
    out = _nan((n + SLACK,), dev, tdt)
    rc = _lib.lib().spe_debug_pack_input(None, code, _p(f32), _p(u8), channels, _p(out), B, S, cpad, _p(amax))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    assert torch.isnan(out[n:]).all()
    return out[:n].reshape(B, S, S, cpad)


@pytest.mark.parametrize("case", PACK_CASES, ids=_id)
@pytest.mark.parametrize("out", PACK_OUT, ids=lambda o: "%sx%d" % o)
@pytest.mark.parametrize("src", ["f32", "u8x3", "u8x1"])
def test_pack_input_is_exact(gpu_device, src, out, case):
    """fp32 source: the channel values bit-equal to the source or to its .to(torch.bfloat16).  8-bit source: numpy
    float32 (u / 255 - mean) / std bit for bit, or its bf16 rounding; one gray value feeds all three channels.  The
    pad channels are exactly +0."""
    (dtype, cpad), (B, S) = out, case
    f32, u8, channels, x3 = _source(gpu_device, src, B, S)
    got = _pack(gpu_device, dtype, cpad, B, S, f32, u8, channels)
    assert _biteq(got, hr.pack(x3, cpad, DT[dtype][1]))
    if src == "u8x1":
        assert not _biteq(got[..., 0], got[..., 1]) and not _biteq(got[..., 1], got[..., 2])   # (three normalisations)


def _slot(dev, preset):
    s = _nan((3,), dev)
    s[1] = preset
    return s


@pytest.mark.parametrize("case", [(2, 16, 8), (2, 16, 4), (3, 5, 8), (17, 256, 8)], ids=_id)
@pytest.mark.parametrize("src", ["f32", "u8x3"])
def test_pack_input_amax_slot_is_raised_to_the_maximum(gpu_device, src, case):
    """Slot preset to 0 -> max |x| bit for bit (one workgroup, two, and 4096 that each publish once); its
    neighbours untouched."""
    B, S, cpad = case
    f32, u8, channels, x3 = _source(gpu_device, src, B, S)
    slot = _slot(gpu_device, 0.0)
    got = _pack(gpu_device, "fp32", cpad, B, S, f32, u8, channels, amax=slot[1:])
    assert _biteq(got, hr.pack(x3, cpad))
    want = x3.abs().max()
    assert want.item() > 0 and _biteq(slot[1].cpu(), want)
    assert torch.isnan(slot[0]) and torch.isnan(slot[2])


@pytest.mark.parametrize("src", ["f32", "u8x3"])
def test_pack_input_amax_slot_is_never_lowered(gpu_device, src):
    B, S = 2, 16
    f32, u8, channels, x3 = _source(gpu_device, src, B, S)
    preset = 2.0 * x3.abs().max().item()
    slot = _slot(gpu_device, preset)
    _pack(gpu_device, "fp32", 8, B, S, f32, u8, channels, amax=slot[1:])
    assert _biteq(slot[1].cpu(), torch.tensor(preset))


def test_pack_input_amax_slot_between_two_workgroups_maxima(gpu_device):
    """(2, 16): one workgroup an image.  A slot preset between the two images' maxima ends at the larger one."""
    B, S = 2, 16
    f32, u8, channels, x3 = _source(gpu_device, "f32", B, S)
    m = x3.abs().reshape(B, -1).max(1).values
    assert m[0].item() != m[1].item()
    slot = _slot(gpu_device, 0.5 * (m[0] + m[1]).item())
    _pack(gpu_device, "fp32", 8, B, S, f32, u8, channels, amax=slot[1:])
    assert _biteq(slot[1].cpu(), m.max())


@pytest.mark.parametrize("preset", [0.0, 1e-3])
def test_pack_input_amax_slot_ignores_a_zero_image(gpu_device, preset):
    B, S = 2, 5
    img = torch.zeros(B, 3, S, S, device=gpu_device)
    slot = _slot(gpu_device, preset)
    got = _pack(gpu_device, "fp32", 8, B, S, img, None, 0, amax=slot[1:])
    assert _biteq(got, torch.zeros(B, S, S, 8))
    assert _biteq(slot[1].cpu(), torch.tensor(preset))


def test_pack_input_bf16_leaves_the_amax_slot_alone(gpu_device):
    """The bf16 launch passes no slot to the kernel (the bf16 stem has no activation scale)."""
    B, S = 2, 16
    f32, _, _, x3 = _source(gpu_device, "f32", B, S)
    slot = _slot(gpu_device, 0.0)
    got = _pack(gpu_device, "bf16", 8, B, S, f32, None, 0, amax=slot[1:])
    assert _biteq(got, hr.pack(x3, 8, torch.bfloat16))
    assert _biteq(slot[1].cpu(), torch.tensor(0.0)) and torch.isnan(slot[0]) and torch.isnan(slot[2])


@pytest.mark.parametrize("dtype,cpad", PACK_OUT)
def test_pack_input_refuses_a_missing_or_two_channel_source(gpu_device, dtype, cpad):
    B, S = 2, 5
    crops = torch.zeros(B * S * S * 3, dtype=torch.uint8, device=gpu_device)
    slot = _slot(gpu_device, 0.0)
    for f32, u8, channels in ((None, None, 0), (None, None, 3), (None, crops, 2), (None, crops, 0)):
        got = _pack(gpu_device, dtype, cpad, B, S, f32, u8, channels, amax=slot[1:], want_rc=REFUSED)
        assert torch.isnan(got).all()
    assert _biteq(slot[1].cpu(), torch.tensor(0.0))


# ---------------------------------------------------------------- pack_input_pad4
def _pad4(dev, B, S, f32, u8, channels, want_rc=0):
    n = B * (S + 6) * (S + 6) * 4
    out = _nan((n + SLACK,), dev, torch.bfloat16)
    rc = _lib.lib().spe_debug_pack_input_pad4(None, _p(f32), _p(u8), channels, _p(out), B, S)
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    assert torch.isnan(out[n:]).all()                            # the element after the last: still NaN
    return out[:n].reshape(B, S + 6, S + 6, 4)


@pytest.mark.parametrize("case", [(1, 2), (2, 5), (2, 16)], ids=_id)
@pytest.mark.parametrize("src", ["f32", "u8x3", "u8x1"])
def test_pack_input_pad4_is_exact_and_rewrites_its_border(gpu_device, src, case):
    """From a NaN-filled buffer (the workspace is shared with later activations): the interior is the bf16 image,
    channel 3 and the whole 3-pixel border are exactly +0."""
    B, S = case
    f32, u8, channels, x3 = _source(gpu_device, src, B, S)
    got = _pad4(gpu_device, B, S, f32, u8, channels)
    want = hr.pack_pad4(x3)
    assert _biteq(got, want)
    assert _biteq(got[:, 3:3 + S, 3:3 + S, :3], x3.to(torch.bfloat16))
    border = torch.ones(S + 6, S + 6, dtype=torch.bool)
    border[3:3 + S, 3:3 + S] = False
    assert (_bits(got.cpu())[:, border] == 0).all() and (_bits(got.cpu())[..., 3] == 0).all()


def test_pack_input_pad4_refuses_a_missing_or_two_channel_source(gpu_device):
    crops = torch.zeros(2 * 5 * 5 * 3, dtype=torch.uint8, device=gpu_device)
    for u8, channels in ((None, 3), (crops, 2)):
        assert torch.isnan(_pad4(gpu_device, 2, 5, None, u8, channels, want_rc=REFUSED)).all()


# ---------------------------------------------------------------- maxpool3s2
# (B, H, W, C, ldo): a one-pixel map / odd H and W, two images / H even and W odd, written into a slice of a
# concat buffer / an even map, more than one workgroup, a slice; fp32 also one 16-byte chunk of four channels
MP_CASES = [(1, 1, 1, 8, 8), (2, 7, 5, 16, 16), (1, 2, 3, 8, 24), (1, 16, 16, 64, 128)]
MP_PARAMS = [(d, c) for d in ("fp32", "bf16") for c in MP_CASES] + [("fp32", (2, 7, 5, 4, 8))]


@pytest.mark.parametrize("kind", ["normal", "negative"])
@pytest.mark.parametrize("dtype,case", MP_PARAMS, ids=_id)
def test_maxpool3s2_is_exact(gpu_device, dtype, case, kind):
    """Random normal input, and a strictly negative one (-1 - |randn|): with a zero pad instead of -inf every border
    window of the latter would give 0."""
    B, H, W, C, ldo = case
    code, tdt, _ = DT[dtype]
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C))
    x = (-1 - x.abs() if kind == "negative" else x).to(tdt)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = B * Ho * Wo
    out = _nan((rows + 3, ldo), gpu_device, tdt)
    xd = x.to(gpu_device)
    rc = _lib.lib().spe_debug_maxpool3s2(None, code, _p(xd), _p(out), B, H, W, C, ldo)
    torch.cuda.synchronize()
    assert rc == 0, rc
    got = out[:rows, :C].cpu().double().reshape(B, Ho, Wo, C)
    assert torch.equal(got, hr.maxpool3s2(x.double()))
    assert torch.isnan(out[:rows, C:]).all() and torch.isnan(out[rows:]).all()
    if kind == "negative":
        assert (got <= -1).all()


def test_maxpool3s2_refuses_shapes_outside_its_contract(gpu_device):
    """C a multiple of the 16-byte chunk (8 bf16, 4 fp32) and ldo >= C: -5 before any launch, nothing written."""
    L, f32, b16 = _lib.lib(), _lib.SPE_DTYPE_F32, _lib.SPE_DTYPE_BF16
    z = torch.zeros(4096, device=gpu_device)
    y = _nan((4096,), gpu_device)
    assert L.spe_debug_maxpool3s2(None, b16, _p(z), _p(y), 1, 4, 4, 12, 16) == REFUSED     # C % 8 in bf16
    assert L.spe_debug_maxpool3s2(None, f32, _p(z), _p(y), 1, 4, 4, 6, 8) == REFUSED       # C % 4 in fp32
    assert L.spe_debug_maxpool3s2(None, f32, _p(z), _p(y), 1, 4, 4, 16, 8) == REFUSED      # ldo < C
    assert L.spe_debug_maxpool3s2(None, b16, _p(z), _p(y), 1, 4, 4, 16, 8) == REFUSED
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ---------------------------------------------------------------- upsample2x
# (B, H, W, C): one pixel / one row / one column (the Ho > 1, Wo > 1 guards) / H != W both ways (swapped axes)
UP_CASES = [(1, 1, 1, 8), (1, 1, 3, 8), (2, 3, 1, 8), (2, 5, 7, 16), (1, 26, 13, 32)]
UP_PARAMS = [(d, c) for d in ("fp32", "bf16") for c in UP_CASES] + [("fp32", (2, 5, 7, 4))]


def _upsample(dev, dtype, case, x=None):
    """-> (the dtype-rounded input on the CPU, the output on the CPU), both NHWC"""
    B, H, W, C = case
    code, tdt, _ = DT[dtype]
    if x is None:
        x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C)) * 2.0
    x = x.to(tdt)
    n = B * 4 * H * W * C
    out = _nan((n + SLACK,), dev, tdt)
    xd = x.to(dev)
    rc = _lib.lib().spe_debug_upsample2x(None, code, _p(xd), _p(out), B, H, W, C)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert torch.isnan(out[n:]).all()
    return x, out[:n].reshape(B, 2 * H, 2 * W, C).cpu()


@pytest.mark.parametrize("dtype,case", UP_PARAMS, ids=_id)
def test_upsample2x_matches_fp64(gpu_device, dtype, case):
    x, got = _upsample(gpu_device, dtype, case)
    ref = hr.upsample2x(x.double())
    assert got.shape == ref.shape
    cpu32 = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    own, err, scale = _err(cpu32, ref), _err(got, ref), max(1.0, ref.abs().max().item())
    gate = max(DT[dtype][2] * scale, 4.0 * own)
    print(f"upsample2x {dtype} {_id(case)}: CPU fp32 vs fp64 {own:.3e}, kernel vs fp64 {err:.3e}, gate {gate:.3e}, max |ref| {scale:.2f}")
    assert err <= gate, (err, gate)                               # (NaN fails)
    # the corners of the output are the corners of the input (align_corners=True)
    assert _err(got[:, 0, 0], x[:, 0, 0]) <= gate and _err(got[:, -1, -1], x[:, -1, -1]) <= gate
    assert _err(got[:, 0, -1], x[:, 0, -1]) <= gate and _err(got[:, -1, 0], x[:, -1, 0]) <= gate


@pytest.mark.parametrize("dtype,case", UP_PARAMS, ids=_id)
def test_upsample2x_of_a_constant_map_is_exact(gpu_device, dtype, case):
    """Per channel a constant 0 or +-2^k (module docstring): bit-equal, whatever the interpolation weights."""
    B, H, W, C = case
    c = torch.arange(C)
    const = torch.where(c % 7 == 3, torch.zeros(C), (1.0 - 2.0 * (c % 2)) * 2.0 ** ((c % 5) - 2.0))
    x, got = _upsample(gpu_device, dtype, case, const.expand(B, H, W, C).contiguous())
    assert _biteq(got, const.to(x.dtype).expand(B, 2 * H, 2 * W, C).contiguous())


def test_upsample2x_refuses_channels_off_the_chunk(gpu_device):
    L = _lib.lib()
    z = torch.zeros(4096, device=gpu_device)
    y = _nan((4096,), gpu_device)
    assert L.spe_debug_upsample2x(None, _lib.SPE_DTYPE_BF16, _p(z), _p(y), 1, 2, 2, 12) == REFUSED
    assert L.spe_debug_upsample2x(None, _lib.SPE_DTYPE_F32, _p(z), _p(y), 1, 2, 2, 6) == REFUSED
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ---------------------------------------------------------------- heads
HEAD_OUT = {"logits": 12, "points": 2, "probs": 12, "points_px": 2, "log_sigmas": 2, "sigmas": 2}
# (B, Q): a lone row / a ragged last workgroup of 4 rows / aligned rows / Q = 11: workgroups whose rows straddle
# two images with different crop boxes
HEAD_CASES = [(1, 1), (1, 5), (3, 4), (2, 11)]


@functools.lru_cache(maxsize=None)
def _head_inputs(B, Q):
    """Weights as torch stores them, randn / 16 (biases 0.2 randn), hs randn, per image a distinct non-square crop
    box with a non-zero origin; and the restatement's outputs in fp64 and in fp32 on the CPU."""
    g = torch.Generator().manual_seed(100 * B + Q)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = {"cls_w": rn(12, 256) / 16, "cls_b": 0.2 * rn(12)}
    for p, n in (("pt", 2), ("sg", 1)):
        w.update({p + "_w0": rn(256, 256) / 16, p + "_b0": 0.2 * rn(256), p + "_w1": rn(256, 256) / 16, p + "_b1": 0.2 * rn(256),
                  p + "_w2": rn(n, 256) / 16, p + "_b2": 0.2 * rn(n)})
    hs = rn(B * Q, 256)
    clip = torch.tensor([[10.0 + 37 * b, 20.0 + 11 * b, 110.0 + 87 * b, 100.0 + 41 * b] for b in range(B)])
    ref64 = hr.heads(hs.double(), {k: v.double() for k, v in w.items()}, Q, clip.double())
    ref32 = hr.heads(hs, w, Q, clip)
    return w, hs, clip, ref64, ref32


def _heads(dev, B, Q, sigma=True, probs=True, px=True, clip=True, D=256, want_rc=0, inputs=None):
    """Runs the kernel with every output pointer given except those switched off; -> the outputs' first B * Q rows
    (on the device).  The rows after them must still be NaN."""
    w, hs, clip_bbox, _, _ = _head_inputs(*(inputs or (B, Q)))
    rows = B * Q
    d = {k: (v.t().contiguous() if v.dim() == 2 else v).to(dev) for k, v in w.items()}      # [in][out], as the kernel reads them
    hs_d, clip_d = hs.to(dev), clip_bbox.to(dev)
    out = {k: _nan((rows + 3, n), dev) for k, n in HEAD_OUT.items()}
    wb = [d[p + s] for p in ("pt", "sg") for s in ("_w0", "_b0", "_w1", "_b1", "_w2", "_b2")]
    if not sigma:
        wb[6:] = [None] * 6
    rc = _lib.lib().spe_debug_heads(None, _p(hs_d), B, Q, D, _p(d["cls_w"]), _p(d["cls_b"]), *[_p(t) for t in wb],
                                    _p(clip_d) if clip else None, _p(out["logits"]), _p(out["points"]),
                                    _p(out["probs"]) if probs else None, _p(out["points_px"]) if px else None,
                                    _p(out["log_sigmas"]), _p(out["sigmas"]))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    for k, v in out.items():
        assert torch.isnan(v[rows:]).all(), k
    return {k: v[:rows] for k, v in out.items()}


@pytest.mark.parametrize("sigma", [True, False], ids=["sigma", "nosigma"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=_id)
def test_heads_match_fp64(gpu_device, case, sigma):
    B, Q = case
    _, _, clip, ref64, ref32 = _head_inputs(B, Q)
    got = {k: v.cpu() for k, v in _heads(gpu_device, B, Q, sigma=sigma).items()}
    for k in ("logits", "points") + (("log_sigmas",) if sigma else ()):
        own, err, scale = _err(ref32[k], ref64[k]), _err(got[k], ref64[k]), max(1.0, ref64[k].abs().max().item())
        gate = max(1e-5 * scale, 4.0 * own)
        print(f"heads {B}x{Q} {k}: CPU fp32 vs fp64 {own:.3e}, kernel vs fp64 {err:.3e}, gate {gate:.3e}, max |ref| {scale:.2f}")
        assert err <= gate, (k, err, gate)                        # (NaN fails)
    assert _err(got["probs"], hr.softmax(got["logits"].double())) <= 1e-6
    # image pixels: torch fp32, two rounded operations, on the kernel's own points and each row's own image's box
    bb = clip[torch.arange(B * Q) // Q]
    scaled = got["points"] * (bb[:, 2:4] - bb[:, 0:2])
    assert _biteq(got["points_px"], scaled + bb[:, 0:2])
    if B > 1:
        other = clip[(torch.arange(B * Q) // Q + 1) % B]
        assert ((got["points_px"] - (got["points"] * (other[:, 2:4] - other[:, 0:2]) + other[:, 0:2])).abs() > 1.0).all()
    if sigma:
        assert ref64["log_sigmas"].abs().max().item() <= 5.0       # so that the relative gate on exp means something
        want = torch.exp(got["log_sigmas"].double())
        assert ((got["sigmas"].double() - want).abs() / want).max().item() <= 1e-6
        assert _biteq(got["log_sigmas"][:, 0], got["log_sigmas"][:, 1]) and _biteq(got["sigmas"][:, 0], got["sigmas"][:, 1])
    else:
        assert torch.isnan(got["log_sigmas"]).all() and torch.isnan(got["sigmas"]).all()


@pytest.mark.parametrize("off", ["probs", "points_px", "clip_bbox"])
def test_heads_optional_outputs(gpu_device, off):
    """probs, points_px or clip_bbox null: that output (points_px without a crop box) is not written, every other
    one is bit-equal to the run with all of them."""
    B, Q = 2, 11
    full = _heads(gpu_device, B, Q)
    part = _heads(gpu_device, B, Q, probs=off != "probs", px=off != "points_px", clip=off != "clip_bbox")
    absent = "points_px" if off == "clip_bbox" else off
    for k in HEAD_OUT:
        if k == absent:
            assert torch.isnan(part[k]).all(), k
        else:
            assert not torch.isnan(full[k]).any() and _biteq(part[k], full[k]), k


def test_heads_empty_batch_writes_nothing(gpu_device):
    got = _heads(gpu_device, 0, 11, inputs=(2, 11))
    assert all(v.numel() == 0 for v in got.values())             # (_heads checked the rows after B * Q = 0: all NaN)


def test_heads_refuse_another_width(gpu_device):
    got = _heads(gpu_device, 1, 5, D=128, want_rc=BAD_SHAPE)
    assert all(torch.isnan(v).all() for v in got.values())


# ---------------------------------------------------------------- postprocess
def _postprocess(dev, logits, points, clip, B, Q):
    rows = B * Q
    probs, px = _nan((rows + 3, 12), dev), _nan((rows + 3, 2), dev)
    rc = _lib.lib().spe_postprocess(None, _p(logits), _p(points), _p(clip), B, Q, _p(probs), _p(px))
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert torch.isnan(probs[rows:]).all() and torch.isnan(px[rows:]).all()
    return probs[:rows], px[:rows]


def test_postprocess_is_the_fused_kernels_tail(gpu_device):
    """On the logits, points and crop boxes of a heads run: bit-equal probs and points_px (the same source, file
    and flags)."""
    B, Q = 2, 11
    full = _heads(gpu_device, B, Q)
    clip = _head_inputs(B, Q)[2].to(gpu_device)
    probs, px = _postprocess(gpu_device, full["logits"].contiguous(), full["points"].contiguous(), clip, B, Q)
    assert _biteq(probs, full["probs"]) and _biteq(px, full["points_px"])


def test_postprocess_alone_more_rows_than_a_block(gpu_device):
    """(B, Q) = (2, 70): 140 rows, one 128-thread block and a ragged second."""
    B, Q = 2, 70
    g = torch.Generator().manual_seed(7)
    logits, points = torch.randn(B * Q, 12, generator=g) * 3.0, torch.rand(B * Q, 2, generator=g)
    clip = torch.tensor([[10.0, 20.0, 110.0, 100.0], [-47.0, 31.0, 190.0, 141.0]])
    probs, px = _postprocess(gpu_device, logits.to(gpu_device), points.to(gpu_device), clip.to(gpu_device), B, Q)
    assert _err(probs, hr.softmax(logits.double())) <= 1e-6
    bb = clip[torch.arange(B * Q) // Q]
    scaled = points * (bb[:, 2:4] - bb[:, 0:2])
    assert _biteq(px.cpu(), scaled + bb[:, 0:2])
    assert _err(px, hr.rescale(points.double(), clip.double(), Q)) <= 1e-5 * 190.0


def test_postprocess_empty_batch_writes_nothing(gpu_device):
    z = torch.zeros(64, device=gpu_device)
    probs, px = _postprocess(gpu_device, z, z, z, 0, 11)
    assert probs.numel() == 0 and px.numel() == 0


# ---------------------------------------------------------------- layernorm
def _layernorm(dev, dtype, x, gam, bet, out=True, out32=True, M=None, D=256, want_rc=0):
    """x [rows][256] already rounded to dtype, on the CPU -> (out, out_f32) on the CPU, rows M and after still NaN"""
    code, tdt, _ = DT[dtype]
    M = x.shape[0] if M is None else M
    o, o32 = _nan((x.shape[0] + 2, 256), dev, tdt), _nan((x.shape[0] + 2, 256), dev)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    rc = _lib.lib().spe_debug_layernorm(None, code, _p(xd), _p(gd), _p(bd), _p(o) if out else None, _p(o32) if out32 else None, M, D)
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    if want_rc != 0:
        M = 0
    assert torch.isnan(o[M:]).all() and torch.isnan(o32[M:]).all()
    assert out or torch.isnan(o).all()
    assert out32 or torch.isnan(o32).all()
    return o[:M].cpu(), o32[:M].cpu()


def _ln_inputs(M, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + M)
    x = (torch.randn(M, 256, generator=g) * 3 + 1).to(DT[dtype][1])
    return x, torch.randn(256, generator=g), torch.randn(256, generator=g)


@pytest.mark.parametrize("outs", ["both", "out", "out_f32"])
@pytest.mark.parametrize("M", [1, 4, 5])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layernorm_few_rows_and_either_output(gpu_device, dtype, M, outs):
    """One row, one full workgroup of 4 rows, a ragged second one; both outputs, or one of them null."""
    x, gam, bet = _ln_inputs(M, dtype)
    o, o32 = _layernorm(gpu_device, dtype, x, gam, bet, out=outs != "out_f32", out32=outs != "out")
    ref = hr.layernorm(x.double(), gam.double(), bet.double())
    scale = max(1.0, ref.abs().max().item())
    if outs != "out_f32":
        assert _err(o, ref) <= DT[dtype][2] * scale
    if outs != "out":
        assert _err(o32, ref) <= 1e-5 * scale
    if outs == "both":
        assert _biteq(o, o32.to(o.dtype))                         # one result, stored twice


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layernorm_of_a_constant_row_is_beta(gpu_device, dtype):
    """256 x 3.25 sums exactly, so the mean is 3.25 and every difference 0: beta exactly (and its bf16 rounding)."""
    x, gam, bet = _ln_inputs(5, dtype)
    x[2] = 3.25
    o, o32 = _layernorm(gpu_device, dtype, x, gam, bet)
    assert torch.equal(o32[2], bet) and torch.equal(o[2], bet.to(o.dtype))
    assert not torch.equal(o32[1], bet)


def test_layernorm_large_mean_small_spread(gpu_device):
    """Rows of mean 1e3 and standard deviation 0.1, fp32 (module docstring)."""
    g = torch.Generator().manual_seed(11)
    x = 1e3 + 0.1 * torch.randn(4, 256, generator=g)
    gam, bet = torch.randn(256, generator=g), torch.randn(256, generator=g)
    o, o32 = _layernorm(gpu_device, "fp32", x, gam, bet)
    ref = hr.layernorm(x.double(), gam.double(), bet.double())
    own, err, scale = _err(F.layer_norm(x, (256,), gam, bet, 1e-5), ref), _err(o32, ref), max(1.0, ref.abs().max().item())
    gate = max(1e-5 * scale, 4.0 * own)
    print(f"layernorm mean 1e3 std 0.1: CPU fp32 vs fp64 {own:.3e}, kernel vs fp64 {err:.3e}, gate {gate:.3e}, max |ref| {scale:.2f}")
    assert err <= gate, (err, gate)
    assert _biteq(o, o32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_layernorm_refuses_another_width_and_accepts_no_rows(gpu_device, dtype):
    """D = 128: -6 before any launch.  M = 0: 0, and nothing is launched (an empty grid is an invalid launch
    configuration).  Neither writes."""
    x, gam, bet = _ln_inputs(4, dtype)
    _layernorm(gpu_device, dtype, x, gam, bet, D=128, want_rc=BAD_SHAPE)
    o, o32 = _layernorm(gpu_device, dtype, x, gam, bet, M=0)
    assert o.numel() == 0 and o32.numel() == 0                    # (_layernorm checked rows 0 and after: all NaN)
