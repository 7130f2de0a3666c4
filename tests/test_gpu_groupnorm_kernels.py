"""GPU: the GroupNorm kernels (csrc/groupnorm.hip: norm.gn.stats + norm.gn.apply) alone, through spe_debug_groupnorm,
against the fp64 restatement of their contract (tests/groupnorm_ref.py).

Shapes are the smallest at which each mechanism can break: C = 64 (2 channels a group: four groups inside one 16-byte
bf16 vector), 256 and 1024 (32 channels a group: a group over several vectors, and over waves); B = 2 (statistics
must not leak between images); 5 x 5 and 13 x 7 pixels (no multiple of any tile; at C = 1024 the 91 pixels split
into ragged tiles of 16); 104 x 104 x 64 (43 tiles a group); row strides C and C + 8; residual and ReLU on and off.

Bounds:
  fp32 storage  |y - fp64| <= 2e-6 max|y|
  bf16 storage  every element bit-equal to, or one bf16 ulp from, the bf16-emulating restatement (the same stored
                inputs, fp32 statistics, one final rounding) -- or, where |y| is so small that its ulp is below the
                fp32 arithmetic's own error, within that error (the fp32 bound above): there the sign itself is noise
  conditioning  x = 100 + N(0, 1) in fp32 storage stays within 1e-4 of fp64; a one-pass fp32 variance does not
  two launches give the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import groupnorm_ref as gr
from spe import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 5, 64), (2, 13, 7, 64), (2, 5, 5, 1024), (2, 13, 7, 1024), (2, 13, 7, 256), (1, 104, 104, 64)]
# (row stride pad, residual, relu)
VARIANTS = [(0, False, False), (8, True, True), (0, True, False), (8, False, True)]
DT = {"fp32": (torch.float32, _lib.SPE_DTYPE_F32), "bf16": (torch.bfloat16, _lib.SPE_DTYPE_BF16)}
_inputs = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _case(shape):
    """x, residual (bf16-representable, so both storages read the same values), gamma, beta; drawn once per shape"""
    if shape not in _inputs:
        rng = np.random.default_rng(1000 + sum(shape))
        C = shape[-1]
        _inputs[shape] = (gr.to_bf16(rng.normal(0.3, 1.7, shape)), gr.to_bf16(rng.normal(0.0, 1.0, shape)),
                          rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0.0, 0.2, C).astype(np.float32))
    return _inputs[shape]


def _rows(a, ld, tdt, dev, fill=7.0):
    """[B, H, W, C] values -> device rows [B*H*W][ld] of dtype tdt, the pad columns holding `fill`"""
    C = a.shape[-1]
    t = torch.full((a.size // C, ld), fill, dtype=tdt, device=dev)
    t[:, :C] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, C)).to(dev, tdt)
    return t


def _launch(dev, dtype, x, gamma, beta, res=None, relu=False, pad=0, inplace=False, scratch=None):
    tdt, code = DT[dtype]
    B, H, W, C = x.shape
    ld = C + pad
    xd = _rows(x, ld, tdt, dev)
    rd = _rows(res, ld, tdt, dev) if res is not None else None
    yd = xd if inplace else torch.full_like(xd, 7.0)
    L = _lib.lib()
    nb = L.spe_debug_groupnorm_scratch_bytes(B, H, W, C)
    assert nb == B * gr.tiles(H, W, C) * 32 * 3 * 4
    sc = scratch if scratch is not None else torch.empty(nb, dtype=torch.uint8, device=dev)
    g, b = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    rc = L.spe_debug_groupnorm(None, code, _p(xd), ld, _p(rd), ld, _p(g), _p(b), _p(yd), ld, B, H, W, C, int(relu),
                               _p(sc), sc.numel())
    assert rc == 0, L.spe_last_error()
    torch.cuda.synchronize()
    if pad and not inplace:
        assert (yd[:, C:].float() == 7.0).all()          # nothing written past C
    return yd[:, :C].float().cpu().numpy().reshape(x.shape), yd


@pytest.mark.parametrize("pad,with_res,relu", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_groupnorm_fp32(gpu_device, shape, pad, with_res, relu):
    x, res, gamma, beta = _case(shape)
    ref = gr.group_norm(x, gamma, beta, res if with_res else None, relu)
    got, _ = _launch(gpu_device, "fp32", x, gamma, beta, res if with_res else None, relu, pad)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"groupnorm fp32 {shape} pad {pad} res {with_res} relu {relu}: err {err:.3e} max|y| {scale:.3e}")
    assert err <= 2e-6 * scale


@pytest.mark.parametrize("pad,with_res,relu", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_groupnorm_bf16(gpu_device, shape, pad, with_res, relu):
    x, res, gamma, beta = _case(shape)
    emu = gr.group_norm_bf16(x, gamma, beta, res if with_res else None, relu)
    got, _ = _launch(gpu_device, "bf16", x, gamma, beta, res if with_res else None, relu, pad)
    ulps = np.abs(gr.bf16_bits(got) - gr.bf16_bits(emu))
    noise = 2e-6 * np.abs(emu).max()
    bad = (ulps > 1) & (np.abs(got - emu) > noise)
    print(f"groupnorm bf16 {shape} pad {pad} res {with_res} relu {relu}: {int((ulps == 0).sum())} of {ulps.size} "
          f"bit-equal, {int((ulps == 1).sum())} one ulp off, {int(bad.sum())} further")
    assert not bad.any()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_in_place(gpu_device, dtype):
    """y == x, the model's form, gives the out-of-place bits."""
    x, res, gamma, beta = _case((2, 13, 7, 1024))
    ref, _ = _launch(gpu_device, dtype, x, gamma, beta, res, True, 8)
    got, _ = _launch(gpu_device, dtype, x, gamma, beta, res, True, 8, inplace=True)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 13, 7, 1024), (1, 104, 104, 64)])
def test_two_launches_same_bits(gpu_device, shape, dtype):
    x, res, gamma, beta = _case(shape)
    _, a = _launch(gpu_device, dtype, x, gamma, beta, res, True)
    _, b = _launch(gpu_device, dtype, x, gamma, beta, res, True)
    assert torch.equal(a, b)


def test_split_over_work_groups_is_taken():
    """104 x 104 x 64: more than one partial per (image, group); 13 x 7 x 1024: ragged tiles (91 = 5 * 16 + 11)."""
    L = _lib.lib()
    assert L.spe_debug_groupnorm_scratch_bytes(1, 104, 104, 64) // (32 * 3 * 4) == 43
    assert L.spe_debug_groupnorm_scratch_bytes(2, 13, 7, 1024) // (2 * 32 * 3 * 4) == 6
    assert L.spe_debug_groupnorm_scratch_bytes(2, 5, 5, 64) // (2 * 32 * 3 * 4) == 1


def test_conditioning(gpu_device):
    """x = 100 + N(0, 1), fp32 storage, 11 tiles a group: within 1e-4 of fp64 on the normalised output, where the
    one-pass fp32 variance (numpy, same input) is not -- the case separates the two."""
    rng = np.random.default_rng(5)
    shape = (2, 26, 26, 256)
    x = (100.0 + rng.normal(0, 1, shape)).astype(np.float32)
    gamma, beta = np.ones(256, np.float32), np.zeros(256, np.float32)
    ref = gr.group_norm(x, gamma, beta)
    got, _ = _launch(gpu_device, "fp32", x, gamma, beta)
    m1, v1 = gr.one_pass_f32(x)
    one_pass = gr._finish(x, m1, np.maximum(v1, 0), gamma, beta, None, False, np.float64)
    err, err1 = np.abs(got - ref).max(), np.abs(one_pass - ref).max()
    print(f"groupnorm conditioning: kernel {err:.3e}, one-pass fp32 variance {err1:.3e} (bound 1e-4)")
    assert err1 > 1e-4
    assert err <= 1e-4


def test_refusals(gpu_device):
    """Every SPE_E_ARG (-1) refusal, before any launch: the output keeps its fill."""
    dev = gpu_device
    L = _lib.lib()
    C, B, H, W = 64, 1, 5, 5
    x = torch.zeros(B * H * W, 128, device=dev)
    y = torch.full_like(x, 7.0)
    g, b = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    sc = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    need = L.spe_debug_groupnorm_scratch_bytes(B, H, W, C)
    assert 0 < need <= sc.numel()

    def call(dtype=_lib.SPE_DTYPE_F32, x=x, ldx=128, res=None, ldr=128, g=g, b=b, y=y, ldy=128, C=C, sc=sc, nbytes=None):
        return L.spe_debug_groupnorm(None, dtype, _p(x), ldx, _p(res), ldr, _p(g), _p(b), _p(y), ldy, B, H, W, C, 0,
                                     _p(sc), sc.numel() if nbytes is None and sc is not None else (nbytes or 0))
    assert call() == 0
    torch.cuda.synchronize()
    y.fill_(7.0)
    refused = {
        "C no multiple of 32": call(C=48), "C / 32 = 3": call(C=96), "ldx below C": call(ldx=56),
        "ldx no multiple of 8": call(ldx=68), "ldy below C": call(ldy=56), "ldy no multiple of 8": call(ldy=68),
        "residual ld below C": call(res=x, ldr=56), "residual ld no multiple of 8": call(res=x, ldr=68),
        "null x": call(x=None), "null gamma": call(g=None), "null beta": call(b=None), "null y": call(y=None),
        "null scratch": call(sc=None), "scratch too small": call(nbytes=need - 1), "dtype": call(dtype=_lib.SPE_DTYPE_F16),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    assert L.spe_debug_groupnorm_scratch_bytes(B, H, W, 48) == 0
    torch.cuda.synchronize()
    assert (y == 7.0).all()
