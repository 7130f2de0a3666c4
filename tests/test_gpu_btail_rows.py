"""GPU: the layer-1 bottleneck tail (btail.hip) with 16-byte row pieces and with the compact y store,
through spe_debug_btail_rows:

    y = relu(A . W3^T + b3 (+ R))      z = relu(y . W1^T + b1)

* rows = 1 (16-byte pieces of R, y, z; the default) against rows = 0 (8-byte pieces), bit for bit, for
  the three instantiations, and both against an fp64 product of the same bf16-rounded operands (z
  against the product of the KERNEL's bf16 y, the separate launches' intermediate) at the tolerance
  of tests/test_gpu_btail_wide.py: max|d| <= 1e-2 * max(1, max|reference|).
* the compact store (the layer-1 -> layer-2 tail): only the pixels with even h and even w, densely;
  equal to that subset of the whole y bit for bit, z unchanged, nothing written past its end; odd
  H or W stores y whole.
* the bf16 model on the s128_q11_l2 golden's weights: bit-identical outputs under both knobs.

Outputs start as NaN, so an element the kernel does not write fails; row strides are wider than the
rows, and the columns between the rows must stay NaN.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from spe import _lib

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-2
PAD = 8                                                    # extra elements per row (strides stay 16-byte multiples)
SHAPES = [(64, 64, True), (64, 128, True), (128, 64, False)]   # (K1, N2, residual): the three instantiations
# one partial tile, the tile edge on both sides, fewer tiles than waves, and 16 tiles of 16 rows + 5
ROWS_M = [1, 15, 16, 17, 129, 16 * 8 * 2 + 5]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int16)


def _operands(dev, M, k1, n2, res):
    dt = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(1000 * k1 + n2 + M)
    A = torch.randn(M, k1 + PAD, generator=g).to(dev, dt)
    R = torch.randn(M, 256 + PAD, generator=g).to(dev, dt) if res else None
    W3 = (torch.randn(256, k1, generator=g) / k1 ** 0.5).to(dev, dt)
    b3 = (0.1 * torch.randn(256, generator=g)).to(dev)
    W1 = (torch.randn(n2, 256, generator=g) / 16).to(dev, dt)
    b1 = (0.1 * torch.randn(n2, generator=g)).to(dev)
    return A, R, W3, b3, W1, b1


def _launch(dev, ops, k1, n2, M, rows, H=0, W=0, y_rows=None, guard=0):
    """(rc, Y, Z): Y has y_rows (default M) rows plus `guard` rows that nobody may write."""
    L = _lib.lib()
    A, R, W3, b3, W1, b1 = ops
    perm = torch.tensor([L.spe_debug_btail_perm(k) for k in range(256)], device=dev)
    W1p = W1[:, perm].contiguous()
    Y = torch.full(((M if y_rows is None else y_rows) + guard, 256 + PAD), float("nan"), dtype=torch.bfloat16, device=dev)
    Z = torch.full((M, n2 + PAD), float("nan"), dtype=torch.bfloat16, device=dev)
    rc = L.spe_debug_btail_rows(None, _p(A), k1 + PAD, k1, _p(R), 256 + PAD, _p(W3), k1, _p(b3), _p(Y), 256 + PAD,
                                _p(W1p), 256, _p(b1), _p(Z), n2 + PAD, n2, M, rows, H, W)
    torch.cuda.synchronize()
    return rc, Y, Z


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.double() - ref).abs().max().item()
    print(f"max|d| = {err:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


def _check_fp64(ops, k1, n2, Y, Z):
    A, R, W3, b3, W1, b1 = ops
    yref = torch.relu(A[:, :k1].double() @ W3.double().t() + b3.double() + (R[:, :256].double() if R is not None else 0))
    _close(Y[:, :256], yref, TOL_BF16)
    zref = torch.relu(Y[:, :256].double() @ W1.double().t() + b1.double())
    _close(Z[:, :n2], zref, TOL_BF16)
    assert torch.isnan(Y[:, 256:]).all() and torch.isnan(Z[:, n2:]).all()


def _rows_cases(gpu_device):
    # more tiles than the persistent grid has waves (8 per CU): both operand sets rotate, the last tile partial
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    return ROWS_M + [16 * (2 * 8 * cus + 3) + 5]


@pytest.mark.parametrize("k1,n2,res", SHAPES)
def test_rows16_equals_rows8_bit_for_bit(gpu_device, k1, n2, res):
    for M in _rows_cases(gpu_device):
        ops = _operands(gpu_device, M, k1, n2, res)
        rc8, Y8, Z8 = _launch(gpu_device, ops, k1, n2, M, rows=0)
        rc16, Y16, Z16 = _launch(gpu_device, ops, k1, n2, M, rows=1)
        assert rc8 == 0 and rc16 == 0, (M, _lib.lib().spe_last_error())
        _check_fp64(ops, k1, n2, Y8, Z8)
        _check_fp64(ops, k1, n2, Y16, Z16)
        dy = (_bits(Y16[:, :256]) != _bits(Y8[:, :256])).sum().item()
        dz = (_bits(Z16[:, :n2]) != _bits(Z8[:, :n2])).sum().item()
        print(f"M = {M}: y differs in {dy} elements, z in {dz}")
        assert dy == 0 and dz == 0, (M, dy, dz)


def test_rows16_needs_16_byte_row_strides(gpu_device):
    """A stride of 4 elements more than the row serves the 8-byte pieces only: rows = 1 launches nothing."""
    L = _lib.lib()
    M, k1, n2 = 40, 64, 64
    A, R, W3, b3, W1, b1 = _operands(gpu_device, M, k1, n2, True)
    Y = torch.full((M, 260), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    Z = torch.full((M, n2), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    rc = L.spe_debug_btail_rows(None, _p(A), k1 + PAD, k1, _p(R), 256 + PAD, _p(W3), k1, _p(b3), _p(Y), 260, _p(W1), 256,
                                _p(b1), _p(Z), n2, n2, M, 1, 0, 0)
    torch.cuda.synchronize()
    assert rc == 1
    assert torch.isnan(Y).all() and torch.isnan(Z).all()


def _even_pixels(Y, B, H, W):
    return Y[: B * H * W].view(B, H, W, -1)[:, 0::2, 0::2].reshape(B * (H // 2) * (W // 2), -1)


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("H,W", [(4, 6), (6, 4), (2, 2)])
def test_compact_y_is_the_even_pixel_subset(gpu_device, H, W, rows):
    B, k1, n2 = 2, 64, 128
    M, Mc, guard = B * H * W, B * (H // 2) * (W // 2), 3
    ops = _operands(gpu_device, M, k1, n2, True)
    rc, Yf, Zf = _launch(gpu_device, ops, k1, n2, M, rows)
    assert rc == 0
    _check_fp64(ops, k1, n2, Yf, Zf)
    rc, Yc, Zc = _launch(gpu_device, ops, k1, n2, M, rows, H, W, y_rows=Mc, guard=guard)
    assert rc == 2, "the compact store did not run"
    assert torch.equal(_bits(Yc[:Mc, :256]), _bits(_even_pixels(Yf, B, H, W)[:, :256]))
    assert torch.equal(_bits(Zc[:, :n2]), _bits(Zf[:, :n2]))
    assert not torch.isnan(Yc[:Mc, :256]).any()
    # nothing beyond the compact buffer, nothing between its rows, nothing between z's rows
    assert torch.isnan(Yc[Mc:]).all() and torch.isnan(Yc[:, 256:]).all() and torch.isnan(Zc[:, n2:]).all()


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("H,W", [(3, 4), (4, 3)])
def test_odd_edges_store_y_whole(gpu_device, H, W, rows):
    B, k1, n2 = 2, 64, 128
    M = B * H * W
    ops = _operands(gpu_device, M, k1, n2, True)
    rc, Yf, Zf = _launch(gpu_device, ops, k1, n2, M, rows)
    assert rc == 0
    rc, Y, Z = _launch(gpu_device, ops, k1, n2, M, rows, H, W, guard=2)
    assert rc == 0, "an odd edge must take the whole store"
    assert torch.equal(_bits(Y[:M, :256]), _bits(Yf[:, :256])) and torch.equal(_bits(Z[:, :n2]), _bits(Zf[:, :n2]))
    assert torch.isnan(Y[M:]).all()


def test_compact_request_on_the_other_instantiations_stores_y_whole(gpu_device):
    """Only the (64, 128, residual) tail has a stride-2 reader: elsewhere the request is answered with the whole y."""
    for k1, n2, res in (SHAPES[0], SHAPES[2]):
        M = 2 * 4 * 4
        ops = _operands(gpu_device, M, k1, n2, res)
        rc, Y, Z = _launch(gpu_device, ops, k1, n2, M, 1, 4, 4)
        assert rc == 0
        _check_fp64(ops, k1, n2, Y, Z)


def test_bf16_model_is_bit_identical_under_both_knobs(gpu_device, monkeypatch):
    """The s128_q11_l2 golden's configuration and weights, at a batch large enough that the layer-1 -> layer-2 tail
    takes the compact store (forward.cpp keeps y whole below one tile per wave): the model reads both knobs when
    it is finalized, so one process builds all four variants.  The launch table tells which path ran: the compact
    tail and the downsample after it account for fewer bytes."""
    import helpers
    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import random_weights, synthetic_batch
    g = np.load(os.path.join(GOLDEN, "model_s128_q11_l2.npz"))
    cfg = SpeConfig(**json.loads(str(g["config"])))
    w = random_weights(cfg, int(g["weight_seed"]))
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    B = -(-16 * 8 * cus // (32 * 32)) + 1                   # layer 1 runs at (S / 4)^2 = 32^2 pixels an image
    b = synthetic_batch(cfg, B, int(g["image_seed"]))
    img = torch.from_numpy(b["images"]).to(gpu_device)
    clip = torch.from_numpy(b["clip_bbox"]).float().to(gpu_device)
    outs, nbytes = {}, {}
    for rows, yc in ((1, 1), (0, 1), (1, 0), (0, 0)):
        monkeypatch.setenv("SPE_BTAIL_ROWS", str(rows))
        monkeypatch.setenv("SPE_BTAIL_YCOMPACT", str(yc))
        m = DETR(cfg, dtype="bf16")
        m.load_state_dict(w)
        o = {}
        table = helpers.launch_table(m, lambda: o.update(m(img, clip_bbox=clip)))
        outs[rows, yc] = {k: v.cpu() for k, v in o.items() if torch.is_tensor(v)}
        nbytes[rows, yc] = sum(r[2] for r in table if r[0].startswith("conv.1x1"))
    M = B * 32 * 32
    for rows in (0, 1):
        # y [M][256] stored as a quarter, and the downsample reads that quarter instead of a strided whole
        assert nbytes[rows, 0] - nbytes[rows, 1] == 2 * (M * 256 * 2 * 3 // 4), nbytes
    ref = outs[0, 0]
    assert {"pred_points", "pred_logits"} <= set(ref)
    diff = {(key, k): int((o[k] != v).sum()) for key, o in outs.items() for k, v in ref.items()
            if not torch.equal(o[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))}
    print("(rows, ycompact), output -> differing elements:", diff)
    assert not diff, diff
