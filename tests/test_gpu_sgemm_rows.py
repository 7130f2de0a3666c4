"""GPU: the streaming GEMM's row-major epilogue (gemm_stream.hip) with 16-byte row pieces, through
spe_debug_gemm:

    C = act(A . W^T + bias (+ R))        bf16 operands, bf16 or fp16 output

* every case against an fp64 product of the same bf16-rounded operands at the tolerance of
  tests/test_gpu_kernels.py test_gemm_streaming_short_k: max|d| <= 1e-2 * max(1, max|reference|);
* every case byte for byte against the 8-byte pieces.  SPE_SGEMM_ROWS is read once per process, so the
  two forms run in two child processes (started side by side, once for the module); each child checks
  its outputs against fp64 and reports a SHA-256 of every whole output buffer, guard rows and the
  columns between the rows included.

The shapes are the smallest that reach the kernel (two row tiles per wave of the persistent grid, from
the device's CU count), plus two tiles and 5 rows: M is no multiple of 16, the last tile's tail rows go
to the sink line.  Outputs start as NaN: an element the kernel does not write fails, and the guard rows
after row M, the columns between the rows and the other half of an ldc = 2N buffer must stay NaN.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-2
GUARD = 3                                                   # rows after row M that nobody may write

# (K, N, residual) -> (BN, RF, OCC) of the instantiation spe_launch_sgemm takes (gemm_stream.hip)
TILES = {(256, 512): (256, 1, 1), (256, 256): (256, 1, 1), (512, 128): (128, 1, 1), (64, 64): (64, 2, 2),
         (128, 512): (256, 1, 2)}


def _case(K, N, res=None, relu=0, f16=0, ldc="pad", ldr="pad"):
    """res: None, "full" (one row per output row) or a period; ldc: "pad" (N + 8), "lo" / "hi" (2N, the first /
    the second half), "off4" (N + 8, from column 4: a base that is no 16-byte multiple), "odd4" (N + 4: rows that are
    no 16-byte multiples); ldr: "pad" (N + 8) or "off4" (N + 8, from column 4)."""
    return dict(K=K, N=N, res=res, relu=relu, f16=f16, ldc=ldc, ldr=ldr)


CASES = {}
for _K, _N in [(256, 512), (256, 256), (512, 128), (64, 64)]:
    for _res in (None, "full"):
        for _relu in (0, 1):
            CASES[f"k{_K}_n{_N}_{'res' if _res else 'nores'}{'_relu' if _relu else ''}"] = _case(_K, _N, _res, _relu)
CASES.update({
    # (without a residual K = 128, N = 512 belongs to the 256-row tiles of gemm2)
    "k128_n512_res": _case(128, 512, "full"),
    "k128_n512_res_relu": _case(128, 512, "full", 1),
    # the encoder's q/k projection: the pos . W^T table of one image's 52 x 52 tokens, fp16 out
    "k256_n512_period2704_f16": _case(256, 512, 2704, f16=1),
    "k256_n512_period2704": _case(256, 512, 2704),
    "k256_n256_period1001": _case(256, 256, 1001),          # a period that is no multiple of 16
    "k64_n64_period1001_relu": _case(64, 64, 1001, 1),
    "k256_n256_ldc2n_lo": _case(256, 256, ldc="lo"),
    "k256_n256_ldc2n_hi_res_relu": _case(256, 256, "full", 1, ldc="hi"),   # (the neck's cat buffer)
    "k512_n128_ldc2n_hi": _case(512, 128, ldc="hi"),
    "k256_n256_f16_relu": _case(256, 256, relu=1, f16=1),
    # bases the 16-byte pieces cannot serve: the 8-byte form, on both sides
    "k256_n256_c_off4": _case(256, 256, ldc="off4"),
    "k256_n256_res_c_off4": _case(256, 256, "full", ldc="off4"),
    "k256_n512_res_r_off4_relu": _case(256, 512, "full", 1, ldr="off4"),
    "k64_n64_c_off4_relu": _case(64, 64, relu=1, ldc="off4"),
})
# ldc % 8 == 4: spe_launch_gemm (the hook's dispatcher) turns a bf16 row stride that is no 16-byte multiple away
# before any kernel is chosen, under either knob: no launch, nothing written (see the test below)
ODD4 = _case(256, 256, "full", ldc="odd4")


def _run_case(name, c, dev, cus):
    import ctypes
    import torch
    from spe import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    K, N = c["K"], c["N"]
    BN, RF, OCC = TILES[K, N]
    nsc = N // BN
    G = (cus * OCC // nsc) * nsc
    M = 2 * (G // nsc) * 4 * RF * 16 + 2 * RF * 16 + 5      # two tiles per wave, two more, 5 rows: M % 16 = 5
    dt = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(sorted(CASES).index(name) + 17 if name in CASES else 16)
    A = torch.randn(M, K, generator=g).to(dev, dt)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev, dt)
    bias = torch.randn(N, generator=g).to(dev)
    y = A.double() @ W.double().t() + bias.double()
    R, ldr, period = None, 0, 0
    if c["res"] is not None:
        period = 0 if c["res"] == "full" else int(c["res"])
        assert period == 0 or M % period != 0
        ldr = N + 8
        R = torch.randn(period or M, ldr, generator=g).to(dev, dt)[:, 4 if c["ldr"] == "off4" else 0:]
        Rr = R[:, :N].double()
        y = y + (Rr.repeat(M // period + 1, 1)[:M] if period else Rr)
    if c["relu"]:
        y = torch.relu(y)
    ldc = {"pad": N + 8, "off4": N + 8, "odd4": N + 4, "lo": 2 * N, "hi": 2 * N}[c["ldc"]]
    c0 = {"hi": N, "off4": 4}.get(c["ldc"], 0)
    buf = torch.full((M + GUARD, ldc), float("nan"), dtype=torch.float16 if c["f16"] else dt, device=dev)
    C = buf[:, c0:]
    rc = L.spe_debug_gemm(None, _lib.SPE_DTYPE_BF16, 0, p(A), K, None, 0, 1, 0, 0, 0, 1, 1, 1, 0, p(W), K, M, N, K,
                          p(bias), p(R), ldr, c["relu"], p(C), ldc, 0, 0, 0, period, None, None, c["f16"])
    torch.cuda.synchronize()
    path = L.spe_debug_gemm_path()
    got = buf[:M, c0:c0 + N]
    written = torch.zeros_like(buf, dtype=torch.bool)
    written[:M, c0:c0 + N] = True
    scale = max(1.0, y.abs().max().item())
    return dict(rc=rc, path=path, M=M, err=(got.double() - y).abs().max().item(), bound=TOL_BF16 * scale,
                unwritten=int(torch.isnan(got).sum().item()), strays=int((~torch.isnan(buf[~written])).sum().item()),
                sha=hashlib.sha256(buf.cpu().view(torch.int16).numpy().tobytes()).hexdigest())


def _child(out_path):
    import torch
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {name: _run_case(name, c, dev, cus) for name, c in CASES.items()}
    res["odd4"] = _run_case("odd4", ODD4, dev, cus)
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def both_forms(gpu_device, tmp_path_factory):
    """{knob: {case: result}} for SPE_SGEMM_ROWS = "1" (16-byte pieces) and "0" (8-byte pieces)."""
    from conftest import ORACLE, PKG
    d = tmp_path_factory.mktemp("sgemm_rows")
    procs = {}
    for knob in ("1", "0"):
        env = dict(os.environ, SPE_SGEMM_ROWS=knob, PYTHONPATH=os.pathsep.join([PKG, ORACLE, os.environ.get("PYTHONPATH", "")]))
        procs[knob] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / f"rows{knob}.json")], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for knob, pr in procs.items():
        log, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, f"SPE_SGEMM_ROWS={knob} child:\n{log}"
        with open(d / f"rows{knob}.json") as f:
            out[knob] = json.load(f)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows16_equals_rows8_and_fp64(both_forms, name):
    r16, r8 = both_forms["1"][name], both_forms["0"][name]
    for form, r in (("16-byte", r16), ("8-byte", r8)):
        print(f"{name} M = {r['M']} {form}: rc {r['rc']} path {r['path']} max|d| = {r['err']:.3e} bound {r['bound']:.3e} "
              f"unwritten {r['unwritten']} strays {r['strays']}")
        assert r["rc"] == 0
        assert r["path"] == 2, "expected the streaming kernel"
        assert r["unwritten"] == 0, "output elements left as they were"
        assert r["strays"] == 0, "guard rows, the columns between the rows or the buffer's other half were written"
        assert r["err"] <= r["bound"], (r["err"], r["bound"])
    assert r16["M"] == r8["M"] and r16["M"] % 16 == 5
    assert r16["sha"] == r8["sha"], "the 16-byte form's output differs from the 8-byte form's"


def test_row_stride_of_half_a_piece_is_turned_away_under_both_knobs(both_forms):
    r16, r8 = both_forms["1"]["odd4"], both_forms["0"]["odd4"]
    print(f"ldc % 8 == 4: 16-byte rc {r16['rc']}, 8-byte rc {r8['rc']}")
    for r in (r16, r8):
        assert r["rc"] != 0 and r["strays"] == 0 and r["unwritten"] == r["M"] * ODD4["N"]
    assert r16["rc"] == r8["rc"] and r16["sha"] == r8["sha"]


if __name__ == "__main__":
    _child(sys.argv[1])
