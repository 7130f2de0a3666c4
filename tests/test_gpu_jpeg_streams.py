"""The device JPEG decoder (csrc/jpeg.hip) on hand-built streams Pillow cannot write.

The files come from tests/jpeg_stream_fixtures.py; tests/test_jpeg_streams_ref.py shows on the CPU
that each is valid, that Pillow's pixels equal jidctint.c's for it, and that it reaches the kernel
path it was built for (the repair path, the long-code walk, the second passes of the chunked loops,
the unstuffing edges).  Here every file must decode with status 0 to exactly Pillow's frame.  The
decoder's workspace is filled with 0xA5 before each decode, so a coefficient or a record that is
read without having been written shows.
"""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_stream_fixtures as F

pytestmark = pytest.mark.gpu


def _pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("L"))


def _decode(dev, files, H, W):
    from spe.datasets import JpegDecoder
    dec = JpegDecoder(H, W, max_bytes=max(len(f) for f in files))
    dec.workspace(len(files), dev).fill_(0xA5)
    o = dec(*JpegDecoder.pack(files, dev))
    torch.cuda.synchronize()
    return o["status"].cpu().numpy(), o["frames"].cpu().numpy()


def _check_exact(dev, cases, expected=_pillow):
    H, W = cases[0]["H"], cases[0]["W"]
    st, got = _decode(dev, [c["data"] for c in cases], H, W)
    assert st.tolist() == [0] * len(cases), dict(zip([c["name"] for c in cases], st.tolist()))
    for i, c in enumerate(cases):
        ref = expected(c["data"]) if expected is _pillow else expected(c)
        assert np.array_equal(got[i], ref), (c["name"], int((got[i] != ref).sum()))


def test_header_variants(gpu_device):
    _check_exact(gpu_device, F.header_variants())


def test_huffman_table_shapes(gpu_device):
    _check_exact(gpu_device, F.huffman_table_shapes())


def test_unstuffing_edges(gpu_device):
    _check_exact(gpu_device, [F.unstuffing()])
    # fill FFs before a marker are no data: behind a segment that is one block short they must not
    # complete it
    c = F.short_segment_behind_fill()
    st, got = _decode(gpu_device, [c["data"]], c["H"], c["W"])
    assert st.tolist() == [2] and (got == 0).all()


def test_restart_layouts(gpu_device):
    _check_exact(gpu_device, F.restart_layouts())


def test_desynchronised_stream_is_repaired(gpu_device):
    r = F.repair()
    _check_exact(gpu_device, [r["alone"]])
    _check_exact(gpu_device, [r["ordinary"][0], r["alone"], r["ordinary"][1]])
    _check_exact(gpu_device, [r["restart"]])
    _check_exact(gpu_device, [r["ordinary"][1], r["restart"], r["alone"], r["ordinary"][0]])


def test_zero_pad_bits(gpu_device):
    _check_exact(gpu_device, F.zero_pad())


def test_small_and_odd_frames(gpu_device):
    for c in F.small_and_odd():
        _check_exact(gpu_device, [c, c])


def test_idct_extremes(gpu_device):
    pat = [c for c in F.idct_extremes() if not c.get("wrap")]
    wrap = [c for c in F.idct_extremes() if c.get("wrap")]
    _check_exact(gpu_device, pat)
    # past +-512 the expected pixel is jidctint.c's range-limit table at ((dc*q + 4) >> 3) & 1023
    _check_exact(gpu_device, wrap, expected=F.dc_wrap_closed_form)
    st, got = _decode(gpu_device, [c["data"] for c in pat + wrap], 48, 64)
    assert st.tolist() == [0, 0, 0]
    assert np.array_equal(got[2], F.dc_wrap_closed_form(wrap[0])) and np.array_equal(got[0], _pillow(pat[0]["data"]))


def test_malformed_streams_get_a_status(gpu_device):
    cases = F.malformed()
    st, got = _decode(gpu_device, [c["data"] for c, _ in cases], 48, 64)
    assert st.tolist() == [s for _, s in cases], {c["name"]: (int(a), s) for (c, s), a in zip(cases, st) if a != s}
    for i, (c, s) in enumerate(cases):
        if s == 0:
            assert np.array_equal(got[i], _pillow(c["data"])), c["name"]
        else:
            assert (got[i] == 0).all(), c["name"]
