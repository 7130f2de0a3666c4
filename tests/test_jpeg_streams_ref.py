"""The hand-built JPEG files of tests/jpeg_stream_fixtures.py are what they claim to be (CPU only).

tests/test_gpu_jpeg_streams.py compares the device decoder with Pillow on these files.  Here, for
every valid file: Pillow decodes it without an exception or a warning, the sequential reference
decoder returns the coefficients that were written, and idct_islow (jidctint.c in int64) of those
coefficients equals Pillow's pixels exactly -- so Pillow on the machine at hand is the decoder the
kernel claims to match.  Then the conditions that make a file exercise its target are asserted, so
that a fixture which stops reaching the kernel path it was built for fails here.
"""
import io
import warnings
from collections import Counter

import numpy as np
import pytest
from PIL import Image

import jpeg_stream_fixtures as F
import jpeg_stream_ref as J


def _pillow(data):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.mode == "L"
        return np.asarray(im)


def _valid_cases():
    r = F.repair()
    fams = [("headers", F.header_variants()), ("tables", F.huffman_table_shapes()), ("unstuffing", [F.unstuffing()]),
            ("restarts", F.restart_layouts()), ("repair", [r["alone"], r["restart"]] + r["ordinary"]),
            ("zero_pad", F.zero_pad()), ("small", F.small_and_odd()), ("idct", F.idct_extremes()),
            ("malformed_neighbours", [c for c, st in F.malformed() if st == 0])]
    return [(fam + "-" + c["name"], c) for fam, cs in fams for c in cs]


VALID = _valid_cases()


@pytest.mark.parametrize("c", [c for _, c in VALID], ids=[n for n, _ in VALID])
def test_fixture_is_the_file_it_claims_to_be(c):
    px = _pillow(c["data"])
    assert px.shape == (c["H"], c["W"])
    d = J.decode(c["data"])
    assert np.array_equal(d["coefs"], c["coefs"])
    assert np.array_equal(d["qt"], c["qt"])
    # the bound the kernel's comment states for its 32-bit arithmetic
    assert np.abs(c["coefs"] * c["qt"]).max() < 1 << 15
    mine = J.assemble(J.idct_islow(c["coefs"], c["qt"]), c["H"], c["W"])
    if c.get("wrap"):
        # DC-only blocks pushed past the range-limit table's first half: jidctint.c's table wraps.
        # Pillow agrees wherever a 16-bit SIMD islow provably computes the same (see the predicate)
        assert np.array_equal(mine, F.dc_wrap_closed_form(c))
        same = F.dc_wrap_simd_agrees(c)
        pre = J.idct_islow(c["coefs"], c["qt"], preclamp=True).reshape(-1, 64)
        assert (same & (np.abs(pre[:, 0]) > 512)).sum() >= 12
        keep = J.assemble(np.repeat(same, 64).reshape(-1, 8, 8), c["H"], c["W"])
        assert np.array_equal(mine[keep], px[keep])
        return
    pre = J.idct_islow(c["coefs"], c["qt"], preclamp=True)
    assert -512 <= pre.min() and pre.max() <= 511, (pre.min(), pre.max())
    assert np.array_equal(mine, px)


def test_idct_extremes_overshoot():
    """The coarse patterns leave 0..255 by a wide margin on both sides (the clamp halves of the
    range-limit table are used), inside the range asserted above."""
    c = F.idct_extremes()[0]
    pre = J.idct_islow(c["coefs"], c["qt"], preclamp=True)
    assert pre.min() < -128 - 40 and pre.max() > 127 + 40


def _symbols(c):
    """(is_dc, symbol) of every symbol of every block, blocks without restarts in between."""
    out, pred = [], 0
    for blk in c["coefs"]:
        zz = blk[J.ZZ]
        out.append([(d, s) for d, s, _, _ in J.block_symbols(zz, pred)])
        pred = int(zz[0])
    return out


def test_header_variants_differ():
    files = [c["data"] for c in F.header_variants()]
    assert len(set(files)) == len(files)
    evil = bytes([0xFF, 0xD0, 0xFF, 0x00, 0xFF, 0xD9])
    by = {c["name"]: c["data"] for c in F.header_variants()}
    assert by["com_with_markers"][2:4] == b"\xff\xfe" and evil in by["com_with_markers"][:16]
    assert by["after_eoi"].index(b"\xff\xd9") < len(by["after_eoi"]) - 8


def test_table_shape_fixtures_reach_their_symbols():
    by = {c["name"]: c for c in F.huffman_table_shapes()}
    # long codes: every DC symbol and the five most frequent AC symbols sit on 10..16-bit codes, past
    # the kernel's 9-bit lookup
    c = by["long_codes"]
    syms = [s for blk in _symbols(c) for s in blk]
    dcl, acl = J.canonical_codes(c["dc"]), J.canonical_codes(c["ac"])
    assert all(dcl[s][1] >= 10 for d, s in syms if d)
    top = [s for s, _ in Counter(s for d, s in syms if not d).most_common(5)]
    assert all(acl[s][1] >= 10 for s in top)
    # one code per length: differences of all twelve categories
    c = by["dc_ladder"]
    assert sorted(set(l for _, l in J.canonical_codes(c["dc"]).values())) == list(range(1, 13))
    d = np.diff(np.concatenate([[0], c["coefs"][:16, 0]]))
    assert {int(abs(x)).bit_length() for x in d} == set(range(12))
    # the permutation moved the symbols
    assert by["ac_permuted"]["ac"][1] != J.STD_AC[1] and sorted(by["ac_permuted"]["ac"][1]) == J.AC_SYMBOLS
    for name in ("dc11_ac10", "dc11_ac10_long"):
        syms = [s for blk in _symbols(by[name]) for s in blk]
        assert any(d and s == 11 for d, s in syms) and any(not d and (s & 15) == 10 for d, s in syms)
    for name in ("long_codes", "ac_permuted"):
        blocks = _symbols(by[name])
        assert len(blocks[5]) == 64 and all(s & 15 for _, s in blocks[5][1:])               # no EOB, no ZRL
        assert [s for _, s in blocks[6][1:]] == [0xF0, 0xF0, 0xF0, 0xE2]
    assert J.unstuffed_length(by["all_eob"]["data"]) * 8 <= F.SUBBITS


def test_unstuffing_fixture_places_its_edges():
    c = F.unstuffing()
    d = J.decode(c["data"])
    data, ecs = c["data"], d["ecs_off"]
    assert d["end"] > 16384 + 1024                          # well into the second 16 KiB tile
    assert len(d["ff00"]) > 4000                            # FF is dense
    assert any(o % 16 == 15 for o in d["ff00"])             # split across a thread's 16-byte span
    assert 16383 in d["ff00"]                               # split across the 16384-byte tile
    assert data[ecs + 16383:ecs + 16385] == b"\xff\x00"
    # FF 00 straight before an RSTn, and before EOI
    assert any(data[ecs + o + 2] == 0xFF and 0xD0 <= data[ecs + o + 3] <= 0xD7 for o in d["ff00"])
    assert data[ecs + d["end"] - 2:ecs + d["end"] + 2] == b"\xff\x00\xff\xd9"
    assert all(s[-1] == 0xFF for s in d["segments"])
    assert any(len(s) % 256 == 0 for s in d["segments"])
    assert sum(len(s) for s in d["segments"]) == J.unstuffed_length(data)


def test_restart_fixtures_have_their_segments():
    for c in F.restart_layouts():
        R = c["restart"]
        n = J.segment_lengths(c["data"])
        assert len(n) == (-(-1089 // R) if 0 < R < 1089 else 1)
        assert J.parse(c["data"])["restart"] == R
    assert len(J.segment_lengths(F.restart_layouts()[0]["data"])) == 1089 > 1024
    # a missed predictor reset adds the previous block's DC: at least 40 * 2 / 8 = 10 grey levels
    c = F.restart_layouts()[0]
    assert c["coefs"][:, 0].min() >= 40 and c["qt"][0] == 2


def _longest_run_of_unrejoined_starts(st, trace):
    """Longest run of consecutive k for which a decoder started at bit k * SUBBITS in block-start
    state does not reach a state of the true decode before the end of subsequence k + 3."""
    true = set(trace) | {(0, 0)}
    best = run = 0
    for k in range(1, st.nbits // F.SUBBITS - 3):
        start = (k * F.SUBBITS, 0)
        tr, _ = J.walk(st, *start, end=(k + 4) * F.SUBBITS)
        ok = start not in true and not any(s in true for s in tr)
        run = run + 1 if ok else 0
        best = max(best, run)
    return best


def test_repair_fixture_stays_desynchronised():
    r = F.repair()
    for c, seg in ((r["alone"], 0), (r["restart"], 0)):
        d = J.decode(c["data"])
        assert _longest_run_of_unrejoined_starts(d["streams"][seg], d["traces"][seg]) >= 8
    # the restart form's second interval is of the ordinary kind: starts inside it rejoin at once
    d = J.decode(r["restart"]["data"])
    assert len(d["segments"]) == 3
    assert _longest_run_of_unrejoined_starts(d["streams"][1], d["traces"][1]) == 0
    # and an ordinary file never comes near the condition
    d = J.decode(r["ordinary"][0]["data"])
    assert _longest_run_of_unrejoined_starts(d["streams"][0], d["traces"][0]) == 0


def test_zero_pad_fixture_counts_a_block_too_many():
    c = F.zero_pad()[0]
    d = J.decode(c["data"])
    assert J.canonical_codes(d["dc_table"])[0] == (0, 2) and J.canonical_codes(d["ac_table"])[0] == (0, 2)
    assert F.ZERO_PAD_BITS <= 7
    hit = 0
    for st, tr, seg in zip(d["streams"], d["traces"], d["segments"]):
        pad = st.nbits - tr[-1][0]
        assert int.from_bytes(seg, "big") & ((1 << pad) - 1) == 0       # pad bits are zeros
        _, counted = J.walk(st)                                          # count-only: to the segment's end
        if pad >= F.ZERO_PAD_BITS:                                       # the pad bits alone are a block
            assert counted >= 4 + 1
        hit += pad >= F.ZERO_PAD_BITS
    assert hit >= 1
    # with the ordinary tables the same pad bits complete nothing
    d = J.decode(F.zero_pad()[1]["data"])
    assert all(J.walk(st)[1] == 4 for st in d["streams"])
