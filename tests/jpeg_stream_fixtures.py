"""The hand-built JPEG files of tests/test_jpeg_streams_ref.py (CPU: each file is what it claims to
be) and tests/test_gpu_jpeg_streams.py (the device decoder on them).  Everything is generated from
seeds with tests/jpeg_stream_ref.py; a case is a dict with name, data (the file), H, W, and for valid
files the coefficients and quantisation table that were written."""
import functools

import numpy as np

import jpeg_stream_ref as J

SUBBITS = 2048          # the kernel's subsequence length in bits (csrc/jpeg.hip SUBBITS)

Q_RAMP = 2 + np.arange(64) // 4
Q_ONE = np.ones(64, np.int64)

# every code 8 bits long; code 0x00 is DC category 8 in the one table and (run 2, size 8) in the
# other, so a symbol is a code byte and a value byte whichever table reads it
DC8 = ([0] * 7 + [12] + [0] * 8, [8, 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11])
AC8 = ([0] * 7 + [162] + [0] * 8, [0x28] + [s for s in J.AC_SYMBOLS if s != 0x28])
# one DC code per length 1..12
DC_LADDER = ([1] * 12 + [0] * 4, list(range(12)))
# frequent symbols on 10..16-bit codes: an unused 1-bit code first / the standard order reversed
DC_LONG = ([1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 1, 1], [12] + list(range(12)))
AC_LONG = (J.STD_AC[0], J.STD_AC[1][::-1])
# EOB on the code 00 next to the standard DC table's 00 for category 0
AC_EOB0 = (J.STD_AC[0], [0x00] + [s for s in J.STD_AC[1] if s != 0x00])


def ac_permuted(seed):
    return (J.STD_AC[0], [int(s) for s in np.random.default_rng(seed).permutation(J.STD_AC[1])])


def case(name, data, H, W, coefs=None, qt=None, **kw):
    return dict(name=name, data=data, H=H, W=W, coefs=coefs, qt=qt, **kw)


def base_coefs(nb, seed, nac=5, amp=12):
    """Positive DC (every restart head's difference is large and of one sign, so a missed or a
    misplaced predictor reset changes pixels) and a few small AC terms among the first 20."""
    rng = np.random.default_rng(seed)
    c = np.zeros((nb, 64), np.int64)
    c[:, 0] = rng.integers(40, 101, nb)
    for b in range(nb):
        z = rng.choice(np.arange(1, 20), nac, replace=False)
        c[b, J.ZZ[z]] = rng.integers(-amp, amp + 1, nac)
    c[:, J.ZZ[3]] = rng.integers(-1, 2, nb)
    return c


def special_blocks(c, seed):
    """Block 5: all 63 AC terms non-zero (no EOB).  Block 6: ZRL, ZRL, ZRL, run 14 to index 63."""
    rng = np.random.default_rng(seed)
    c = c.copy()
    c[5, 1:] = rng.integers(1, 4, 63) * rng.choice([-1, 1], 63)
    c[6, 1:] = 0
    c[6, 63] = -3
    return c


def nblocks(H, W):
    return ((H + 7) // 8) * ((W + 7) // 8)


# ------------------------------------------------------------------------------ headers
@functools.lru_cache(None)
def header_variants():
    H, W = 48, 64
    c = base_coefs(48, 1)
    c[7, 63] = 1
    q16 = Q_RAMP.copy()
    q16[J.ZZ[3]] = 600
    q16[63] = 1000
    evil = bytes([0xFF, 0xD0, 0xFF, 0x00, 0xFF, 0xD9])
    decoy = (DC_LADDER, ac_permuted(9))
    knobs = [
        ("plain", {}),
        ("restart5", dict(restart=5)),
        ("pad_zeros", dict(restart=5, pad_ones=False)),
        ("fill_before_markers", dict(restart=4, fill_before_marker=3)),
        ("after_eoi", dict(trailer=evil + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x12\x34\xff\xd9")),
        ("comp_id_0", dict(comp_id=0)),
        ("comp_id_200", dict(comp_id=200)),
        ("sampling_22", dict(sampling=0x22)),
        ("sampling_14", dict(sampling=0x14)),
        ("qt_id_3", dict(qt_id=3)),
        ("qt_16bit", dict(qt_bits=16, qt=q16)),
        ("slots_1_1", dict(dc_slot=1, ac_slot=1)),
        ("slots_2_3", dict(dc_slot=2, ac_slot=3)),
        ("slots_3_2", dict(dc_slot=3, ac_slot=2)),
        ("sof1", dict(sof=0xC1)),
        ("dht_joint", dict(dht_layout="joint")),
        ("dht_decoy", dict(dht_layout="decoy", decoy=decoy)),
        ("com_with_markers", dict(extra_segments=((0xFE, evil),))),
        ("appn", dict(extra_segments=((0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0"), (0xE1, evil * 7 + b"\xff\xda\xff\xc4"),
                                      (0xEF, b"")))),
        ("header_fill", dict(header_fill=2)),
        ("dri_zero", dict(dri_zero=True)),
        ("dri_beyond_blocks", dict(restart=1000)),
        ("all_at_once", dict(restart=7, pad_ones=False, fill_before_marker=2, trailer=evil, comp_id=77, sampling=0x22,
                             qt_id=2, qt_bits=16, qt=q16, dc_slot=3, ac_slot=1, sof=0xC1, dht_layout="decoy",
                             decoy=decoy, extra_segments=((0xFE, evil), (0xE5, evil * 3)), header_fill=3)),
    ]
    out = []
    for name, kw in knobs:
        kw = dict(kw)
        qt = kw.pop("qt", Q_RAMP)
        out.append(case(name, J.write_jpeg(c, H, W, qt, J.STD_DC, J.STD_AC, **kw), H, W, c, qt))
    return out


# ------------------------------------------------------------------------------ table shapes
@functools.lru_cache(None)
def huffman_table_shapes():
    H, W = 48, 64
    rng = np.random.default_rng(2)
    c = special_blocks(base_coefs(48, 2), 2)
    out = [case("long_codes", J.write_jpeg(c, H, W, Q_RAMP, DC_LONG, AC_LONG), H, W, c, Q_RAMP, dc=DC_LONG, ac=AC_LONG)]
    # DC differences of every category 0..11 on the one-code-per-length table
    d = np.concatenate([[0, 1, -2, 4, -8, 16, -32, 64, -128, 256, -512, 1024, -1500], np.zeros(35, np.int64)])
    lad = c.copy()
    lad[:, 0] = np.cumsum(d)
    lad[13:, 0] += rng.integers(-1000, 1001, 35)
    out.append(case("dc_ladder", J.write_jpeg(lad, H, W, Q_ONE, DC_LADDER, J.STD_AC, restart=16), H, W, lad, Q_ONE,
                    dc=DC_LADDER, ac=J.STD_AC))
    perm = ac_permuted(3)
    out.append(case("ac_permuted", J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, perm), H, W, c, Q_RAMP, dc=J.STD_DC, ac=perm))
    big = np.zeros((48, 64), np.int64)
    big[:, 0] = 1000 * (-1) ** np.arange(48)                      # differences of +-2000: category 11
    big[np.arange(48), rng.integers(1, 64, 48)] = rng.integers(512, 1024, 48) * rng.choice([-1, 1], 48)
    out.append(case("dc11_ac10", J.write_jpeg(big, H, W, Q_ONE, J.STD_DC, J.STD_AC), H, W, big, Q_ONE,
                    dc=J.STD_DC, ac=J.STD_AC))
    out.append(case("dc11_ac10_long", J.write_jpeg(big, H, W, Q_ONE, DC_LONG, AC_LONG, restart=9), H, W, big, Q_ONE,
                    dc=DC_LONG, ac=AC_LONG))
    z = np.zeros((48, 64), np.int64)
    out.append(case("all_eob", J.write_jpeg(z, H, W, Q_RAMP, J.STD_DC, J.STD_AC), H, W, z, Q_RAMP, dc=J.STD_DC, ac=J.STD_AC))
    return out


# ------------------------------------------------------------------------------ unstuffing
def _byte_coef(v):
    """The size-8 coefficient whose value bits are the byte v."""
    return v if v >= 128 else v - 255


@functools.lru_cache(None)
def unstuffing():
    """264x264, restart interval 48.  Every symbol is a code byte (never FF) and a value byte, eight
    symbols per block and no EOB, so the file offset of every byte is known while the values are
    chosen: value bytes are FF (coefficient +255) more often than not, one FF is steered to offset
    16383 of the entropy-coded data, and every segment ends on an FF."""
    H = W = 264
    nb, R, target = 1089, 48, 16383
    rng = np.random.default_rng(5)
    c = np.zeros((nb, 64), np.int64)
    o, pred, placed = 0, 0, False
    for b in range(nb):
        if b and b % R == 0:
            o, pred = o + 2, 0
        # seven runs that end on index 63
        cuts = np.sort(rng.choice(np.arange(1, 63), 6, replace=False))
        steps = np.diff(np.concatenate([[0], cuts, [63]]))
        while steps.max() > 16:
            cuts = np.sort(rng.choice(np.arange(1, 63), 6, replace=False))
            steps = np.diff(np.concatenate([[0], cuts, [63]]))
        idx = np.cumsum(steps)
        for j in range(8):
            last = j == 7 and ((b + 1) % R == 0 or b == nb - 1)
            d = target - (o + 1)
            if last or d == 0:
                ff = True
                placed |= d == 0
            elif d in (2, 4):
                ff = False
            elif d == 3:
                ff = True
            elif j == 0:
                ff = False
            else:
                ff = rng.random() < 0.6
            if ff:
                v = 255
            elif j == 0:
                v = int(rng.integers(128, 255)) if pred < 0 else int(rng.integers(0, 128))
            else:
                v = int(rng.integers(0, 255))
            if j == 0:
                pred += _byte_coef(v)
                c[b, 0] = pred
            else:
                c[b, J.ZZ[idx[j - 1]]] = _byte_coef(v)
            o += 3 if ff else 2
    assert placed
    return case("unstuffing", J.write_jpeg(c, H, W, Q_ONE, DC8, AC8, restart=R), H, W, c, Q_ONE, restart=R)


def short_segment_behind_fill(n_fill=6):
    """A file whose third restart segment is one block short and is followed by fill FFs: corrupt.
    Fill bytes taken for data would read as a DC and an AC symbol and complete the missing block."""
    c = base_coefs(48, 4)
    segs = J.encode_scan(c, J.STD_DC, J.STD_AC, 4)
    segs[2] = J.encode_scan(c[8:11], J.STD_DC, J.STD_AC, 0)[0]
    return case("short_segment_behind_fill",
                J.write_jpeg(None, 48, 64, Q_RAMP, J.STD_DC, J.STD_AC, restart=4, segments=segs,
                             fill_before_marker=n_fill), 48, 64)


# ------------------------------------------------------------------------------ restart layouts
RESTARTS = (1, 7, 1000, 1024, 1088, 1089, 5000)


@functools.lru_cache(None)
def restart_layouts():
    H = W = 264
    c = base_coefs(1089, 6, nac=3)
    out = [case("R%d" % r, J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, J.STD_AC, restart=r), H, W, c, Q_RAMP, restart=r)
           for r in RESTARTS]
    out.append(case("dri_zero", J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, J.STD_AC, dri_zero=True), H, W, c, Q_RAMP, restart=0))
    return out


# ------------------------------------------------------------------------------ repair
def shifted_blocks(nb, seed):
    """Blocks of 22 symbols of 16 bits each (DC category 8, then 21 times run 2 / size 8, the last
    on index 63): 352 bits, no divisor of 2048, and every block alike -- a decoder that starts
    inside a block in block-start state keeps its offset in the coefficient index for good.  Of eight
    sign patterns per block the one with the smallest IDCT swing is kept."""
    rng = np.random.default_rng(seed)
    c = np.zeros((nb, 64), np.int64)
    pos = J.ZZ[np.arange(3, 64, 3)]
    pred = 0
    for b in range(nb):
        pred += int(rng.integers(128, 256)) * (-1 if pred > 0 else 1)
        cand = np.zeros((8, 64), np.int64)
        cand[:, 0] = pred
        cand[:, pos] = rng.integers(128, 256, (8, 21)) * rng.choice([-1, 1], (8, 21))
        swing = np.abs(J.idct_islow(cand, Q_ONE, preclamp=True)).reshape(8, -1).max(1)
        c[b] = cand[np.argmin(swing)]
    return c


@functools.lru_cache(None)
def repair():
    """alone / two ordinary files for a batch / the restart form: intervals of 96 blocks, the second
    one of ordinary blocks."""
    H = W = 128
    sh = shifted_blocks(256, 7)
    mixed = sh.copy()
    mixed[96:192] = base_coefs(96, 8)
    mixed[192:] = shifted_blocks(64, 12)
    ordinary = [base_coefs(256, 9), base_coefs(256, 10)]
    return dict(
        alone=case("shifted", J.write_jpeg(sh, H, W, Q_ONE, DC8, AC8), H, W, sh, Q_ONE, restart=0),
        restart=case("shifted_R96", J.write_jpeg(mixed, H, W, Q_ONE, DC8, AC8, restart=96), H, W, mixed, Q_ONE, restart=96),
        ordinary=[case("ordinary0", J.write_jpeg(ordinary[0], H, W, Q_RAMP, J.STD_DC, J.STD_AC), H, W, ordinary[0], Q_RAMP),
                  case("ordinary1", J.write_jpeg(ordinary[1], H, W, Q_RAMP, J.STD_DC, J.STD_AC, restart=11), H, W,
                       ordinary[1], Q_RAMP)])


# ------------------------------------------------------------------------------ zero pad bits
ZERO_PAD_BITS = 4        # DC category 0 (00) + EOB (00)


@functools.lru_cache(None)
def zero_pad():
    H, W = 48, 64
    c = base_coefs(48, 11)
    return [case("zero_pad_eob0", J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, AC_EOB0, restart=4, pad_ones=False), H, W, c,
                 Q_RAMP, restart=4),
            case("zero_pad_std", J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, J.STD_AC, restart=4, pad_ones=False), H, W, c,
                 Q_RAMP, restart=4)]


# ------------------------------------------------------------------------------ small and odd
SMALL_SIZES = ((1, 1), (8, 8), (7, 9), (1, 64), (64, 1), (9, 16))


@functools.lru_cache(None)
def small_and_odd():
    out = []
    for i, (H, W) in enumerate(SMALL_SIZES):
        c = base_coefs(nblocks(H, W), 20 + i)
        r = 3 if nblocks(H, W) > 4 else 0
        out.append(case("%dx%d" % (H, W), J.write_jpeg(c, H, W, Q_RAMP, J.STD_DC, J.STD_AC, restart=r), H, W, c, Q_RAMP))
    return out


# ------------------------------------------------------------------------------ IDCT extremes
def _patterns():
    yy, xx = np.mgrid[0:8, 0:8]
    p = []
    for n in (1, 2, 4):
        p += [((yy // n + xx // n) % 2) * 255, ((yy // n) % 2) * 255, ((xx // n) % 2) * 255]
    for y, x in ((0, 0), (3, 4), (7, 7), (0, 7), (5, 1)):
        hot = np.zeros((8, 8), np.int64)
        hot[y, x] = 255
        p += [hot, 255 - hot]
    p += [255 - q for q in p[:9]]
    return np.stack(p)


DC_WRAP_Q = 16
DC_WRAP = (1000, -1000, 2000, -2000, 257, -257, 256, -256, 313, -313, 2047, -2047, 769, -769, 64, -64)


@functools.lru_cache(None)
def idct_extremes():
    H, W = 48, 64
    pat = _patterns()
    pix = pat[np.arange(48) % len(pat)]
    F = J.fdct(pix)
    q_coarse = np.full(64, 255, np.int64)
    q_coarse[0] = 8
    out = []
    for name, q in (("coarse", q_coarse), ("q1", Q_ONE)):
        c = np.clip(np.rint(F.reshape(48, 64) / q), -1023, 1023).astype(np.int64)
        out.append(case("patterns_" + name, J.write_jpeg(c, H, W, q, J.STD_DC, J.STD_AC, restart=1), H, W, c, q))
    c = np.zeros((48, 64), np.int64)
    c[:, 0] = np.resize(DC_WRAP, 48)
    q = Q_ONE.copy()
    q[0] = DC_WRAP_Q
    out.append(case("dc_wrap", J.write_jpeg(c, H, W, q, J.STD_DC, J.STD_AC, restart=1), H, W, c, q, wrap=True))
    return out


def dc_wrap_simd_agrees(c):
    """Per block: does a 16-bit SIMD islow (libjpeg-turbo: int16 workspace after pass 1, saturating
    pack at the end) give the same pixel as jidctint.c's table?  Where (dc*q + 4) >> 3, taken modulo
    2048 into [-1024, 1023], lands in [-128, 127] both wrap to the same in-range value; elsewhere
    the SIMD code saturates where the table wraps, so Pillow's pixel depends on how it was built."""
    v = (c["coefs"][:, 0] * int(c["qt"][0]) + 4) >> 3
    w = (v + 1024) % 2048 - 1024
    return (w >= -128) & (w <= 127)


def dc_wrap_closed_form(c):
    """range_limit(((dc*q + 4) >> 3) & 1023) for every block of the DC-only case, as a frame."""
    v = (c["coefs"][:, 0] * int(c["qt"][0]) + 4) >> 3
    px = J.RANGE_LIMIT[v & 1023].astype(np.uint8)
    return J.assemble(np.repeat(px, 64).reshape(-1, 8, 8), c["H"], c["W"])


# ------------------------------------------------------------------------------ malformed
@functools.lru_cache(None)
def malformed():
    """(case, expected status) in batch order: every bad file between good neighbours."""
    H, W = 48, 64
    c = base_coefs(48, 30)
    std = (J.STD_DC, J.STD_AC)

    def w(name, status, **kw):
        dc, ac = kw.pop("tables", std)
        return case(name, J.write_jpeg(c, H, W, Q_RAMP, dc, ac, **kw), H, W), status

    one = J.encode_scan(c, *std, 1)
    r4 = J.encode_scan(c, *std, 4)
    short = list(r4)
    short[5] = J.encode_scan(c[20:23], *std, 0)[0]
    full_dc = ([1] * 11 + [2] + [0] * 4, list(range(13)))           # the second 12-bit code is all ones
    sof = bytes([8, 0, H, 0, W])
    bad = [
        w("rst_as_many_as_blocks", 2, restart=1, segments=one + one[-1:]),
        w("rst_more_than_blocks", 2, restart=1, segments=one + one[-3:]),
        w("adjacent_rst", 2, restart=4, segments=r4[:5] + [b""] + r4[6:]),
        w("undefined_ac_slot", 2, override=dict(sos=bytes([1, 1, 0x01, 0, 63, 0]))),
        w("undefined_dc_slot", 2, override=dict(sos=bytes([1, 1, 0x20, 0, 63, 0]))),
        w("undefined_qt_slot", 2, override=dict(sof=sof + bytes([1, 1, 0x11, 2]))),
        w("all_ones_code", 2, tables=(DC_LADDER, J.STD_AC), override=dict(dht=[J.dht_payload(0, 0, full_dc),
                                                                             J.dht_payload(1, 0, J.STD_AC)])),
        w("dht_counts_overrun", 2, override=dict(dht=[J.dht_payload(0, 0, J.STD_DC) + J.dht_payload(1, 0, J.STD_AC)[:-9]])),
        w("segment_one_block_short", 2, restart=4, segments=short),
        w("two_components", 1, override=dict(sof=sof + bytes([2, 1, 0x11, 0, 2, 0x11, 0]))),
        w("twelve_bit", 1, override=dict(sof=bytes([12]) + sof[1:] + bytes([1, 1, 0x11, 0]))),
        w("spectral_selection", 1, override=dict(sos=bytes([1, 1, 0x00, 0, 5, 0]))),
        w("successive_approximation", 1, override=dict(sos=bytes([1, 1, 0x00, 0, 63, 1]))),
        w("ss_nonzero", 1, override=dict(sos=bytes([1, 1, 0x00, 1, 63, 0]))),
    ]
    good = [base_coefs(48, 40 + i) for i in range(len(bad) + 1)]
    out = []
    for i, g in enumerate(good):
        out.append((case("good%d" % i, J.write_jpeg(g, H, W, Q_RAMP, *std, restart=(0, 5, 1)[i % 3]), H, W, g, Q_RAMP), 0))
        if i < len(bad):
            out.append(bad[i])
    return out
