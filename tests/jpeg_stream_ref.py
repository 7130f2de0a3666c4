"""Hand-built baseline-JPEG streams and a plain reference for them (numpy only, nothing from spe).

write_jpeg     quantised coefficient blocks -> a grayscale JPEG file, with a knob for every header
               and entropy-stream shape the device decoder (csrc/jpeg.hip) has to accept
decode         the sequential decoder: file -> coefficient blocks and, per restart segment, the
               (bit position, zig-zag index) state after every symbol
walk           the same state machine started anywhere in a segment (what a speculative decoder of
               the device pipeline sees)
idct_islow     libjpeg's jidctint.c in int64 with its range-limit table (index & 1023)
helpers        unstuffed length, file offsets of the FF 00 pairs, segment lengths

Coefficient blocks are [nblocks, 64] in natural (row-major) order, DC absolute (not differences).
A Huffman table is (bits, huffval): bits[l-1] codes of length l, huffval in code order.
"""
import numpy as np

# zig-zag index -> natural index
ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
               13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
               45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.3 luminance tables
STD_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_AC_HEAD = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22,
            0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33,
            0x62, 0x72, 0x82, 0x09, 0x0A]
_AC_TAIL = [(r << 4) | s for r, s0 in ((1, 6), (2, 5), (3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2),
                                       (10, 2), (11, 2), (12, 2), (13, 2), (14, 1), (15, 1)) for s in range(s0, 11)]
STD_AC = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], _AC_HEAD + _AC_TAIL)
AC_SYMBOLS = sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])
assert len(STD_AC[1]) == 162 and sorted(STD_AC[1]) == AC_SYMBOLS


# ------------------------------------------------------------------------------ Huffman tables
def canonical_codes(table):
    """symbol -> (code, length), codes assigned in order of length (T.81 Annex C)."""
    bits, vals = table
    assert len(bits) == 16 and sum(bits) == len(vals)
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out.setdefault(vals[p], (code, l))
            code += 1
            p += 1
        assert code <= (1 << l), "over-subscribed table"
        code <<= 1
    return out


_LUTS = {}


def _lut16(table):
    """16-bit window -> (length, symbol) lists; length 0 where no code matches."""
    key = (tuple(table[0]), tuple(table[1]))
    if key not in _LUTS:
        _LUTS[key] = _build_lut16(table)
    return _LUTS[key]


def _build_lut16(table):
    bits, vals = table
    ln = np.zeros(1 << 16, np.int64)
    sy = np.zeros(1 << 16, np.int64)
    code, p = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo, hi = code << (16 - l), (code + 1) << (16 - l)
            ln[lo:hi] = l
            sy[lo:hi] = vals[p]
            code += 1
            p += 1
        code <<= 1
    return ln.tolist(), sy.tolist()


# ------------------------------------------------------------------------------ writer
def _size_and_bits(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def block_symbols(zz, pred):
    """One block (zig-zag order, DC absolute) -> [(is_dc, symbol, value bits, size)]."""
    s, v = _size_and_bits(int(zz[0]) - pred)
    out = [(True, s, v, s)]
    run = 0
    for z in range(1, 64):
        c = int(zz[z])
        if c == 0:
            run += 1
            continue
        while run > 15:
            out.append((False, 0xF0, 0, 0))
            run -= 16
        s, v = _size_and_bits(c)
        out.append((False, (run << 4) | s, v, s))
        run = 0
    if run:
        out.append((False, 0x00, 0, 0))
    return out


def encode_scan(coefs, dc_table, ac_table, restart=0, pad_ones=True):
    """Coefficient blocks -> the unstuffed bytes of every restart segment."""
    coefs = np.asarray(coefs).reshape(-1, 64)
    dc, ac = canonical_codes(dc_table), canonical_codes(ac_table)
    nb = len(coefs)
    R = restart if restart > 0 else nb
    segs = []
    for b0 in range(0, nb, R):
        parts, pred = [], 0
        for blk in coefs[b0:b0 + R]:
            zz = blk[ZZ]
            for is_dc, sym, v, s in block_symbols(zz, pred):
                code, l = (dc if is_dc else ac)[sym]
                parts.append(format(code, "0%db" % l))
                if s:
                    parts.append(format(v, "0%db" % s))
            pred = int(zz[0])
        bits = "".join(parts)
        bits += ("1" if pad_ones else "0") * (-len(bits) % 8)
        segs.append(int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b"")
    return segs


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dht_payload(tc, slot, table):
    bits, vals = table
    return bytes([(tc << 4) | slot]) + bytes(bits) + bytes(vals)


def write_jpeg(coefs, H, W, qt, dc_table, ac_table, *, restart=0, pad_ones=True, fill_before_marker=0,
               trailer=b"", comp_id=1, sampling=0x11, qt_id=0, qt_bits=8, dc_slot=0, ac_slot=0, sof=0xC0,
               dht_layout="separate", decoy=None, extra_segments=(), header_fill=0, dri_zero=False,
               segments=None, override=None):
    """A one-component JPEG file.  Knobs: restart interval (blocks), pad-bit polarity, fill FF bytes
    before every RSTn and EOI, bytes after EOI, component id, sampling byte, quantisation-table id
    and precision, Huffman slot ids, SOF0/SOF1, DHT layout ("separate": one segment per table,
    "joint": both in one segment, "decoy": the tables of `decoy` defined in one segment and
    redefined in the next), extra (marker, payload) segments after SOI, fill FFs before every header
    marker, an explicit DRI 0.  `segments` replaces the encoded scan (unstuffed bytes per segment);
    `override` replaces the raw payload of "sof", "sos" or the list of "dht" payloads."""
    ov = override or {}
    qt = np.asarray(qt).reshape(64)
    if segments is None:
        segments = encode_scan(coefs, dc_table, ac_table, restart, pad_ones)
    fill = b"\xff" * header_fill
    out = [b"\xff\xd8"]
    for m, payload in extra_segments:
        out += [fill, segment(m, payload)]
    q = qt[ZZ]
    qb = b"".join(int(x).to_bytes(2, "big") for x in q) if qt_bits == 16 else bytes(int(x) for x in q)
    out += [fill, segment(0xDB, bytes([((qt_bits == 16) << 4) | qt_id]) + qb)]
    sof_p = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([1, comp_id, sampling, qt_id])
    out += [fill, segment(sof, ov.get("sof", sof_p))]
    real = [dht_payload(0, dc_slot, dc_table), dht_payload(1, ac_slot, ac_table)]
    if "dht" in ov:
        dht = ov["dht"]
    elif dht_layout == "separate":
        dht = real
    elif dht_layout == "joint":
        dht = [real[0] + real[1]]
    elif dht_layout == "decoy":
        dht = [dht_payload(0, dc_slot, decoy[0]) + dht_payload(1, ac_slot, decoy[1]), real[0] + real[1]]
    else:
        raise ValueError(dht_layout)
    for p in dht:
        out += [fill, segment(0xC4, p)]
    if restart > 0 or dri_zero:
        out += [fill, segment(0xDD, int(restart).to_bytes(2, "big"))]
    sos_p = bytes([1, comp_id, (dc_slot << 4) | ac_slot, 0, 63, 0])
    out += [fill, segment(0xDA, ov.get("sos", sos_p))]
    mfill = b"\xff" * fill_before_marker
    for i, s in enumerate(segments):
        if i:
            out += [mfill, bytes([0xFF, 0xD0 + (i - 1) % 8])]
        out.append(s.replace(b"\xff", b"\xff\x00"))
    out += [mfill, b"\xff\xd9", trailer]
    return b"".join(out)


# ------------------------------------------------------------------------------ reference decoder
def parse(data):
    """Marker walk up to SOS: frame, quantisation table (natural order), the scan's tables."""
    assert data[:2] == b"\xff\xd8"
    p, qts, huff, out = 2, {}, {}, {"restart": 0}
    while True:
        assert data[p] == 0xFF
        while data[p] == 0xFF:
            p += 1
        m = data[p]
        p += 1
        n = int.from_bytes(data[p:p + 2], "big")
        s = data[p + 2:p + n]
        if m in (0xC0, 0xC1):
            assert s[0] == 8 and s[5] == 1
            out.update(sof=m, H=int.from_bytes(s[1:3], "big"), W=int.from_bytes(s[3:5], "big"), comp_id=s[6],
                       sampling=s[7], tq=s[8])
        elif m == 0xC4:
            q = 0
            while q < len(s):
                bits = list(s[q + 1:q + 17])
                huff[s[q]] = (bits, list(s[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xDB:
            q = 0
            while q < len(s):
                pq, tq = s[q] >> 4, s[q] & 15
                raw = s[q + 1:q + 1 + 64 * (pq + 1)]
                v = np.frombuffer(raw, ">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZZ] = v
                qts[tq] = nat
                q += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            out["restart"] = int.from_bytes(s[:2], "big")
        elif m == 0xDA:
            assert s[0] == 1 and s[1] == out["comp_id"] and tuple(s[3:6]) == (0, 63, 0)
            out.update(dc_table=huff[s[2] >> 4], ac_table=huff[0x10 | (s[2] & 15)], qt=qts[out["tq"]], ecs_off=p + n)
            return out
        p += n


def split_entropy(data, ecs_off):
    """Entropy-coded data -> (unstuffed bytes of every segment, offsets of the FF 00 pairs relative
    to ecs_off, offset of the terminating marker's FF).  FF 00 is a data FF, FF Dn a restart, FF FF a
    fill byte, FF anything-else ends the scan."""
    segs, cur, pairs, i = [], bytearray(), [], ecs_off
    while True:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nx = data[i + 1]
        if nx == 0x00:
            pairs.append(i - ecs_off)
            cur.append(0xFF)
            i += 2
        elif nx == 0xFF:
            i += 1
        elif 0xD0 <= nx <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            segs.append(bytes(cur))
            return segs, pairs, i - ecs_off


def ff00_offsets(data):
    return split_entropy(data, parse(data)["ecs_off"])[1]


def segment_lengths(data):
    return [len(s) for s in split_entropy(data, parse(data)["ecs_off"])[0]]


def unstuffed_length(data):
    return sum(segment_lengths(data))


class Stream:
    """One segment's bits with the two tables: 16-bit windows at every bit position."""

    def __init__(self, seg, dc_table, ac_table):
        bits = np.unpackbits(np.frombuffer(bytes(seg) + bytes(8), np.uint8)).astype(np.int64)
        n = len(seg) * 8
        win = np.zeros(n + 32, np.int64)
        for i in range(16):
            win += bits[i:i + n + 32] << (15 - i)
        self.nbits, self.win = n, win.tolist()
        self.dc, self.ac = _lut16(dc_table), _lut16(ac_table)


def walk(st, p=0, z=0, end=None, max_blocks=None, blocks_out=None):
    """Decode from bit p at zig-zag index z (0 = block start) until p >= end or max_blocks blocks
    are complete.  Returns (trace, blocks): trace holds (p, z) after every symbol, z back at 0 when
    the symbol completed a block.  An invalid code decodes as symbol 0 of length 16 (libjpeg).
    blocks_out, a list, receives each completed block as 64 zig-zag DC-difference/AC values."""
    end = st.nbits if end is None else end
    win, trace, nblk = st.win, [], 0
    cur = [0] * 80
    while p < end and (max_blocks is None or nblk < max_blocks):
        ln, sy = st.dc if z == 0 else st.ac
        w = win[p]
        l, sym = ln[w], sy[w]
        if l == 0:
            l, sym = 16, 0
        p += l
        s = sym & 15
        v = win[p] >> (16 - s) if s else 0
        if s and v < (1 << (s - 1)):
            v += 1 - (1 << s)
        if z == 0:
            cur[0] = v
            p += s
            z = 1
        elif s:
            z += sym >> 4
            cur[z] = v
            z += 1
            p += s
        else:
            z = z + 16 if (sym >> 4) == 15 else 64
        if z >= 64:
            z = 0
            nblk += 1
            if blocks_out is not None:
                blocks_out.append(cur[:64])
            cur = [0] * 80
        trace.append((p, z))
    return trace, nblk


def decode(data):
    """Sequential decode of a valid file: coefficient blocks (natural order, DC absolute), the
    per-segment traces and unstuffed segments, and the header fields of parse()."""
    h = parse(data)
    nb = ((h["H"] + 7) // 8) * ((h["W"] + 7) // 8)
    R = h["restart"] if h["restart"] > 0 else nb
    segs, pairs, end = split_entropy(data, h["ecs_off"])
    assert len(segs) == (nb + R - 1) // R, (len(segs), nb, R)
    coefs = np.zeros((nb, 64), np.int64)
    traces, streams = [], []
    for i, seg in enumerate(segs):
        own = min(R, nb - i * R)
        st = Stream(seg, h["dc_table"], h["ac_table"])
        blks = []
        tr, n = walk(st, max_blocks=own, blocks_out=blks)
        assert n == own and st.nbits - 8 < tr[-1][0] <= st.nbits, (i, n, own)
        zz = np.asarray(blks, np.int64)
        zz[:, 0] = np.cumsum(zz[:, 0])
        coefs[i * R:i * R + own][:, ZZ] = zz
        traces.append(tr)
        streams.append(st)
    h.update(coefs=coefs, traces=traces, streams=streams, segments=segs, ff00=pairs, end=end)
    return h


# ------------------------------------------------------------------------------ IDCT
_F = dict(F0298=2446, F0390=3196, F0541=4433, F0765=6270, F0899=7373, F1175=9633, F1501=12299, F1847=15137,
          F1961=16069, F2053=16819, F2562=20995, F3072=25172)
CONST_BITS, PASS1_BITS = 13, 2
# prepare_range_limit_table (jdmaster.c), seen from the centre: index = (value & 1023)
RANGE_LIMIT = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)])


def _idct_1d(d):
    """jidctint.c's 1-D kernel on d[..., 8] (int64), before descaling."""
    F = _F
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F["F0541"]
    t2 = z1 - z3 * F["F1847"]
    t3 = z1 + z2 * F["F0765"]
    t0 = (d[..., 0] + d[..., 4]) << CONST_BITS
    t1 = (d[..., 0] - d[..., 4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F["F1175"]
    a0, a1, a2, a3 = a0 * F["F0298"], a1 * F["F2053"], a2 * F["F3072"], a3 * F["F1501"]
    z1, z2 = -z1 * F["F0899"], -z2 * F["F2562"]
    z3, z4 = z5 - z3 * F["F1961"], z5 - z4 * F["F0390"]
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_islow(coefs, qt, preclamp=False):
    """jpeg_idct_islow on [nblocks, 64] coefficients: uint8 [nblocks, 8, 8]; with preclamp the
    values handed to the range-limit table instead (before & 1023)."""
    d = (np.asarray(coefs, np.int64).reshape(-1, 64) * np.asarray(qt, np.int64).reshape(64)).reshape(-1, 8, 8)
    ws = _descale(_idct_1d(d.transpose(0, 2, 1)), CONST_BITS - PASS1_BITS).transpose(0, 2, 1)   # columns
    o = _descale(_idct_1d(ws), CONST_BITS + PASS1_BITS + 3)                                      # rows
    return o if preclamp else RANGE_LIMIT[o & 1023].astype(np.uint8)


def assemble(blocks, H, W):
    """[nblocks, 8, 8] -> the [H, W] frame (blocks in raster order, cropped)."""
    bh, bw = (H + 7) // 8, (W + 7) // 8
    return np.asarray(blocks).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:H, :W]


def fdct(pixels):
    """Float forward DCT of [n, 8, 8] pixel blocks (level shift 128): unquantised coefficients."""
    k = np.arange(8)
    C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(0.125), 0.5)
    return C @ (np.asarray(pixels, np.float64) - 128.0) @ C.T
