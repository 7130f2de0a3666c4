"""CPU: the index maps of the layer-1 bottleneck tail's 16-byte row pieces (btail.hip, rows = 1).

The first product runs in the C^T form MFMA(W3, A): fragment j covers rows 16 j .. 16 j + 15 of the
kernel's image of W3, and lane group fg = lane >> 4 receives in register r the output of image row
16 j + 4 fg + r (lane & 15 selects the pixel, so every lane of a group sees the same channels).
spe_debug_btail_row_perm(p) names the channel that image row p holds; the fragment pair (2i, 2i + 1)
then forms the lane's piece i of 8 values, channels 32 i + 8 sg .. + 7 with sg = (0, 2, 1, 3)[fg], which
is stored as 16 bytes at byte 64 i + 16 sg of the row.

sg and not fg (the order the issue proposed), because z has to stay bit-identical and the MFMA's internal
sum depends on the K slot: before the second product the kernel swaps, between the lane groups (0, 1)
and (2, 3), the upper 4 values of the even group with the lower 4 of the odd one (v_permlane16_swap), and
with sg that leaves group g with channels 32 i + 4 g + {0..3} and 32 i + 16 + 4 g + {0..3} -- the K slots
of the 8-byte form, so W1's column order spe_debug_btail_perm is unchanged.
"""
from spe import _lib

SG = (0, 2, 1, 3)


def _lane_channels(L, fg):
    """Channels of lane group fg's registers after the first product: [8 i + e] for piece i, element e."""
    out = []
    for i in range(8):                     # pieces: fragment pairs (2i, 2i + 1)
        for e in range(8):
            j, r = 2 * i + e // 4, e % 4
            out.append(L.spe_debug_btail_row_perm(16 * j + 4 * fg + r))
    return out


def test_row_perm_is_a_bijection_on_every_32_row_group():
    L = _lib.lib()
    for n in (64, 128, 256):               # W1's rows (n2 = 64 / 128) and W3's (256)
        assert sorted(L.spe_debug_btail_row_perm(p) for p in range(n)) == list(range(n))
    assert L.spe_debug_btail_row_perm(-1) == -1


def test_row_perm_gives_a_lane_eight_consecutive_channels():
    L = _lib.lib()
    for j in range(16):
        for fg in range(4):
            for r in range(4):
                assert L.spe_debug_btail_row_perm(16 * j + 4 * fg + r) == 32 * (j // 2) + 8 * SG[fg] + 4 * (j % 2) + r


def test_column_perm_is_a_bijection():
    L = _lib.lib()
    assert sorted(L.spe_debug_btail_perm(k) for k in range(256)) == list(range(256))


def test_pieces_cover_a_row_in_channel_order():
    """Every (lane, register): piece i of lane group fg is channels 32 i + 8 sg .. + 7, so the 16-byte stores at
    byte 64 i + 16 sg of a row write channels 0 .. 255 in order."""
    L = _lib.lib()
    row = [None] * 256
    for fg in range(4):
        ch = _lane_channels(L, fg)
        for i in range(8):
            for e in range(8):
                row[32 * i + 8 * SG[fg] + e] = ch[8 * i + e]      # the element's position in the stored row
    assert row == list(range(256))


def _swapped(lo, hi):
    """v_permlane16_swap on (lo, hi) indexed by lane group: the odd groups of lo <-> the even groups of hi."""
    lo, hi = list(lo), list(hi)
    for g in (0, 2):
        lo[g + 1], hi[g] = hi[g], lo[g + 1]
    return lo, hi


def test_second_product_pairs_each_k_slot_with_its_channel():
    """After the swap lane group g feeds K slots 32 kc + 8 g + e of the second product; W1's stored column with that
    index holds channel spe_debug_btail_perm(32 kc + 8 g + e): both must be the same channel for every slot."""
    L = _lib.lib()
    held = [_lane_channels(L, fg) for fg in range(4)]
    for kc in range(8):
        lo = [held[fg][8 * kc: 8 * kc + 4] for fg in range(4)]
        hi = [held[fg][8 * kc + 4: 8 * kc + 8] for fg in range(4)]
        lo, hi = _swapped(lo, hi)
        for g in range(4):
            slots = lo[g] + hi[g]
            assert slots == [L.spe_debug_btail_perm(32 * kc + 8 * g + e) for e in range(8)]
            assert slots == [32 * kc + 4 * g + e for e in range(4)] + [32 * kc + 16 + 4 * g + e for e in range(4)]
