"""LDS bank behaviour and fragment map of the flash-attention tile image.

A lane-by-lane model of the three access kinds of ops/csrc/flash_attn.hip
(ds_write_b128 staging, ds_read_b128 row reads, ds_read_b64_tr_b16
transposed reads) on the layout of tile_off, which this file mirrors; the
kernel's own reduced read offsets are tied to tile_off by a static_assert
in the source.  Bank of byte address a: (a/4) % 64 for the two reads,
(a/4) % 32 for writes.  Lane groups served in one LDS cycle: the two
32-lane halves for the transposed read, 8 consecutive lanes for
ds_write_b128, and for ds_read_b128 four groups of 16 made of aligned
4-lane runs.
"""
import pytest

B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
]
B128_GROUPS += [[lane + 32 for lane in g] for g in B128_GROUPS[:2]]
HALVES = [list(range(32)), list(range(32, 64))]
ROWS = 64  # the largest staged tile


def tile_off(d, row, ch):
    """Byte offset of 16-byte chunk ch of row `row` (tile_off, in bytes)."""
    return 2 * (8 * d * (row >> 3) + 256 * (ch >> 2) + 32 * (row & 7)
                + 8 * ((ch & 3) ^ ((row >> 2) & 3)))


def stage_map(d, tid, p):
    rest = tid >> 3
    row = 2 * (rest // (d // 32)) + ((tid >> 2) & 1) + p * (4096 // d)
    return row, 4 * (rest % (d // 32)) + (tid & 3)


def worst_conflict(addrs, width, groups, banks):
    worst = 1
    for group in groups:
        hit = {}
        for lane in group:
            for dword in range(width // 4):
                a = addrs[lane] + 4 * dword
                hit.setdefault((a // 4) % banks, set()).add(a)
        worst = max(worst, max(len(v) for v in hit.values()))
    return worst


@pytest.mark.parametrize("d", [64, 128])
def test_image_is_dense_and_writes_do_not_conflict(d):
    seen = set()
    for p in range(ROWS * d // 8 // 512):
        addrs = []
        for tid in range(512):
            row, ch = stage_map(d, tid, p)
            assert 0 <= row < ROWS and 0 <= ch < d // 8
            seen.add((row, ch))
            addrs.append(tile_off(d, row, ch))
        for wave in range(0, 512, 64):
            groups = [list(range(wave + 8 * k, wave + 8 * k + 8))
                      for k in range(8)]
            assert worst_conflict(addrs, 16, groups, 32) == 1
    assert len(seen) == ROWS * d // 8
    offs = {tile_off(d, r, c) for r in range(ROWS) for c in range(d // 8)}
    assert offs == set(range(0, ROWS * d * 2, 16))


@pytest.mark.parametrize("d", [64, 128])
def test_row_reads_do_not_conflict(d):
    for rb in (0, 32):
        for ks in range(d // 16):
            addrs = [tile_off(d, rb + (lane & 31), 2 * ks + (lane >> 5))
                     for lane in range(64)]
            assert worst_conflict(addrs, 16, B128_GROUPS, 64) == 1


@pytest.mark.parametrize("d", [64, 128])
def test_transposed_reads_give_the_fragment_without_conflicts(d):
    """Two transposed reads must deliver T[row0 + 8*hi + j][32*dt + col],
    j = 0..7, to lane (col = l & 31, hi = l >> 5)."""
    where = {}
    for row in range(ROWS):
        for col in range(d):
            where[tile_off(d, row, col // 8) + 2 * (col % 8)] = (row, col)
    for row0 in range(0, ROWS, 16):
        for dt in range(d // 32):
            frag = [[None] * 8 for _ in range(64)]
            for second in (0, 1):
                addrs = []
                for lane in range(64):
                    g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
                    row = row0 + 8 * (g >> 1) + 4 * second + q
                    ch = 4 * dt + 2 * (g & 1) + (p >> 1)
                    addrs.append(tile_off(d, row, ch) + 8 * (p & 1))
                assert all(a % 8 == 0 for a in addrs)
                assert worst_conflict(addrs, 8, HALVES, 64) == 1
                # the instruction: lane 4q+p of a 16-lane group addresses
                # row q, columns 4p..4p+3 of a 4 x 16 block; lane i gets
                # column i, row q in element q
                for lane in range(64):
                    g, i = lane >> 4, lane & 15
                    for q in range(4):
                        src = addrs[16 * g + 4 * q + (i >> 2)] + 2 * (i & 3)
                        frag[lane][4 * second + q] = where[src]
            for lane in range(64):
                for j in range(8):
                    assert frag[lane][j] == (row0 + 8 * (lane >> 5) + j,
                                             32 * dt + (lane & 31))
