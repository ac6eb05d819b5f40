"""The verifier's launch plan (minbft_amd/csrc/verify_plan.h) compiled for the
HOST into tests/libverify_plan_check.so (tests/csrc/verify_plan_check.cpp).

(a) The form of every kind of batch is the one the two decision sites the
plan replaced chose between them -- verify_device's `small` and the old
launcher's branches, written out below as they stood -- over n x s^-1 source x
device count x planes workspace x split_max x small_form x MBFT_LANE_INV_MAX.
(b) For every row the `slowq` buffer covers the queues plus 36 spill planes
of the 256-rounded threads the form's kernel indexes: 4 n for the lane
quads, 2 n for the lane pairs, the grid for k_verify (a MBFT_VERIFY_BPC cap
only lowers it), none for the split kernel.  The old size, verify_words(n, n
<= lane_inv_max || count), did not: host planes past MBFT_LANE_INV_MAX got
n threads of scratch under the lane quads' 4 n (NAMED_ROW).
(c) The large form's three grids -- k_verify under a MBFT_VERIFY_BPC cap,
k_verify_slow at four blocks per CU clamped to k_verify's, k_verify_ladder at
two per CU -- are the expressions the launcher held, below, at and above each
cap on 1, 8, 256 and 304 CUs."""
import ctypes
import itertools

import pytest

SPLIT_HOST, SPLIT_WAVE, QUADS_INLINE, QUADS_PLANES, QUADS_HOST, PAIRS_PLANES, PAIRS_LANE, LARGE = range(8)

NS = (1, 64, 65, 256, 257, 4096, 4097, 1 << 20)
ROWS = list(itertools.product(NS, (False, True), (False, True), (False, True), (0, 256), (0, 1, 2, 3), (0, 4096)))
# n = 65, host planes, no count, no workspace, split_max 0, small_form 2, lane_inv_max 0
NAMED_ROW = (65, True, False, False, 0, 2, 0)


@pytest.fixture(scope="module")
def lib():
    from __graft_entry__ import build_verify_plan_check
    lib = ctypes.CDLL(build_verify_plan_check())
    lib.verify_plan_check.argtypes = [ctypes.c_long, ctypes.c_ulong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    lib.verify_plan_check.restype = None
    return lib


def plan(lib, row):
    n, host_planes, has_count, has_ws, split_max, small_form, lane_inv_max = row
    out = (ctypes.c_long * 7)()
    lib.verify_plan_check(n, lane_inv_max, host_planes, has_count, has_ws, split_max, small_form, out)
    return dict(zip(("form", "threads", "ninv_first", "queue_reset", "words", "scratch", "spill"), out))


def old_form(row):
    """What the two old sites chose, as they stood."""
    n, host_planes, has_count, has_ws, split_max, small_form, lane_inv_max = row
    # verify_device: the planes handed to the launcher
    small = n <= lane_inv_max or has_count
    winv = "host" if host_planes else None if small else "batch"
    # the launcher
    if host_planes:
        if n <= split_max:
            return SPLIT_HOST
        if small_form >= 2:
            return QUADS_HOST
        winv = None
    if winv is None and n <= split_max:
        return SPLIT_WAVE
    if winv is None or has_count:
        if winv is None and has_ws and small_form != 0:
            return {2: QUADS_INLINE, 3: QUADS_PLANES, 1: PAIRS_PLANES}[small_form]
        return PAIRS_LANE
    return LARGE


def round256(t):
    return (t + 255) // 256 * 256


def scratch_offset(n):
    """The queues in front of the spill planes: n + 2 words, then n words,
    each rounded up to 64."""
    queue2 = (n + 2 + 63) // 64 * 64
    return (queue2 + n + 63) // 64 * 64


INDEXED = {SPLIT_HOST: 0, SPLIT_WAVE: 0, QUADS_INLINE: 4, QUADS_PLANES: 4, QUADS_HOST: 4, PAIRS_PLANES: 2,
           PAIRS_LANE: 2, LARGE: 1}


def test_named_row_is_in_the_table():
    assert NAMED_ROW in ROWS and old_form(NAMED_ROW) == QUADS_HOST


def test_form_of_every_row(lib):
    seen = set()
    for row in ROWS:
        p, want = plan(lib, row), old_form(row)
        assert p["form"] == want, row
        assert p["ninv_first"] == (want in (QUADS_PLANES, PAIRS_PLANES)), row
        assert p["queue_reset"] == (want == LARGE), row
        seen.add(want)
    assert seen == set(range(8))  # the table reaches every form


def test_slowq_covers_what_the_kernel_indexes(lib):
    for row in ROWS:
        n = row[0]
        p = plan(lib, row)
        threads = INDEXED[p["form"]] * n
        if INDEXED[p["form"]]:
            assert p["threads"] == threads, row  # the grid is what the kernel indexes
        else:
            assert p["threads"] == 256 * n, row  # one workgroup an item
        assert p["scratch"] == scratch_offset(n), row
        assert p["words"] >= scratch_offset(n) + 36 * round256(threads), row


def test_old_size_missed_the_named_row(lib):
    n, host_planes, has_count, _, _, _, lane_inv_max = NAMED_ROW
    small = n <= lane_inv_max or has_count
    old_words = scratch_offset(n) + 36 * round256(4 * n if small else n)  # verify_words(n, small)
    need = scratch_offset(n) + 36 * round256(4 * n)
    assert old_words < need
    assert plan(lib, NAMED_ROW)["words"] >= need


# ------------------------------------------------- the kLarge form's three grids
def large_grids(lib, blocks, bpc, ncu):
    out = (ctypes.c_long * 5)()
    lib.verify_large_grids_check(blocks, bpc, ncu, out)
    return tuple(out)


def launcher_grids(blocks, bpc, ncu):
    """mbft_launch::verify's kLarge branch as it stood before the rules moved
    into verify_plan.h, expression for expression."""
    vblocks = bpc * ncu if bpc > 0 and blocks > bpc * ncu else blocks
    k_slow_bpc = 4
    sblocks = blocks if blocks < ncu * k_slow_bpc else ncu * k_slow_bpc
    if sblocks > vblocks:
        sblocks = vblocks
    lblocks = blocks if blocks < ncu * 2 else ncu * 2
    return vblocks, sblocks, lblocks


NCUS = (1, 8, 256, 304)
BPCS = (0, 1, 2, 3, 4, 8)


def grid_rows():
    """Below, at and above every cap: bpc ncu (k_verify), 4 ncu (k_verify_slow),
    2 ncu (k_verify_ladder), for each ncu and bpc; plus one block and 2^22."""
    rows = []
    for ncu, bpc in itertools.product(NCUS, BPCS):
        edges = {1, 1 << 22}
        for cap in (bpc * ncu, 2 * ncu, 4 * ncu):
            edges.update(b for b in (cap - 1, cap, cap + 1) if b >= 1)
        rows += [(b, bpc, ncu) for b in sorted(edges)]
    return rows


def test_large_grids_are_the_launchers(lib):
    lib.verify_large_grids_check.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_void_p]
    lib.verify_large_grids_check.restype = None
    rows = grid_rows()
    assert len(rows) > 200
    capped = slow_clamped = 0
    for blocks, bpc, ncu in rows:
        got = large_grids(lib, blocks, bpc, ncu)
        assert got[3:] == (4, 2)
        assert got[:3] == launcher_grids(blocks, bpc, ncu), (blocks, bpc, ncu)
        v, s, ld = got[:3]
        # what the kernels rely on: no empty grid, none past the plan's blocks,
        # k_verify_slow inside the spill planes laid out for k_verify's threads
        assert 1 <= s <= v <= blocks and 1 <= ld <= blocks, (blocks, bpc, ncu)
        assert s <= 4 * ncu and ld <= 2 * ncu and (bpc == 0 or v <= bpc * ncu)
        capped += v < blocks
        slow_clamped += s < min(blocks, 4 * ncu)
    assert capped > 50 and slow_clamped > 20
    # the sizes the issue of the second pass names, on 256 CUs
    assert large_grids(lib, 1 << 12, 0, 256)[:3] == (4096, 1024, 512)  # 1M items: 8 ladder passes
    assert large_grids(lib, 512, 0, 256)[:3] == (512, 512, 512)        # 131,072 items: the last single pass
    assert large_grids(lib, 513, 0, 256)[:3] == (513, 513, 512)
    # bpc = 1: the ladder's 2 ncu blocks are MORE than k_verify's grid (it spills
    # nothing), k_verify_slow's are clamped to it
    assert large_grids(lib, 2054, 1, 256)[:3] == (256, 256, 512)
    assert large_grids(lib, 2054, 1, 304)[:3] == (304, 304, 608)
    assert large_grids(lib, 17, 1, 8)[:3] == (8, 8, 16)
    assert large_grids(lib, 3, 1, 1)[:3] == (1, 1, 2)
