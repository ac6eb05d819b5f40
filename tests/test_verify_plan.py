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
n threads of scratch under the lane quads' 4 n (NAMED_ROW)."""
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
