"""The use-count stage k_key_account (minbft_amd/csrc/key_account.hip) through
the library's launcher on INJECTED slot words, statuses, descriptors and device
count (tests/csrc/key_account_check.hip): per slot, uses = the items whose slot
is < nslots and valid, rejects = those of them whose status is not 0.  The
counters are compared EXACTLY with numpy.bincount.

Sizes 1, 63, 64, 65, 1,000 and 66,000: a partial last wave, more than one
block; and 300,000, past the grid's cap of 4 blocks per CU on a 256-CU GPU
(262,144 items), where the kernel strides and a wave carries its last slot's
sums from one step to the next.  Slot patterns: one slot for all; 64 distinct slots in
every wave; two alternating; random over 8; random over 5,000.  Sprinkled in:
slot words >= nslots, >= kHostSlot, invalid slots, statuses 0..10.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_HOST_SLOT = 0xFFFFFF00
SIZES = [1, 63, 64, 65, 1000, 66000, 300000]
PATTERNS = ["one", "wave64", "two", "rand8", "rand5000"]


@pytest.fixture(scope="module")
def harness(lib):
    from __graft_entry__ import build_key_account_check
    h = ctypes.CDLL(build_key_account_check())
    vp = ctypes.c_void_p
    h.key_account_run.argtypes = [vp, vp, ctypes.c_long, ctypes.c_long, ctypes.c_long, vp, ctypes.c_uint32,
                                  ctypes.c_int, vp, vp]
    h.key_account_run.restype = ctypes.c_int
    return h


def make_case(pattern, n, rng, sprinkle=True):
    nslots = {"one": 3, "wave64": 64, "two": 7, "rand8": 8, "rand5000": 5000}[pattern]
    i = np.arange(n)
    if pattern == "one":
        slot = np.full(n, 2)
    elif pattern == "wave64":
        slot = i % 64
    elif pattern == "two":
        slot = np.where(i % 2 == 0, 1, 5)
    else:
        slot = rng.integers(0, nslots, n)
    slot = slot.astype(np.uint32)
    status = rng.integers(0, 11, n).astype(np.uint8)
    status[rng.random(n) < 0.5] = 0
    valid = np.ones(nslots, dtype=np.uint8)
    if sprinkle:
        r = rng.random(n)
        slot[r < 0.05] = nslots + rng.integers(0, 1000, n).astype(np.uint32)[r < 0.05]       # not registered
        slot[(r >= 0.05) & (r < 0.10)] = (K_HOST_SLOT + rng.integers(0, 256, n))[(r >= 0.05) & (r < 0.10)]
        slot[(r >= 0.10) & (r < 0.11)] = nslots                                                 # the first one past
        if nslots > 4:
            valid[rng.integers(0, nslots, max(1, nslots // 10))] = 0                            # invalid slots
    return slot, status, valid, nslots


def expected(slot, status, valid, nslots, count):
    s, st = slot[:count].astype(np.int64), status[:count]
    ok = s < nslots
    ok[ok] &= valid[s[ok]] != 0
    uses = np.bincount(s[ok], minlength=nslots).astype(np.uint64)
    rej = np.bincount(s[ok & (st != 0)], minlength=nslots).astype(np.uint64)
    return uses, rej


def run(harness, slot, status, n, count, valid, nslots, launches=1, start=0):
    cap = len(slot)
    uses = np.full(nslots + 1, start, dtype=np.uint64)
    rej = np.full(nslots + 1, start, dtype=np.uint64)
    uses[-1] = rej[-1] = 0xABCD  # the guard past the last slot
    rc = harness.key_account_run(slot.ctypes.data, status.ctypes.data, n, cap, count, valid.ctypes.data, nslots,
                                 launches, uses.ctypes.data, rej.ctypes.data)
    assert rc == 0
    assert uses[-1] == 0xABCD and rej[-1] == 0xABCD
    return uses[:-1], rej[:-1]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_counts_equal_bincount(harness, pattern):
    rng = np.random.default_rng(PATTERNS.index(pattern) + 7)
    for n in SIZES:
        for sprinkle in (False, True):
            slot, status, valid, nslots = make_case(pattern, n, rng, sprinkle)
            uses, rej = run(harness, slot, status, n, -1, valid, nslots)
            wu, wr = expected(slot, status, valid, nslots, n)
            assert np.array_equal(uses, wu), (pattern, n, sprinkle)
            assert np.array_equal(rej, wr), (pattern, n, sprinkle)


@pytest.mark.parametrize("n,count", [(65, 0), (65, 1), (1000, 63), (1000, 999), (66000, 64), (66000, 65537),
                                     (300000, 262145)])
def test_device_count_bounds_the_read(harness, n, count):
    """has_count batches: n is an upper bound, the count is on the device.
    Past it slots and statuses are poison that would be counted if read:
    valid slot numbers with status 0 and with status 1."""
    rng = np.random.default_rng(n + count)
    slot, status, valid, nslots = make_case("rand8", n, rng)
    slot[count:] = np.arange(n - count) % nslots
    status[count:] = np.arange(n - count) % 2
    uses, rej = run(harness, slot, status, n, count, valid, nslots)
    wu, wr = expected(slot, status, valid, nslots, count)
    assert np.array_equal(uses, wu) and np.array_equal(rej, wr)
    # a count above n (never produced, but the kernel clamps): n items
    if count:
        uses, rej = run(harness, slot[:count].copy(), status[:count].copy(), count - 1, count, valid, nslots)
        wu, wr = expected(slot, status, valid, nslots, count - 1)
        assert np.array_equal(uses, wu) and np.array_equal(rej, wr)


def test_launches_accumulate(harness):
    """Two launches into the same counters, which start from a value of their
    own (above 2^32: the counters are 64-bit)."""
    rng = np.random.default_rng(99)
    start = (1 << 32) + 5
    for pattern, n in (("one", 300000), ("rand5000", 66000), ("wave64", 1000)):
        slot, status, valid, nslots = make_case(pattern, n, rng)
        uses, rej = run(harness, slot, status, n, -1, valid, nslots, launches=2, start=start)
        wu, wr = expected(slot, status, valid, nslots, n)
        assert np.array_equal(uses, 2 * wu + np.uint64(start))
        assert np.array_equal(rej, 2 * wr + np.uint64(start))
