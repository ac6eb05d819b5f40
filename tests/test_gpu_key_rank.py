"""The key memory budget's ranking kernels (minbft_amd/csrc/key_rank.hip)
through the library's launchers on INJECTED descriptors and counter arrays
(tests/csrc/key_rank_check.hip): k_key_age shifts every counter, k_key_hist
counts the ladder slots per (rung, use bin) and the valid slots outside the
ladder, k_key_pick lists the slots a plan moves (per target rung) or the cold
ones.  Everything is compared EXACTLY with numpy, and every output buffer has a
guard word past its end.

Sizes 1, 63, 64, 65, 1,000 and 66,000: a partial last wave, more than one
block; and 300,000, past the grid's cap of 4 blocks per CU on a 256-CU GPU
(262,144 slots), where a lane strides.  Use patterns: all zero (one histogram
cell takes every slot), the bin edges, log-uniform random; 1, 2 and 3 counter
arrays whose entries cross a bin edge only as a sum.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NBINS, MAXL = 496, 8
OUTSIDE = MAXL * NBINS
GUARD32, GUARD64 = 0xABCD1234, 0xABCD1234ABCD
SIZES = [1, 63, 64, 65, 1000, 66000, 300000]


def S(t):
    return 0x200 | t


LADDERS = {1: [0], 4: [0, S(3), S(6), 8], 8: [0, S(2), S(3), S(4), S(5), S(7), S(9), 8]}
OFF_LADDER = [16, 0x104, 12]


@pytest.fixture(scope="module")
def harness(lib):
    from __graft_entry__ import build_key_rank_check
    h = ctypes.CDLL(build_key_rank_check())
    vp, u32, i, sz, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64
    h.key_rank_age.argtypes = [vp, vp, sz, ctypes.c_uint]
    h.key_rank_add.argtypes = [vp, vp, sz]
    h.key_rank_hist.argtypes = [vp, vp, u32, vp, i, vp, i, vp]
    h.key_rank_pick_plan.argtypes = [vp, vp, u32, vp, i, vp, i, vp, vp, vp, vp]
    h.key_rank_pick_cold.argtypes = [vp, vp, u32, vp, i, u64, u32, vp, vp]
    for f in (h.key_rank_age, h.key_rank_add, h.key_rank_hist, h.key_rank_pick_plan, h.key_rank_pick_cold):
        f.restype = ctypes.c_int
    return h


def use_bins(u):
    """key_use_bin over a uint64 array: exact below 16, then eight bins an
    octave (the position of the leading one by halving, no floating point)."""
    v, e = u.copy(), np.zeros(len(u), dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (v >> np.uint64(s)) != 0
        e += s * m
        v = np.where(m, v >> np.uint64(s), v)
    sh = np.maximum(e - 3, 0).astype(np.uint64)
    big = 16 + 8 * (e - 4) + ((u >> sh) & np.uint64(7)).astype(np.int64)
    return np.where(u < 16, u.astype(np.int64), big)


def bin_edges():
    pts = list(range(41))
    for k in range(4, 64):
        pts += [2 ** k - 1, 2 ** k, 2 ** k + 2 ** (k - 3) - 1, 2 ** k + 2 ** (k - 3)]
    return np.array(pts + [2 ** 64 - 1], dtype=np.uint64)


def test_the_model_of_the_bins():
    """The numpy restatement agrees with the definition in Python integers."""
    def one(u):
        if u < 16:
            return u
        e = u.bit_length() - 1
        return 16 + 8 * (e - 4) + ((u >> (e - 3)) & 7)
    pts = bin_edges()
    assert use_bins(pts).tolist() == [one(int(u)) for u in pts]
    assert use_bins(pts).max() == NBINS - 1


def make_uses(pattern, n, rng):
    if pattern == "zero":
        return np.zeros(n, dtype=np.uint64)
    if pattern == "edges":
        e = bin_edges()
        return e[(np.arange(n) * 7 + 3) % len(e)]
    k = rng.integers(0, 64, n).astype(np.uint64)
    return (np.uint64(1) << k) | (rng.integers(0, 2 ** 63, n).astype(np.uint64) & ((np.uint64(1) << k) - np.uint64(1)))


def split_parts(u, nparts, rng):
    """nparts arrays that sum to u: the first ones random below what is left
    (so most sums cross bin edges that no part reaches)."""
    parts, left = [], u.copy()
    for _ in range(nparts - 1):
        top = np.uint64(2 ** 64 - 1)
        p = rng.integers(0, 2 ** 63, len(u)).astype(np.uint64) % np.where(left == top, top, left + np.uint64(1))
        parts.append(p)
        left = left - p
    parts.append(left)
    return np.ascontiguousarray(np.stack(parts))


def make_store(n, ladder, rng, mixed=True):
    """classes and valid words: slots spread over the rungs, and -- mixed --
    some outside the ladder and some invalid."""
    cls = np.array(ladder, dtype=np.uint32)[rng.integers(0, len(ladder), n)]
    valid = np.ones(n, dtype=np.uint8)
    if mixed:
        r = rng.random(n)
        cls[r < 0.1] = np.array(OFF_LADDER, dtype=np.uint32)[rng.integers(0, len(OFF_LADDER), n)][r < 0.1]
        valid[(r >= 0.1) & (r < 0.2)] = 0
    return cls, valid


def rungs_of(cls, valid, ladder):
    rung = np.full(len(cls), -1, dtype=np.int64)
    for j, c in enumerate(ladder):
        rung[cls == c] = j
    rung[valid == 0] = -1
    return rung


def model_hist(cls, valid, parts, ladder):
    u = parts.sum(axis=0, dtype=np.uint64) if len(parts) else np.zeros(len(cls), dtype=np.uint64)
    rung = rungs_of(cls, valid, ladder)
    on = rung >= 0
    want = np.zeros(OUTSIDE + 1, dtype=np.uint32)
    want[:OUTSIDE] = np.bincount(rung[on] * NBINS + use_bins(u[on]), minlength=OUTSIDE)
    want[OUTSIDE] = np.count_nonzero((valid != 0) & ~on)
    return want


def run_hist(h, cls, valid, parts, ladder):
    out = np.full(OUTSIDE + 2, 0x55, dtype=np.uint32)   # (stale words: the launcher zeroes them)
    out[-1] = GUARD32
    lad = np.array(ladder, dtype=np.uint32)
    rc = h.key_rank_hist(cls.ctypes.data, valid.ctypes.data, len(cls), parts.ctypes.data if len(parts) else None,
                         len(parts), lad.ctypes.data, len(lad), out.ctypes.data)
    assert rc == 0
    assert out[-1] == GUARD32
    return out[:-1]


# ------------------------------------------------------------------- k_key_age
@pytest.mark.parametrize("shift", [1, 7, 63])
def test_age_shifts_every_counter(harness, shift):
    rng = np.random.default_rng(shift)
    for n in SIZES[:6]:
        uses, rej = make_uses("rand", n + 1, rng), make_uses("edges", n + 1, rng)
        uses[0], rej[0] = 2 ** 64 - 1, 0
        if n > 1:
            uses[1], rej[1] = 0, 2 ** 64 - 1
        uses[-1] = rej[-1] = GUARD64
        wu, wr = uses >> np.uint64(shift), rej >> np.uint64(shift)
        assert harness.key_rank_age(uses.ctypes.data, rej.ctypes.data, n, shift) == 0
        assert uses[-1] == GUARD64 and rej[-1] == GUARD64
        assert np.array_equal(uses[:-1], wu[:-1]) and np.array_equal(rej[:-1], wr[:-1]), n


def test_add_sums_counter_arrays(harness):
    rng = np.random.default_rng(2)
    for n in (1, 65, 66000):
        dst, src = make_uses("rand", n + 1, rng), make_uses("rand", n, rng)
        dst[-1] = GUARD64
        want = dst[:-1] + src   # (wraps like the kernel's)
        assert harness.key_rank_add(dst.ctypes.data, src.ctypes.data, n) == 0
        assert dst[-1] == GUARD64 and np.array_equal(dst[:-1], want)


# ------------------------------------------------------------------ k_key_hist
@pytest.mark.parametrize("pattern", ["zero", "edges", "rand"])
def test_hist_equals_bincount(harness, pattern):
    rng = np.random.default_rng(["zero", "edges", "rand"].index(pattern) + 5)
    for n in SIZES:
        for nl in (1, 4, 8):
            nparts = 1 + (n + nl) % 3
            cls, valid = make_store(n, LADDERS[nl], rng)
            parts = split_parts(make_uses(pattern, n, rng), nparts, rng)
            got = run_hist(harness, cls, valid, parts, LADDERS[nl])
            want = model_hist(cls, valid, parts, LADDERS[nl])
            assert np.array_equal(got, want), (pattern, n, nl, nparts)
            assert got.sum() == np.count_nonzero(valid)


def test_hist_one_cell_takes_all(harness):
    """No uses at all and one class: every slot of 300,000 lands in cell
    (0, 0); and with no counter array at all the counts read as zero."""
    n = 300000
    cls, valid = np.zeros(n, dtype=np.uint32), np.ones(n, dtype=np.uint8)
    for parts in (np.zeros((3, n), dtype=np.uint64), np.zeros((0, n), dtype=np.uint64)):
        got = run_hist(harness, cls, valid, parts, LADDERS[4])
        assert got[0] == n and got.sum() == n


def test_hist_sums_cross_edges_only_as_sums(harness):
    """15 + 1, 2^40 - 1 + 1, 2^63 + 2^63 - 1 ...: no part is in the sum's bin."""
    a = np.array([15, 2 ** 40 - 1, 2 ** 63, 8, 2 ** 20 + 2 ** 17 - 1, 0], dtype=np.uint64)
    b = np.array([1, 1, 2 ** 63 - 1, 8, 1, 0], dtype=np.uint64)
    parts = np.ascontiguousarray(np.stack([a, b]))
    s = a + b
    assert all(use_bins(s)[i] not in (use_bins(a)[i], use_bins(b)[i]) for i in range(5))
    cls, valid = np.zeros(6, dtype=np.uint32), np.ones(6, dtype=np.uint8)
    got = run_hist(harness, cls, valid, parts, LADDERS[1])
    assert np.array_equal(got, model_hist(cls, valid, parts, LADDERS[1]))
    assert sorted(np.flatnonzero(got).tolist()) == sorted(set(use_bins(s).tolist()))


# ------------------------------------------------------------------ k_key_pick
def run_plan(h, cls, valid, parts, ladder, rob, caps):
    lad = np.array(ladder, dtype=np.uint32)
    caps = np.array(list(caps) + [0] * (MAXL - len(caps)), dtype=np.uint32)
    lists = np.full(int(caps[:len(lad)].sum()) + len(lad), GUARD32, dtype=np.uint32)
    count = np.full(MAXL + 1, 0x55, dtype=np.uint32)
    count[-1] = GUARD32
    rc = h.key_rank_pick_plan(cls.ctypes.data, valid.ctypes.data, len(cls), parts.ctypes.data, len(parts),
                              lad.ctypes.data, len(lad), rob.ctypes.data, caps.ctypes.data, lists.ctypes.data,
                              count.ctypes.data)
    assert rc == 0 and count[-1] == GUARD32
    out, off = [], 0
    for t in range(len(lad)):
        assert lists[off + caps[t]] == GUARD32, t
        out.append(lists[off:off + caps[t]])
        off += int(caps[t]) + 1
    return out, count[:MAXL]


def model_plan(cls, valid, parts, ladder, rob):
    u = parts.sum(axis=0, dtype=np.uint64)
    rung = rungs_of(cls, valid, ladder)
    target = rob.astype(np.int64)[use_bins(u)]
    return [np.flatnonzero((rung >= 0) & (target == t) & (rung != t)).astype(np.uint32) for t in range(len(ladder))]


@pytest.mark.parametrize("nl", [1, 4, 8])
def test_pick_plan_lists(harness, nl):
    """Each target's list, sorted, is numpy's; the counts are what the
    histogram and the plan give (what the host sizes the lists from)."""
    rng = np.random.default_rng(nl)
    ladder = LADDERS[nl]
    for n in SIZES:
        cls, valid = make_store(n, ladder, rng)
        parts = split_parts(make_uses("edges" if n % 2 else "rand", n, rng), 1 + n % 3, rng)
        rob = np.sort(rng.integers(0, nl, NBINS)).astype(np.uint8)
        want = model_plan(cls, valid, parts, ladder, rob)
        hist = run_hist(harness, cls, valid, parts, ladder)[:OUTSIDE].reshape(MAXL, NBINS)
        from_hist = [int(sum(hist[j][rob == t].sum() for j in range(nl) if j != t)) for t in range(nl)]
        assert from_hist == [len(w) for w in want]
        lists, count = run_plan(harness, cls, valid, parts, ladder, rob, from_hist)
        assert count.tolist() == from_hist + [0] * (MAXL - nl), n
        for t in range(nl):
            assert np.array_equal(np.sort(lists[t]), want[t]), (n, t)


def test_pick_plan_nothing_and_everything(harness):
    ladder, n = LADDERS[4], 66000
    rng = np.random.default_rng(3)
    parts = split_parts(make_uses("rand", n, rng), 2, rng)
    valid = np.ones(n, dtype=np.uint8)
    cls = np.full(n, ladder[2], dtype=np.uint32)
    # every slot is where the plan wants it
    lists, count = run_plan(harness, cls, valid, parts, ladder, np.full(NBINS, 2, dtype=np.uint8), [0, 0, 0, 0])
    assert not count.any()
    # every slot moves, to rung 3
    lists, count = run_plan(harness, cls, valid, parts, ladder, np.full(NBINS, 3, dtype=np.uint8), [0, 0, 0, n])
    assert count.tolist() == [0, 0, 0, n, 0, 0, 0, 0]
    assert np.array_equal(np.sort(lists[3]), np.arange(n, dtype=np.uint32))
    # a list shorter than what belongs on it is filled and not overrun: the count says so
    lists, count = run_plan(harness, cls, valid, parts, ladder, np.full(NBINS, 0, dtype=np.uint8), [1000, 0, 0, 0])
    assert count[0] == n and len(np.unique(lists[0])) == 1000 and lists[0].max() < n


@pytest.mark.parametrize("n", SIZES)
def test_pick_cold(harness, n):
    """The valid slots of any class with summed uses <= max_uses, with room
    for all of them and for fewer."""
    rng = np.random.default_rng(n)
    cls, valid = make_store(n, LADDERS[4], rng)
    u = make_uses("rand", n, rng)
    u[rng.random(n) < 0.3] = 0
    parts = split_parts(u, 1 + n % 3, rng)
    for max_uses in (0, 2 ** 20, 2 ** 64 - 1):
        want = np.flatnonzero((valid != 0) & (u <= np.uint64(max_uses))).astype(np.uint32)
        for cap in sorted({len(want) + 5, len(want), len(want) // 2, 0}):
            lst = np.full(cap + 1, GUARD32, dtype=np.uint32)
            count = np.array([0x55, GUARD32], dtype=np.uint32)
            rc = harness.key_rank_pick_cold(cls.ctypes.data, valid.ctypes.data, n, parts.ctypes.data, len(parts),
                                            max_uses, cap, lst.ctypes.data, count.ctypes.data)
            assert rc == 0 and count[1] == GUARD32 and lst[cap] == GUARD32
            assert count[0] == len(want), (n, max_uses, cap)
            got = lst[:min(cap, len(want))]
            if cap >= len(want):
                assert np.array_equal(np.sort(got), want)
                assert (lst[len(want):] == GUARD32).all()
            else:
                assert len(np.unique(got)) == cap and np.isin(got, want).all()
