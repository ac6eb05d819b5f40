"""The signed compact key class's tables entry by entry (k_steeth_table
through mbft_launch::build_steeth_tables, via the test-only harness
tests/csrc/steeth_tables_check.hip) against the oracle's scalar multiples
(oracle/p256.py).

The table of key pt for t teeth is 2^(t-1) entries of 64 bytes at
pt * 2^(t-1); entry idx must hold exactly x 2^261 mod p, y 2^261 mod p
(canonical Montgomery form, 8 little-endian words each -- the comb-entry
format) of the affine point m Q, m = 2^((t-1) d) + sum_(j < t-1) sigma_j
2^(j d), sigma_j = +1 iff bit j of idx is set, d = ceil(256 / t).  Entry 0 IS
read.  Keys: a random Q, Q = G and Q = -G.  Every entry for t <= 6; for
t = 7, 8, 9, 32 sampled entries per key: the first, the last, the single-bit
indices and random ones; and the keys on either side of a launch boundary.
"""
import ctypes
import random

import numpy as np
import pytest

from comb_layout import entry_bytes
from oracle import p256 as o
from steeth_util import entry_mult

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(lib):
    from __graft_entry__ import build_steeth_tables_check
    h = ctypes.CDLL(build_steeth_tables_check())
    h.steeth_tables_check_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    h.steeth_tables_check_run.restype = ctypes.c_int
    h.steeth_tables_check_words.argtypes = [ctypes.c_int]
    h.steeth_tables_check_words.restype = ctypes.c_uint64
    return h


@pytest.fixture(scope="module")
def keys():
    rng = random.Random(0x57ee7ab)
    return [o.scalar_mult(rng.randrange(1, o.N), o.G), o.G, o.point_neg(o.G)]


def xy_words(pts):
    return np.frombuffer(b"".join(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little") for p in pts),
                         dtype=np.uint32).copy()


def _tables(harness, keys, t):
    ne = 1 << (t - 1)
    assert harness.steeth_tables_check_words(t) == 16 * ne
    out = np.zeros(16 * ne * len(keys), dtype=np.uint32)
    assert harness.steeth_tables_check_run(xy_words(keys).ctypes.data, len(keys), t, out.ctypes.data) == 0
    return out.tobytes()


def _compare(got, keys, t, entries_of):
    ne, bad = 1 << (t - 1), []
    for pi, q in enumerate(keys):
        for idx in entries_of(pi):
            assert 0 <= idx < ne
            k = pi * ne + idx
            if got[64 * k: 64 * k + 64] != entry_bytes(o.scalar_mult(entry_mult(idx, t), q)):
                bad.append((pi, idx))
    assert not bad, (t, len(bad), bad[:10])


def test_refused_teeth(harness, keys):
    out = np.zeros(64, dtype=np.uint32)
    for t in (0, 1, 10, -1):
        assert harness.steeth_tables_check_run(xy_words(keys).ctypes.data, len(keys), t, out.ctypes.data) == -1


@pytest.mark.parametrize("t", [2, 3, 4, 5, 6])
def test_tables_exhaustive(harness, keys, t):
    """Every entry of the three keys' tables."""
    _compare(_tables(harness, keys, t), keys, t, lambda pi: range(1 << (t - 1)))


@pytest.mark.parametrize("t", [7, 8, 9])
def test_tables_sampled(harness, keys, t):
    """32 entries per key: the first, the last, the single-bit indices and
    random ones."""
    rng = random.Random(0x57ee7ab + t)
    ne = 1 << (t - 1)

    def sample(pi):
        s = {0, ne - 1} | {1 << j for j in range(t - 1)}
        while len(s) < 32:
            s.add(rng.randrange(ne))
        return sorted(s)

    _compare(_tables(harness, keys, t), keys, t, sample)


def test_launch_boundary(harness):
    """t = 9, 4,100 keys (64 MiB of tables): the build runs in launches of at
    most 4,096 keys with a `first` offset and launch-local scratch, so the
    second launch starts at key 4,096.  Key i is (i + 2) G; sampled entries of
    the keys on either side of the boundary and of the last key."""
    t, n = 9, 4100
    ne = 1 << (t - 1)
    assert (64 << 20) // (64 * ne) == 4096
    pts, p = [], o.point_add(o.G, o.G)
    for _ in range(n):
        pts.append(p)
        p = o.point_add(p, o.G)
    got = _tables(harness, pts, t)
    bad = []
    for pi in (0, 4095, 4096, 4097, n - 1):
        for idx in (0, 1, 2, 3, 128, 129, 254, 255):
            k = pi * ne + idx
            if got[64 * k: 64 * k + 64] != entry_bytes(o.scalar_mult(entry_mult(idx, t) * (pi + 2) % o.N, o.G)):
                bad.append((pi, idx))
    assert not bad, bad
