"""Comb tables entry by entry (k_table_pow2, k_table_fill through
mbft_launch::build_tables, via the test-only harness
tests/csrc/launch_check.hip) against big-integer point arithmetic
(oracle/p256.py).

Entry (pt, win, d), d >= 1, lies at index pt * table_entries(W) +
(win << (W - 1)) + d - 1 and must hold exactly x 2^261 mod p, y 2^261 mod p
(canonical Montgomery form, 8 little-endian words each) of the affine point
(d 2^(W win) mod N) P_pt.  The verifier's tests reach only the entries random
scalars hit; here every entry of the small windows is compared (runs shorter
than 32 at W = 4, a last window of two entries at W = 5, of eight at W = 11)
and, at W = 16 and 20, the first and last entry of every window, both ends of
random runs, random entries, and the runs on either side of the fill
kernel's 2^19-run launch boundary.  One wrong entry is a signature that the
GPU alone rejects (or accepts).
"""
import ctypes
import os
import random

import numpy as np
import pytest

from comb_layout import entries, entry_bytes, last_bits, steps, window_bases, window_entries
from oracle import p256 as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = 32  # k_table_fill's run length (kFillRun)


@pytest.fixture(scope="module")
def harness(lib):
    path = os.path.join(ROOT, "tests", "liblaunch_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_launch_check
        build_launch_check()
    h = ctypes.CDLL(path)
    h.table_check_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.c_long, ctypes.c_void_p]
    h.table_check_run.restype = ctypes.c_int
    for f in (h.table_check_entries, h.table_check_words):
        f.argtypes = [ctypes.c_int]
        f.restype = ctypes.c_uint64
    h.table_check_steps.argtypes = [ctypes.c_int]
    h.table_check_steps.restype = ctypes.c_int
    return h


def points(n, seed):
    """G, then n - 1 random keys."""
    rng = random.Random(seed)
    return [o.G] + [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(n - 1)]


def xy_words(pts):
    return np.frombuffer(b"".join(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little") for p in pts),
                         dtype=np.uint32).copy()


def test_table_geometry(harness):
    """table_entries / table_steps / table_words against the formula for every
    window the library accepts: a table allocated one entry short puts the
    top window's last entry (digit 2^L) in the next key's table."""
    for W in range(4, 30):
        S = -(-256 // W)
        L = 256 - (S - 1) * W
        assert 0 < L <= W
        want = (S - 1) * (1 << (W - 1)) + (1 << L)
        assert harness.table_check_steps(W) == S
        assert harness.table_check_entries(W) == want
        assert harness.table_check_words(W) == 16 * want


@pytest.mark.parametrize("W", [4, 5, 6, 7, 8, 11])
def test_tables_exhaustive(harness, W):
    """Every entry of two points' tables (G and a random key) at the small
    windows: W = 4 (8-entry windows: runs shorter than 32), 5 (a last window
    of 2 entries), 6 (the signer's largest: 42 windows of 32 entries and a
    last window of 16), 7, 8, 11 (a last window of 8).  Catches a wrong run
    geometry (run length, runs per window, the last window's own geometry),
    a wrong first multiple of a run, the doubling at d = 2, and a Z-ratio
    walked back one step off."""
    pts = points(2, 0x7AB0 + W)
    ent = entries(W)
    want = bytearray()
    for pi, p in enumerate(pts):
        for win, b in enumerate(window_bases(p, W)):
            acc = b
            n = window_entries(W, win)
            for d in range(1, n + 1):
                want += entry_bytes(acc)
                if d < n:
                    acc = o.point_add(acc, b)
            # the window's last multiple, independently of the chain
            assert acc == o.scalar_mult((n << (W * win)) % o.N, p)
    assert len(want) == 64 * ent * len(pts)
    out = np.zeros(16 * ent * len(pts), dtype=np.uint32)
    assert harness.table_check_run(xy_words(pts).ctypes.data, len(pts), W, None, 0, out.ctypes.data) == 0
    got = out.tobytes()
    bad = [divmod(k, ent) for k in range(ent * len(pts)) if got[64 * k: 64 * k + 64] != want[64 * k: 64 * k + 64]]
    assert not bad, (len(bad), bad[:10])


def sample_indices(W, rng, nruns=64, nrand=256):
    """(win, d) samples of one table: the first and last entry of every
    window (the table's last entry among them), both ends of random runs,
    random entries."""
    S = steps(W)
    out = []
    for win in range(S):
        out += [(win, 1), (win, window_entries(W, win))]
    for _ in range(nruns):
        win = rng.randrange(S)
        run = rng.randrange(window_entries(W, win) // RUN)
        out += [(win, run * RUN + 1), (win, run * RUN + RUN)]
    for _ in range(nrand):
        win = rng.randrange(S)
        out.append((win, rng.randrange(1, window_entries(W, win) + 1)))
    return out


def check_samples(harness, pts, W, samples):
    """samples: (pt, win, d) triples."""
    ent = entries(W)
    bases = [window_bases(p, W) for p in pts]
    idx = np.array([pt * ent + (win << (W - 1)) + d - 1 for pt, win, d in samples], dtype=np.uint64)
    out = np.zeros(16 * len(samples), dtype=np.uint32)
    assert harness.table_check_run(xy_words(pts).ctypes.data, len(pts), W, idx.ctypes.data, len(idx),
                                   out.ctypes.data) == 0
    got = out.tobytes()
    bad = []
    for k, (pt, win, d) in enumerate(samples):
        assert 1 <= d <= window_entries(W, win)
        if got[64 * k: 64 * k + 64] != entry_bytes(o.scalar_mult(d, bases[pt][win])):
            bad.append((pt, win, d))
    assert not bad, (len(bad), bad[:10])


def test_table_sampled_w16(harness):
    """W = 16, one point (34 MiB): window ends -- the last entry of every
    window is digit 2^15, the largest positive digit, and the table's last
    entry digit 2^16 of the top window -- run ends and random entries."""
    rng = random.Random(0x7AB16)
    pts = points(2, 0x7AB16)[1:]
    check_samples(harness, pts, 16, [(0, win, d) for win, d in sample_indices(16, rng)])


def test_table_sampled_w20_launch_boundary(harness):
    """W = 20, three points (1.1 GiB, 595,968 runs): the fill kernel is
    launched over at most 2^19 runs at a time with a `first` offset, so the
    second launch starts inside point 2's table.  All 64 entries of the two
    runs on either side of global run 2^19, each point's last entry, and the
    per-point samples: a wrong `first`, a scratch plane indexed by the global
    instead of the launch-local thread, or a table base off by one point."""
    W = 20
    rng = random.Random(0x7AB20)
    pts = points(3, 0x7AB20)
    samples = [(pt, win, d) for pt in range(3) for win, d in sample_indices(W, rng)]
    S = steps(W)
    r0 = (1 << (W - 1)) // RUN
    runs = (S - 1) * r0 + (1 << last_bits(W)) // RUN
    assert 2 * runs < (1 << 19) < 3 * runs
    for g in ((1 << 19) - 1, 1 << 19):
        pt, rr = divmod(g, runs)
        assert pt == 2 and rr < (S - 1) * r0
        win, run = divmod(rr, r0)
        samples += [(pt, win, run * RUN + j + 1) for j in range(RUN)]
    samples += [(pt, S - 1, 1 << last_bits(W)) for pt in range(3)]
    check_samples(harness, pts, W, samples)
