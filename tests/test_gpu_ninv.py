"""The batched s^-1 planes of the verifier, read back directly
(mbft_launch::batch_inverse_s, batch_inverse_s_local,
batch_inverse_s_pipelined through the test-only harness
tests/csrc/launch_check.hip) against big integers.

The verifier multiplies e and r by these planes and then makes u1, u2
canonical with ONE conditional subtraction (scalar_dev.h scalars()), which
rests on every plane value w being below 2^258 with normalized limbs.  The
suite otherwise sees the planes only through accept / reject of signatures
with random s; here, for every item of batches at each form's chain and
block boundaries:

* a valid s_i gives w_i = s_i^-1 2^261 (mod N);
* an invalid s_i (0, N, N + 1, 2^256 - 1) gives w_i = 2^261 (mod N) -- the
  forms treat it as 1 so that Montgomery's trick stays consistent -- and
  leaves every other item of its chain, block and batch exact;
* w_i < 2^258 and limbs 0..7 <= 2^29 - 1.

A prefix product handed to the wrong item, a chain walked back one step off
at a ragged end, a root shared across a block boundary, or an invalid s
poisoning its chain (a zero in Montgomery's trick makes every inverse of the
chain zero) each break the first property on the GPU replica alone.
"""
import ctypes
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
RN = (1 << 261) % N
MASK = (1 << 29) - 1
INVALID = [0, N, N + 1, (1 << 256) - 1]
SPECIAL = [1, 2, N - 1, N - 2, (N + 1) // 2, 1 << 255, 3, 5, 0xFFFF, 1 << 29, (1 << 232) - 1]

LEVELS, BLOCK, WAVE = 0, 1, 2   # ninv_check_run's forms
SIZES = {
    LEVELS: [1, 15, 16, 17, 4096, 4097, 65537],            # chains of 16; 4,096 roots at the top
    BLOCK: [1, 7, 8, 9, 2047, 2048, 2049, 5 * 2048 + 77],  # 256 threads x 8 items a block
    WAVE: [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097],  # 64 lanes x 16 items a wave
}
TINY = 17  # batches up to this size take an invalid s in every position


@pytest.fixture(scope="module")
def harness(lib):
    path = os.path.join(ROOT, "tests", "liblaunch_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_launch_check
        build_launch_check()
    h = ctypes.CDLL(path)
    h.ninv_check_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    h.ninv_check_run.restype = ctypes.c_int
    return h


def chain_of(form, n):
    """The items of one whole strided chain of the form (one that reaches the
    batch's ragged end where there is one)."""
    if form == LEVELS:
        G = -(-n // 16)
        return list(range(G // 2, n, G))
    span, stride = (2048, 256) if form == BLOCK else (1024, 64)
    base = (n - 1) // span * span
    t = min(3, n - 1 - base)
    return [i for i in range(base + t, min(base + span, n), stride)]


def check(harness, form, svals, invalid):
    """Run one batch; every item against its definition."""
    n = len(svals)
    s = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in svals), dtype=np.uint8).copy()
    planes = np.zeros((9, n), dtype=np.uint32)
    assert harness.ninv_check_run(form, s.ctypes.data, n, planes.ctypes.data) == 0
    assert (planes[:8] <= MASK).all(), np.nonzero((planes[:8] > MASK).any(axis=0))[0][:10]
    cols = planes.T.tolist()
    bad = []
    for i, (sv, l) in enumerate(zip(svals, cols)):
        v = sum(x << (29 * k) for k, x in enumerate(l))
        assert (i in invalid) == (sv == 0 or sv >= N)
        # (w s == 2^261 mod N  <=>  w == s^-1 2^261; an invalid s counts as 1)
        if v >= (1 << 258) or v * (1 if i in invalid else sv) % N != RN:
            bad.append((i, hex(sv), hex(v)))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("form,n", [(f, n) for f in (LEVELS, BLOCK, WAVE) for n in SIZES[f]])
def test_inverse_planes(harness, form, n):
    """Every plane value of a batch of n items: special values (1, 2, N - 1,
    N - 2, (N + 1) / 2, 2^255, small ones) and random ones, all valid; then
    the same batch with an invalid s at index 0 and at index n - 1, with one
    whole strided chain invalid, and (tiny batches) with an invalid s in each
    position in turn."""
    rng = random.Random((form << 20) | n)
    base = [rng.randrange(1, N) for _ in range(n)]
    for v in SPECIAL:                     # at both ends, and scattered
        for i in {SPECIAL.index(v) % n, (n - 1 - SPECIAL.index(v)) % n, rng.randrange(n)}:
            base[i] = v
    check(harness, form, base, set())
    scenarios = [{0, n - 1}, set(chain_of(form, n))]
    if n <= TINY:
        scenarios += [{i} for i in range(n)] + [set(range(n))]
    for k, inv in enumerate(scenarios):
        assert inv and max(inv) < n
        sv = list(base)
        for j, i in enumerate(sorted(inv)):
            sv[i] = INVALID[(j + k) % 4]
        check(harness, form, sv, inv)
