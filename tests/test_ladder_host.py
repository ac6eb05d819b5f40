"""The table-free ladder's recoding (minbft_amd/csrc/ladder_dev.h: naf_init,
naf_next) compiled for the HOST into tests/libladder_check.so
(tests/csrc/ladder_check.cpp) and checked against Python integers: the digits
reconstruct the scalar, they are the non-adjacent form, and the integer model
of the ladder meets a degenerate addition (accumulator == +-Q) for exactly the
scalars the header's argument lists.  The GPU run of the ladder is compared
with the oracle in tests/test_gpu_tablefree.py."""
import ctypes
import random

import numpy as np
import pytest

from ladder_util import DEGENERATE, N, model_degenerate_steps, naf, named_scalars, power_scalars


@pytest.fixture(scope="module")
def lib():
    from __graft_entry__ import build_ladder_check
    lib = ctypes.CDLL(build_ladder_check())
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.ladder_check_recode.argtypes = [vp, i, vp]
    lib.ladder_check_digits.argtypes = []
    return lib


def _digits(lib, scalars):
    nd = lib.ladder_check_digits()
    assert nd == 257
    n = len(scalars)
    u = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in scalars), dtype=np.uint8).copy()
    out = np.zeros(n * nd, dtype=np.int8)
    assert lib.ladder_check_recode(u.ctypes.data, n, out.ctypes.data) == 0
    return out.reshape(n, nd)


@pytest.fixture(scope="module")
def cases(lib):
    rng = random.Random(0x1adde7)
    scalars = [rng.randrange(1, N) for _ in range(10000)] + named_scalars() + power_scalars()
    return scalars, _digits(lib, scalars)


def test_digits_reconstruct_the_scalar(cases):
    scalars, digs = cases
    w = [1 << (256 - j) for j in range(257)]
    for u, d in zip(scalars, digs):
        assert sum(int(x) * wj for x, wj in zip(d, w) if x) == u


def test_digits_are_the_non_adjacent_form(cases):
    scalars, digs = cases
    assert set(np.unique(digs).tolist()) <= {-1, 0, 1}
    # no two adjacent nonzero digits, over the whole set at once
    assert not np.any((digs[:, 1:] != 0) & (digs[:, :-1] != 0))
    # the form is unique, so it equals the textbook right-to-left recoding
    for u, d in list(zip(scalars, digs))[::97] + list(zip(scalars, digs))[10000:]:
        ref = naf(u)
        ref = [0] * (257 - len(ref)) + ref[::-1]
        assert d.tolist() == ref, hex(u)


def test_scalars_beyond_the_order_recode_too(lib):
    """naf_init takes any u < 2^256 (3 u has 258 bits): the verifier only
    passes u < N, the recoding itself does not depend on it."""
    top = [(1 << 256) - 1, (1 << 256) - 2, N, N + 1]
    for u, d in zip(top, _digits(lib, top)):
        assert sum(int(x) << (256 - j) for j, x in enumerate(d)) == u


def test_degenerate_additions_are_exactly_the_listed_scalars(cases):
    scalars, digs = cases
    hit = {}
    for u, d in zip(scalars, digs):
        steps, m = model_degenerate_steps(d.tolist())
        assert m == u
        if steps:
            hit[u] = steps
    assert set(hit) == set(DEGENERATE)
    # u = N - 2: the LAST step adds -Q to (N - 1) Q = -Q (a doubling)
    (j, m, d), = hit[N - 2]
    assert j == 256 and m == N - 1 and d == -1


def test_prefixes_stay_inside_the_order(cases):
    """Every prefix from the first nonzero digit on is in [1, N): the
    accumulator is never infinity again and no doubling meets order 2."""
    scalars, digs = cases
    for u, d in list(zip(scalars, digs))[::53] + list(zip(scalars, digs))[10000:]:
        m, started = 0, False
        for x in d.tolist():
            m = 2 * m + x
            started = started or x != 0
            if started:
                assert 0 < m < N, hex(u)
