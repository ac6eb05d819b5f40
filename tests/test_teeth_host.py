"""The compact key class's recoding (minbft_amd/csrc/teeth_dev.h:
teeth_columns, teeth_column) compiled for the HOST into
tests/libteeth_check.so (tests/csrc/teeth_check.cpp) and checked against
Python integers for every t in 2..8: the columns are the scalar's bits tooth
by tooth, they rebuild the scalar, no bit at a position >= 256 sets a tooth;
and the integer model of the evaluation meets no degenerate addition and no
zero prefix for any scalar in [1, N), as the header argues.  The GPU run is
compared with the oracle in tests/test_gpu_compact_keys.py."""
import ctypes
import random

import numpy as np
import pytest

from teeth_util import N, TEETH, column_values, columns, corner_scalars, from_columns, model_steps, val


@pytest.fixture(scope="module")
def lib():
    from __graft_entry__ import build_teeth_check
    lib = ctypes.CDLL(build_teeth_check())
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.teeth_check_recode.argtypes = [vp, i, i, vp]
    lib.teeth_check_columns.argtypes = [i]
    return lib


def _cols(lib, scalars, t):
    d = lib.teeth_check_columns(t)
    assert d == columns(t)
    n = len(scalars)
    u = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in scalars), dtype=np.uint8).copy()
    out = np.full(n * d, 0xEE, dtype=np.uint8)
    assert lib.teeth_check_recode(u.ctypes.data, n, t, out.ctypes.data) == 0
    return out.reshape(n, d)


@pytest.mark.parametrize("t", list(TEETH))
def test_columns_against_python_integers(lib, t):
    rng = random.Random(0x7ee7 + t)
    scalars = [rng.randrange(1, 1 << 256) for _ in range(2000)] + corner_scalars(t)
    d = columns(t)
    cols = _cols(lib, scalars, t)
    assert int(cols.max()) < 1 << t
    for u, row in zip(scalars, cols.tolist()):
        assert row == column_values(u, t), hex(u)
        assert from_columns(row, t) == u, hex(u)  # sum_c val(v_c) 2^c == u
        # no tooth bit stands for a position >= 256 (the ragged top tooth)
        for k, v in enumerate(row):
            c = d - 1 - k
            for j in range(t):
                if (v >> j) & 1:
                    assert j * d + c < 256, (hex(u), j, c)


def test_refused_teeth(lib):
    buf = np.zeros(256, dtype=np.uint8)
    for t in (0, 1, 9, -1):
        assert lib.teeth_check_recode(buf.ctypes.data, 1, t, buf.ctypes.data) == -1


@pytest.mark.parametrize("t", list(TEETH))
def test_integer_model_has_no_degenerate_step(lib, t):
    """Over 10,000 random scalars in [1, N) and the corners below N: no
    addition with 2 m' == +-k (mod N), no prefix == 0 (mod N) after the first
    nonzero column, and the model ends at u."""
    rng = random.Random(0xc0317 + t)
    scalars = [rng.randrange(1, N) for _ in range(10000)] + [u for u in corner_scalars(t) if 1 <= u < N]
    for u, row in zip(scalars, _cols(lib, scalars, t).tolist()):
        degen, zeros, m = model_steps(row, t)
        assert m == u and not degen and not zeros, (hex(u), degen[:2], zeros[:2])


@pytest.mark.parametrize("t", list(TEETH))
def test_table_multipliers(t):
    mult = [val(v, t) for v in range(1, 1 << t)]
    assert all(1 <= m < N for m in mult)
    assert len(set(mult)) == len(mult)
    assert len({m % N for m in mult}) == len(mult)
