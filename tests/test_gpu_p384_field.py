"""The P-384 class's field, scalar and point arithmetic ON THE DEVICE
(minbft_amd/csrc/p384_fe.h, p384_ecc.h): the vectors and the
model of tests/test_p384_host.py (tests/p384_ops_util.py), run by
tests/libp384_check.so one item per lane and compared with Python integers
word for word.  Host and device compile the same text to different code (the
device's products are v_mad_u64_u32), so the host run does not stand in for
this one."""
import ctypes

import numpy as np
import pytest

import p384_ops_util as u

pytestmark = pytest.mark.gpu

WORDS, MAX_IN, MAX_OUT = 14, 6, 3


@pytest.fixture(scope="module")
def harness(lib):
    import __graft_entry__ as ge
    h = ctypes.CDLL(ge.build_p384_check())
    h.p384_check_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    h.p384_check_run.restype = ctypes.c_int
    h.p384_check_op_code.argtypes = [ctypes.c_char_p]
    return h


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(WORDS)]


def run_op(h, op, operands):
    """operands: one tuple of integers per item -> one tuple of results each."""
    n = len(operands)
    code = h.p384_check_op_code(op.encode())
    assert code >= 0, op
    buf = np.zeros((n, MAX_IN, WORDS), dtype=np.uint32)
    for i, a in enumerate(operands):
        for k, v in enumerate(a):
            buf[i, k] = words(v)
    out = np.full((n, MAX_OUT, WORDS), 0xDEADBEEF, dtype=np.uint32)
    rc = h.p384_check_run(code, ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(out.ctypes.data), n)
    assert rc == 0, (op, rc)
    res = []
    for i in range(n):
        res.append(tuple(sum(int(w) << (32 * j) for j, w in enumerate(out[i, k])) for k in range(u.OPS[op][1])))
    return res


@pytest.mark.parametrize("op", sorted(u.OPS))
def test_operation_on_the_device(harness, op):
    operands = [a for o_, a in u.cases() if o_ == op]
    assert operands, op
    assert u.OPS[op][0] == len(operands[0])
    for a, got in zip(operands, run_op(harness, op, operands)):
        u.check(op, a, got)
