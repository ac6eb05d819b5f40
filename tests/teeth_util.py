"""Scalars and the integer model shared by the compact key class's tests
(tests/test_teeth_host.py, tests/test_gpu_teeth_tables.py) and its fixture
script (tests/golden/make_teeth_edges.py).  The class is
minbft_amd/csrc/teeth_dev.h: t teeth, d = ceil(256 / t) columns."""
from oracle import p256 as o

N = o.N
TEETH = range(2, 9)


def columns(t):
    return (256 + t - 1) // t


def val(v, t):
    """The table's multiplier of entry v: sum_j bit_j(v) 2^(j d)."""
    d = columns(t)
    return sum(1 << (j * d) for j in range(t) if (v >> j) & 1)


def column_values(u, t):
    """v_c for c = d - 1 .. 0 (the order the evaluation takes them), from
    Python integers; bits of u at positions >= 256 do not exist."""
    d = columns(t)
    out = []
    for c in range(d - 1, -1, -1):
        v = 0
        for j in range(t):
            p = j * d + c
            if p < 256 and (u >> p) & 1:
                v |= 1 << j
        out.append(v)
    return out


def from_columns(cols, t):
    """u with the given column values (cols[k] = v_(d - 1 - k))."""
    d = columns(t)
    assert len(cols) == d
    return sum(val(v, t) << (d - 1 - k) for k, v in enumerate(cols))


def corner_scalars(t):
    """The issue's corners for t teeth, all below 2^256 (some at or above N:
    the recoding takes any 256-bit value)."""
    d = columns(t)
    out = [1, 2, N - 1, N - 2, 1 << 255, (1 << 256) - 1]
    for j in range(t):
        for v in ((1 << (j * d)), (1 << (j * d)) - 1):
            if 1 <= v < 1 << 256:
                out.append(v)
        for c in (1, d // 2, d - 1):
            if j * d + c < 256:
                out.append(1 << (j * d + c))
    # all-ones columns: every tooth's bit c set (where the position exists)
    for c in (0, 1, d // 2, d - 1):
        out.append(sum(1 << (j * d + c) for j in range(t) if j * d + c < 256))
    return out


def model_steps(cols, t):
    """The integer model of the evaluation over column values given from the
    top down.  Returns (degenerate steps, prefixes that are 0 mod N after the
    first nonzero column, final multiplier): a step is degenerate when an
    addition to a finite accumulator has 2 m' == +-k (mod N)."""
    m, started, degen, zeros = 0, False, [], []
    for k, v in enumerate(cols):
        m *= 2
        if v:
            kv = val(v, t)
            if started and ((m - kv) % N == 0 or (m + kv) % N == 0):
                degen.append((k, m, kv))
            m += kv
            started = True
        if started and m % N == 0:
            zeros.append(k)
    return degen, zeros, m
