"""Scalars and the integer model shared by the signed compact key class's
tests (tests/test_steeth_host.py, tests/test_gpu_steeth_tables.py) and its
fixture script (tests/golden/make_steeth_edges.py).  The class is the signed
part of minbft_amd/csrc/teeth_dev.h: t = 2..9 teeth, d = ceil(256 / t)
columns, L = t d, a table of 2^(t-1) entries."""
from oracle import p256 as o

N = o.N
STEETH = range(2, 10)


def columns(t):
    return (256 + t - 1) // t


def flip(u):
    """(k, flipped): the odd scalar the comb evaluates for u in [1, N)."""
    return (u, False) if u & 1 else (N - u, True)


def digits(k, t):
    """b_(L-1) .. b_0 as a function i -> +-1 of the odd k < 2^L."""
    L = t * columns(t)
    assert k & 1 and 0 < k < 1 << L
    return lambda i: 1 if i == L - 1 or (k >> (i + 1)) & 1 else -1


def entry_mult(idx, t):
    """The table's multiplier of entry idx: 2^((t-1) d) + sum_(j < t-1)
    sigma_j 2^(j d), sigma_j = +1 iff bit j of idx is set."""
    d = columns(t)
    return (1 << ((t - 1) * d)) + sum((1 if (idx >> j) & 1 else -1) << (j * d) for j in range(t - 1))


def column_list(k, t):
    """[(idx, neg)] for c = d - 1 .. 0 (the order the evaluation takes them),
    from the digits alone (no raw-bit trick: the definition)."""
    d, b = columns(t), digits(k, t)
    out = []
    for c in range(d - 1, -1, -1):
        s = [b(j * d + c) for j in range(t)]
        neg = s[t - 1] < 0
        idx = sum(1 << j for j in range(t - 1) if s[j] == s[t - 1])
        out.append((idx, neg))
    return out


def column_value(idx, neg, t):
    m = entry_mult(idx, t)
    return -m if neg else m


def model(cols, t):
    """The integer model of the evaluation over [(idx, neg)] from the top
    down.  Returns (final multiplier, prefixes outside (0, N) as (step, m),
    degenerate steps as (step, 2 m', val)): a step is degenerate when 2 m' ==
    +-val (mod N)."""
    m, outside, degen = 0, [], []
    for k, (idx, neg) in enumerate(cols):
        v = column_value(idx, neg, t)
        if k:
            m *= 2
            if (m - v) % N == 0 or (m + v) % N == 0:
                degen.append((k, m, v))
        m += v
        if not 0 < m < N:
            outside.append((k, m))
    return m, outside, degen


def degenerate_scalars(t):
    """The odd k in [1, N) whose LAST column meets the doubling case, derived
    from the condition 2 m_1 == val_0 (mod N) with m_0 = 2 m_1 + val_0 = k:
    k == 2 val_0(k) (mod N), searched over the 2^t sign patterns of column 0.
    Each comes with the even u = N - k that is evaluated through it."""
    d, out = columns(t), []
    for pat in range(1 << t):
        v0 = sum((1 if (pat >> j) & 1 else -1) << (j * d) for j in range(t))
        k = 2 * v0 % N
        if not k & 1:
            continue
        b = digits(k, t)
        if all((b(j * d) > 0) == bool((pat >> j) & 1) for j in range(t)):
            out.append(k)
    return sorted(out)


def corner_scalars(t):
    """The corners for t teeth, all in [1, N): small and large values, single
    bits on both sides of every tooth boundary, all-same-sign columns, the
    ragged top."""
    d = columns(t)
    out = [1, 2, 3, N - 1, N - 2, N - 3, 1 << 255, (1 << 255) + 1]
    for j in range(1, t):
        for p in (j * d - 1, j * d, j * d + 1):
            if p < 256:
                out += [1 << p, (1 << p) + 1]
    for c in (0, 1, d // 2, d - 2):
        teeth = sum(1 << (j * d + c + 1) for j in range(t) if j * d + c + 1 < 256)
        out.append(teeth | 1)                    # column c all positive (where the bits exist)
        out.append(((1 << 255) - 1) & ~teeth | 1)  # column c all negative below the top
    out += [(1 << 256) - (1 << 224) - 1, (1 << 255) | 1, (1 << 254) | 1, N - (1 << 200)]  # the ragged top
    out += [k for k in degenerate_scalars(t)] + [N - k for k in degenerate_scalars(t)]
    return [u for u in out if 1 <= u < N]
