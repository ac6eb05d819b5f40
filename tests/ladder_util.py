"""Scalars and the integer model shared by the table-free ladder's tests
(tests/test_ladder_host.py) and its fixture script
(tests/golden/make_ladder_edges.py)."""
from oracle import p256 as o

N = o.N

#: the scalars in [1, N) whose ladder meets a degenerate addition
#: (minbft_amd/csrc/ladder_dev.h gives the argument): the last step of
#: u = N - 2 adds -Q to (N - 1) Q = -Q
DEGENERATE = (N - 2,)


def named_scalars():
    """The corner scalars of the issue's list, all in [1, N)."""
    pat5 = int("55" * 32, 16) % N
    pata = int("aa" * 32, 16) % N
    return [1, 2, 3, 4, N - 1, N - 2, N - 3, (N + 1) // 2, (N - 1) // 2,
            1 << 255, (1 << 255) + 1, (1 << 255) - 1, pat5, pata]


def power_scalars():
    """Every 2^k and 2^k - 1 in [1, N)."""
    out = []
    for k in range(257):
        for v in ((1 << k), (1 << k) - 1):
            if 1 <= v < N:
                out.append(v)
    return out


def naf(u):
    """Reference non-adjacent form of u >= 0, least significant digit first."""
    d = []
    while u:
        if u & 1:
            z = 2 - (u & 3)
            u -= z
        else:
            z = 0
        d.append(z)
        u >>= 1
    return d


def model_degenerate_steps(digits_top_down):
    """The integer model of the ladder over digits given from the top down:
    the steps (index, prefix m before the addition, digit d) at which an
    addition to a finite accumulator has m == +-d (mod N)."""
    m, hits = 0, []
    for j, d in enumerate(digits_top_down):
        m *= 2
        if d == 0:
            continue
        if m % N != 0 and ((m - d) % N == 0 or (m + d) % N == 0):
            hits.append((j, m, d))
        m += d
    return hits, m
