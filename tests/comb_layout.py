"""The comb-table layout (k_table_fill; the signer's generator table has the
same one) as plain Python over oracle/p256.py, shared by
tests/test_gpu_tables.py, which verifies the product's table build against
it entry by entry, and tests/test_gpu_sign_dev.py, which hands sign_comb a
table made here so that its checks do not depend on that build.

Entry (win, d), d >= 1, lies at index (win << (W - 1)) + d - 1 and holds
x 2^261 mod p, then y 2^261 mod p (canonical Montgomery form, 8 little-endian
words each) of the affine point (d 2^(W win) mod N) P."""
import random

from oracle import p256 as o

R = 1 << 261


def steps(W):
    return -(-256 // W)


def last_bits(W):
    return 256 - (steps(W) - 1) * W


def entries(W):
    return ((steps(W) - 1) << (W - 1)) + (1 << last_bits(W))


def window_entries(W, win):
    return 1 << (last_bits(W) if win == steps(W) - 1 else W - 1)


def entry_bytes(pt):
    return (pt[0] * R % o.P).to_bytes(32, "little") + (pt[1] * R % o.P).to_bytes(32, "little")


def window_bases(p, W):
    """2^(W win) P for every window."""
    out, b = [], p
    for _ in range(steps(W)):
        out.append(b)
        for _ in range(W):
            b = o.point_add(b, b)
    return out


def structured_scalars(W, edges=(), nrandom=200, seed=0x5CA1A):
    """(name, k) with 1 <= k < N: the scalars at which a low-to-high signed
    comb of window W changes state -- a long stay at infinity, then the entry
    itself (2^(W j)); a carry chain from window 0 up to window j
    (2^(W j) - 1); a run of zero digits between two nonzero windows
    (2^(W j) + 1); the tie digit 2^(W-1) and the first negative digit after it
    in a low, a middle and the last recoded window; the top window alone, its
    largest digit below N, a carry through every window into it; `edges`
    ((name, u) pairs, reduced into [1, N)); and `nrandom` random ones (the
    same for every W).  Names starting with "pow" and "rnd" are the large
    families; every other name is a single case."""
    N = o.N
    S = steps(W)
    top = W * (S - 1)
    out = [("1", 1), ("2", 2), ("3", 3), ("N-1", N - 1), ("N-2", N - 2), ("(N-1)/2", (N - 1) // 2),
           ("(N+1)/2", (N + 1) // 2)]
    for j in range(S):
        b = 1 << (W * j)
        out += [(f"pow{j}", b), (f"pow{j}-1", b - 1), (f"pow{j}+1", b + 1)]
    t = 1 << (W - 1)
    for j in (0, S // 2, S - 2):
        out += [(f"tie@{j}", t << (W * j)), (f"tie+1@{j}", (t + 1) << (W * j))]
    out.append(("top_only", 1 << top))
    out.append(("top_largest", (N >> top) << top))
    out.append(("carry_through", (1 << 255) - 1))
    out += [("edge_" + name, u % N or 1) for name, u in edges]
    rng = random.Random(seed)
    out += [(f"rnd{i}", rng.randrange(1, N)) for i in range(nrandom)]
    out = [(name, k) for name, k in out if k != 0]
    assert all(1 <= k < N for _, k in out)
    return out


def table_bytes(p, W):
    """The whole table of the point p for window W."""
    out = bytearray()
    for win, b in enumerate(window_bases(p, W)):
        acc = b
        n = window_entries(W, win)
        for d in range(1, n + 1):
            out += entry_bytes(acc)
            if d < n:
                acc = o.point_add(acc, b)
    assert len(out) == 64 * entries(W)
    return bytes(out)
