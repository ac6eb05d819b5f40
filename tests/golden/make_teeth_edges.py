"""Makes tests/golden/teeth_edges.json: prehashed vectors (the format of
prehashed.json and ladder_edges.json) crafted from chosen (u1, u2) for the
compact key class, whose doubling comb computes u2 Q column by column
(minbft_amd/csrc/teeth_dev.h: t teeth, d = ceil(256 / t) columns).

For a target (u1, u2) under key Q: R = u1 G + u2 Q, r = R.x mod N,
s = r / u2, e = u1 s (mod N) -- so ecdsa.Verify recomputes exactly u1 and u2
and accepts; the same vector with r + 1 in place of r rejects.  A target
whose R is infinity gets an arbitrary r and rejects.  Every vector is
asserted against oracle.go_ecdsa_verify ("expect": 1 accept, 0 reject).

Targets, for each t in 2..8, u2 with
  * only the top tooth set;
  * only column 0 set (the accumulator stays at infinity until the last step);
  * an all-ones column;
  * a zero column between nonzero ones;
  * the ragged top (t = 3, 5, 6, 7: the top tooth is shorter than d bits):
    bit 255 set, so the top tooth's highest existing column is used;
and N - 1, N - 2 once; u1 in {0, 1, N - 1, random}.  Then the keys Q = G and
Q = -G with the pairs that make the join a doubling (accept) and the pairs
that sum to infinity (reject).

    python tests/golden/make_teeth_edges.py
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import p256 as o  # noqa: E402
from teeth_util import TEETH, column_values, columns  # noqa: E402

N = o.N


def craft(label, q, u1, u2, rng):
    """The accepting vector of (u1, u2) under q and its r + 1 twin, or one
    rejecting vector when u1 G + u2 Q is infinity."""
    assert 0 < u2 < N and 0 <= u1 < N
    R = o.combined_mult(u1, u2, q)
    out = []
    if R is None:
        r = rng.randrange(1, N)
        s = r * pow(u2, -1, N) % N
        cases = [(label + ":inf", r, 0)]
    else:
        r = R[0] % N
        assert r != 0
        s = r * pow(u2, -1, N) % N
        cases = [(label, r, 1), (label + ":r+1", r + 1, 0)]
    e = (u1 * s % N).to_bytes(32, "big")
    for lab, rr, expect in cases:
        assert 0 < rr < N and 0 < s < N
        assert o.go_ecdsa_verify(q, e, rr, s) == (expect == 1), lab
        if expect == 1:
            w = pow(s, -1, N)
            assert (int.from_bytes(e, "big") * w % N, rr * w % N) == (u1, u2)
        out.append({"label": lab, "qx": "%064x" % q[0], "qy": "%064x" % q[1], "e": e.hex(),
                    "r": "%064x" % rr, "s": "%064x" % s, "expect": expect})
    return out


def targets(t, rng):
    """(name, u2) for t teeth; each asserted to have the shape it is named for."""
    d = columns(t)
    topw = 256 - (t - 1) * d  # bits of the top tooth
    out = []
    u = (rng.getrandbits(topw - 1) | 1) << ((t - 1) * d)
    assert all(v in (0, 1 << (t - 1)) for v in column_values(u, t))
    out.append(("top-tooth", u))
    u = sum(1 << (j * d) for j in range(t) if j % 2 == 0 or j == t - 1)
    cols = column_values(u, t)
    assert not any(cols[:-1]) and cols[-1]
    out.append(("column0", u))
    c = 3
    u = rng.getrandbits(255) | sum(1 << (j * d + c) for j in range(t))
    assert column_values(u, t)[d - 1 - c] == (1 << t) - 1
    out.append(("all-ones-column", u))
    c = 5
    u = rng.getrandbits(255) & ~sum(1 << (j * d + c) for j in range(t)) | (1 << (c - 1)) | (1 << (d + c + 1))
    cols = column_values(u, t)
    assert cols[d - 1 - c] == 0 and cols[d - c] and cols[d - 2 - c]
    out.append(("zero-column", u))
    if t * d > 256:
        u = (1 << 255) | rng.getrandbits(254)
        cols = column_values(u, t)
        assert cols[d - topw] >> (t - 1) == 1 and all(v >> (t - 1) == 0 for v in cols[:d - topw])
        out.append(("ragged-top", u))
    assert all(0 < u < N for _, u in out)
    return out


def main():
    rng = random.Random(0x7ee7ed9e)
    d = int.from_bytes(hashlib.sha256(b"teeth-edges").digest(), "big") % N
    q = o.pubkey(d)
    vecs = []
    for t in TEETH:
        for name, u2 in targets(t, rng):
            for u1 in (0, 1, N - 1, rng.randrange(1, N)):
                vecs += craft("u2=%s,t=%d,u1=%x" % (name, t, u1), q, u1, u2, rng)
    for u2 in (N - 1, N - 2):
        for u1 in (0, 1, N - 1, rng.randrange(1, N)):
            vecs += craft("u2=%x,u1=%x" % (u2, u1), q, u1, u2, rng)
    g, ng = o.G, o.point_neg(o.G)
    for u in (1, 2, N - 2, rng.randrange(1, N)):
        vecs += craft("Q=G,u1=u2=%x" % u, g, u, u, rng)            # u G + u G: the join doubles
        vecs += craft("Q=G,u1=-u2=%x" % u, g, u, N - u, rng)       # infinity
        vecs += craft("Q=-G,u1=-u2=%x" % u, ng, u, N - u, rng)     # u G + u G again
        vecs += craft("Q=-G,u1=u2=%x" % u, ng, u, u, rng)          # infinity
    assert len(vecs) <= 400
    with open(os.path.join(HERE, "teeth_edges.json"), "w") as f:
        json.dump(vecs, f, indent=0)
        f.write("\n")
    print(len(vecs), "vectors,", sum(v["expect"] == 1 for v in vecs), "accepting")


if __name__ == "__main__":
    main()
