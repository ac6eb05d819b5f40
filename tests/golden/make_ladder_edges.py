"""Makes tests/golden/ladder_edges.json: prehashed vectors (the format of
prehashed.json) crafted from chosen (u1, u2) for the table-free key class,
whose ladder computes u2 Q digit by digit (minbft_amd/csrc/ladder_dev.h).

For a target (u1, u2) under key Q: R = u1 G + u2 Q, r = R.x mod N,
s = r / u2, e = u1 s (mod N) -- so ecdsa.Verify recomputes exactly u1 and u2
and accepts; the same vector with r + 1 in place of r rejects.  A target
whose R is infinity gets an arbitrary r and rejects.  Every vector is
asserted against oracle.go_ecdsa_verify ("expect": 1 accept, 0 reject, as in
prehashed.json).

Targets: the corner scalars of tests/ladder_util.py as u2 (the degenerate
scalar N - 2 of the recoding among them) with u1 in {0, 1, N - 1, random};
2^k and 2^k - 1 for every eighth k with a random u1; the keys Q = G and
Q = -G with the pairs that make the join a doubling (accept) and the pairs
that sum to infinity (reject).

    python tests/golden/make_ladder_edges.py
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
from ladder_util import DEGENERATE, named_scalars  # noqa: E402

N = o.N


def craft(label, q, u1, u2, rng):
    """The accepting vector of (u1, u2) under q and its r + 1 twin, or one
    rejecting vector when u1 G + u2 Q is infinity."""
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


def main():
    rng = random.Random(0x1adde7ed)
    d = int.from_bytes(hashlib.sha256(b"ladder-edges").digest(), "big") % N
    q = o.pubkey(d)
    vecs = []
    names = named_scalars()
    for u2 in names + [u for u in DEGENERATE if u not in names]:
        for u1 in (0, 1, N - 1, rng.randrange(1, N)):
            vecs += craft("u2=%x,u1=%x" % (u2, u1), q, u1, u2, rng)
    for k in range(0, 257, 8):
        for u2 in ((1 << k), (1 << k) - 1):
            if 1 <= u2 < N:
                vecs += craft("u2=2^%d%s" % (k, "" if u2 == 1 << k else "-1"), q, rng.randrange(1, N), u2, rng)
    g, ng = o.G, o.point_neg(o.G)
    for u in (1, 2, N - 2, rng.randrange(1, N)):
        vecs += craft("Q=G,u1=u2=%x" % u, g, u, u, rng)            # u G + u G: the join doubles
        vecs += craft("Q=G,u1=-u2=%x" % u, g, u, N - u, rng)       # infinity
        vecs += craft("Q=-G,u1=-u2=%x" % u, ng, u, N - u, rng)     # u G + u G again
        vecs += craft("Q=-G,u1=u2=%x" % u, ng, u, u, rng)          # infinity
    with open(os.path.join(HERE, "ladder_edges.json"), "w") as f:
        json.dump(vecs, f, indent=0)
        f.write("\n")
    print(len(vecs), "vectors,", sum(v["expect"] == 1 for v in vecs), "accepting")


if __name__ == "__main__":
    main()
