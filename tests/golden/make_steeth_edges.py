"""Makes tests/golden/steeth_edges.json: prehashed vectors (the format of
prehashed.json and teeth_edges.json) crafted from chosen (u1, u2) for the
SIGNED compact key class, whose comb evaluates k = u2 (odd) or N - u2 (even)
column by column over a signed all-nonzero recoding
(minbft_amd/csrc/teeth_dev.h: t = 2..9 teeth, d = ceil(256 / t) columns).

For a target (u1, u2) under key Q: R = u1 G + u2 Q, r = R.x mod N,
s = r / u2, e = u1 s (mod N) -- so ecdsa.Verify recomputes exactly u1 and u2
and accepts; the same vector with r + 1 in place of r rejects.  A target
whose R is infinity gets an arbitrary r and rejects.  Every vector is
asserted against oracle.go_ecdsa_verify ("expect": 1 accept, 0 reject).

Targets, u2 being
  * for each t: each scalar whose LAST column meets the doubling case -- the
    odd k with k == 2 val_0(k) (mod N) and the even N - k that is evaluated
    through it -- re-derived here from that condition
    (steeth_util.degenerate_scalars: two scalars each for t = 2, 3, 8, 9);
  * 1, 2, N - 1, N - 2;
  * for each t: a scalar with an all-positive column and one with an
    all-negative column (both read the table's last entry), and, where t d >
    256, one whose top tooth's digits at positions >= 256 matter (bit 255 set);
with u1 in {0, random}, u1 = u2 d (u1 G == u2 Q: the join doubles) and u1 =
-u2 d (infinity) for the key's own d.  Then the keys Q = G and Q = -G with
the pairs that make the join a doubling (accept) and the pairs that sum to
infinity (reject).

    python tests/golden/make_steeth_edges.py
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from make_teeth_edges import craft  # noqa: E402
from oracle import p256 as o  # noqa: E402
from steeth_util import STEETH, column_list, columns, degenerate_scalars, flip, model  # noqa: E402

N = o.N


def targets(t, rng):
    """(name, u2) for t teeth; each asserted to have the shape it is named for."""
    d = columns(t)
    last = (1 << (t - 1)) - 1
    out = []
    for k in degenerate_scalars(t):
        for name, u in (("degenerate-odd", k), ("degenerate-even", N - k)):
            kk, flipped = flip(u)
            _, outside, degen = model(column_list(kk, t), t)
            assert kk == k and flipped == (name == "degenerate-even")
            assert not outside and [s for s, _, _ in degen] == [d - 1]
            out.append((name, u))
    c = 3
    teeth = sum(1 << (j * d + c + 1) for j in range(t))
    u = rng.getrandbits(250) | teeth | 1
    assert column_list(u, t)[d - 1 - c] == (last, False)
    out.append(("all-positive-column", u))
    u = (rng.getrandbits(250) & ~teeth) | 1
    assert column_list(u, t)[d - 1 - c] == (last, True)
    out.append(("all-negative-column", u))
    if t * d > 256:
        u = (1 << 255) | rng.getrandbits(254) | 1
        cols = column_list(u, t)
        # the top tooth's digits at positions >= 256 are -1 below the forced top digit
        assert cols[0][1] is False and cols[1][1] is True
        out.append(("ragged-top", u))
        out.append(("ragged-top-even", N - u))
    assert all(0 < u < N for _, u in out)
    return out


def main():
    rng = random.Random(0x51ee7ed9e)
    d = int.from_bytes(hashlib.sha256(b"steeth-edges").digest(), "big") % N
    q = o.pubkey(d)
    vecs = []

    def under_key(name, u2):
        for u1 in (0, rng.randrange(1, N), u2 * d % N, (N - u2) * d % N):
            vecs.extend(craft("u2=%s,u1=%x" % (name, u1), q, u1, u2, rng))

    for t in STEETH:
        for name, u2 in targets(t, rng):
            under_key("%s,t=%d" % (name, t), u2)
    for u2 in (1, 2, N - 1, N - 2):
        under_key("%x" % u2, u2)
    g, ng = o.G, o.point_neg(o.G)
    for u in (1, 2, N - 2, rng.randrange(1, N)):
        vecs += craft("Q=G,u1=u2=%x" % u, g, u, u, rng)            # u G + u G: the join doubles
        vecs += craft("Q=G,u1=-u2=%x" % u, g, u, N - u, rng)       # infinity
        vecs += craft("Q=-G,u1=-u2=%x" % u, ng, u, N - u, rng)     # u G + u G again
        vecs += craft("Q=-G,u1=u2=%x" % u, ng, u, u, rng)          # infinity
    assert 200 <= len(vecs) <= 400
    with open(os.path.join(HERE, "steeth_edges.json"), "w") as f:
        json.dump(vecs, f, indent=0)
        f.write("\n")
    print(len(vecs), "vectors,", sum(v["expect"] == 1 for v in vecs), "accepting")


if __name__ == "__main__":
    main()
