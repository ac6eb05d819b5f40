"""Writes tests/golden/p384_edges.json: the P-384 class's vectors (DESIGN.md
§4.14), from a fixed seed, with tests/p384_ref.py as the only arithmetic.

    python tests/golden/make_p384_edges.py

Two kinds of vector.  "prehashed": e, r, s (48 bytes) and x, y (48 bytes each)
as hex, for mbft_verify_prehashed_p384_keys*.  "scheme": msg, tag, xy as hex,
for mbft_scheme_verify_p384_flat32.  Each carries the status the restatement
gives it (0 accept, 1 reject, 2 malformed DER, 5 bad key); what a group is
built to show is asserted here as well.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import p384_ref as o  # noqa: E402

ACCEPT, REJECT, MALFORMED, BAD_KEY = o.ACCEPT, o.REJECT, o.MALFORMED_DER, o.BAD_KEY
TOP = (1 << 384) - 1


def build():
    rng = random.Random(384)
    out = []

    def pre(label, e, r, s, x, y, want=None):
        st = o.prehashed_status(x, y, e, r, s)
        assert want is None or st == want, (label, st, want)
        out.append({"kind": "prehashed", "label": label, "e": "%096x" % e, "r": "%096x" % r, "s": "%096x" % s,
                    "x": "%096x" % x, "y": "%096x" % y, "status": st})

    def sch(label, msg, tag, xy, want=None):
        st = o.scheme_status(msg, tag, xy)
        assert want is None or st == want, (label, st, want)
        out.append({"kind": "scheme", "label": label, "msg": bytes(msg).hex(), "tag": bytes(tag).hex(),
                    "xy": bytes(xy).hex(), "status": st})

    # 64 keys: a valid signature each, and one corruption each (e, r, s or the key of the next)
    keys = [(d, o.pubkey(d)) for d in (rng.randrange(1, o.N) for _ in range(64))]
    for j, (d, q) in enumerate(keys):
        e = rng.getrandbits(384)
        r, s = o.ecdsa_sign(d, e)
        pre("valid %d" % j, e, r, s, *q, want=ACCEPT)
        kind = j % 4
        if kind == 0:
            pre("wrong e %d" % j, e ^ (1 << rng.randrange(384)), r, s, *q, want=REJECT)
        elif kind == 1:
            pre("wrong r %d" % j, e, r % (o.N - 1) + 1, s, *q, want=REJECT)
        elif kind == 2:
            pre("high s %d" % j, e, r, o.N - s, *q, want=ACCEPT)  # (r, -s) verifies as well
        else:
            pre("other key %d" % j, e, r, s, *keys[(j + 1) % 64][1], want=REJECT)

    # Q = G and Q = -G: G + Q is 2 G, or the point at infinity
    for name, d in (("Q = G", 1), ("Q = -G", o.N - 1)):
        q = o.pubkey(d)
        assert q == (o.G if d == 1 else o.neg(o.G))
        for t in range(3):
            e = rng.getrandbits(384)
            r, s = o.ecdsa_sign(d, e)
            pre("%s valid %d" % (name, t), e, r, s, *q, want=ACCEPT)
            pre("%s wrong e %d" % (name, t), e + 1, r, s, *q, want=REJECT)
    # u1 = u2 under Q = -G and u1 = -u2 under Q = G: the sum is the point at infinity
    for t in range(2):
        r, s = rng.randrange(1, o.N), rng.randrange(1, o.N)
        pre("Q = -G, u1 = u2 %d" % t, r, r, s, *o.neg(o.G), want=REJECT)
        pre("Q = G, u1 = -u2 %d" % t, o.N - r, r, s, *o.G, want=REJECT)

    # u1 = 0: e = 0 and e = N
    for t, e in enumerate((0, o.N, 0, o.N)):
        d, q = keys[t]
        r, s = o.ecdsa_sign(d, e)
        pre("u1 = 0 (e = %s) valid" % ("0" if e == 0 else "N"), e, r, s, *q, want=ACCEPT)
        pre("u1 = 0 (e = %s) wrong r" % ("0" if e == 0 else "N"), e, r ^ 1 or 2, s, *q)

    # u1 G = u2 Q (e = r d) and u1 G = -u2 Q (e = -r d), with the private key known
    for t in range(4):
        d, q = keys[8 + t]
        k = rng.randrange(1, o.N)
        r = o.mul(k, o.G)[0] % o.N
        e = r * d % o.N
        s = 2 * r * d * pow(k, -1, o.N) % o.N
        w = pow(s, -1, o.N)
        assert o.mul(e * w % o.N, o.G) == o.mul(r * w % o.N, q)
        pre("u1 G = u2 Q valid %d" % t, e, r, s, *q, want=ACCEPT)
        pre("u1 G = u2 Q wrong s %d" % t, e, r, s + 1 if s + 1 < o.N else 1, *q, want=REJECT)
        e = (-r * d) % o.N
        s = rng.randrange(1, o.N)
        w = pow(s, -1, o.N)
        assert o.add(o.mul(e * w % o.N, o.G), o.mul(r * w % o.N, q)) is None
        pre("u1 G = -u2 Q %d" % t, e, r, s, *q, want=REJECT)
        pre("u1 G = -u2 Q, e + N %d" % t, e + o.N if e + o.N <= TOP else e, r, s, *q, want=REJECT)

    # e >= N
    for t, e in enumerate((o.N + 5, TOP, o.N + rng.randrange(TOP - o.N), o.N + 1)):
        d, q = keys[16 + t]
        r, s = o.ecdsa_sign(d, e)
        pre("e >= N valid %d" % t, e, r, s, *q, want=ACCEPT)
        pre("e - N instead %d" % t, e - o.N, r, s, *q, want=ACCEPT)  # the same residue
        pre("e >= N wrong %d" % t, e - 1, r, s, *q, want=REJECT)

    # r or s at 0, N, N - 1, 2^384 - 1 under a good key
    d, q = keys[20]
    e = rng.getrandbits(384)
    r, s = o.ecdsa_sign(d, e)
    for v in (0, o.N, o.N - 1, TOP):
        name = {0: "0", o.N: "N", o.N - 1: "N - 1", TOP: "2^384 - 1"}[v]
        pre("r = %s" % name, e, v, s, *q, want=REJECT)
        pre("s = %s" % name, e, r, v, *q, want=REJECT)
    pre("r = s = 0", e, 0, 0, *q, want=REJECT)

    # x = r + N: the finish's second comparison.  r + N < p needs r < p - N (< 2^190), which no
    # honest nonce yields; the host and device harnesses inject it into the finish instead.

    # bad keys
    kk = 0
    while True:
        a = (kk ** 3 - 3 * kk + o.B) % o.P
        yy = pow(a, (o.P + 1) // 4, o.P)
        if yy * yy % o.P == a:
            break
        kk += 1
    assert o.on_curve(kk, yy) and o.P + kk <= TOP
    rk, sk = o.ecdsa_sign(rng.randrange(1, o.N), e)  # (any numbers in range)
    bad = [("X = p + k", o.P + kk, yy), ("X = p", o.P, q[1]), ("Y = p", q[0], o.P), ("X = 2^384 - 1", TOP, q[1]),
           ("Y = 2^384 - 1", q[0], TOP), ("(0, 0)", 0, 0), ("Y + 1", q[0], (q[1] + 1) % o.P),
           ("X + 1", (q[0] + 1) % o.P, q[1]), ("(X, X)", q[0], q[0]), ("Y = p + y", kk, o.P + yy if o.P + yy <= TOP else o.P)]
    for name, x, y in bad:
        pre("bad key %s" % name, e, r, s, x, y, want=BAD_KEY)
        pre("bad key %s, r = 0" % name, e, 0, s, x, y, want=BAD_KEY)
        pre("bad key %s, s = N" % name, e, r, o.N, x, y, want=BAD_KEY)
    pre("the small point is a key", e, rk, sk, kk, yy, want=REJECT)

    # ------------------------------------------------------------ the scheme form
    def xy(q_):
        return q_[0].to_bytes(48, "big") + q_[1].to_bytes(48, "big")

    bad_xy = xy((q[0], (q[1] + 1) % o.P))
    msgs = [b"", b"\x01", bytes(range(15)), bytes(range(16)), bytes(range(17)), b"REQ-VIEW-CHANGE:" + bytes(7),
            bytes(range(100)), bytes(47), bytes(range(48, 96)), b"\xff" * 15]
    assert [len(m) for m in msgs[:7]] == [0, 1, 15, 16, 17, 23, 100]
    for j, msg in enumerate(msgs):
        d, q_ = keys[24 + j]
        ee = o.hash_to_int(o.scheme_digest(msg))
        assert (ee.bit_length() <= 8 * (len(msg) + 32)) and (len(msg) >= 16 or ee == int.from_bytes(msg + o.EMPTY_HASH, "big"))
        rr, ss = o.ecdsa_sign(d, ee)
        tag = o.der_encode_sig(rr, ss)
        sch("valid %d B" % len(msg), msg, tag, xy(q_), want=ACCEPT)
        sch("trailing %d B" % len(msg), msg, tag + b"\x00\x01trailing", xy(q_), want=ACCEPT)
        sch("other key %d B" % len(msg), msg, tag, xy(keys[25 + j][1]), want=REJECT)
        sch("bad key %d B" % len(msg), msg, tag, bad_xy, want=BAD_KEY)
        if msg:
            t = bytearray(msg)
            t[(3 * j) % min(len(msg), 48)] ^= 1
            sch("tamper in e %d B" % len(msg), t, tag, xy(q_), want=REJECT)
        if len(msg) > 48:
            t = bytearray(msg)
            t[48 + j % (len(msg) - 48)] ^= 0x40
            sch("tamper past e %d B" % len(msg), t, tag, xy(q_), want=ACCEPT)
    d, q_ = keys[40]
    msg = msgs[5]
    ee = o.hash_to_int(o.scheme_digest(msg))
    rr, ss = o.ecdsa_sign(d, ee)
    tag = o.der_encode_sig(rr, ss)
    malformed = [b"", tag[:-1], tag[:5], b"\x31" + tag[1:], b"\x30\x80" + tag[2:], tag[:2] + b"\x03" + tag[3:],
                 b"\x30\x81" + tag[1:], o.der_encode_sig(rr, ss)[:2] + b"\x02\x00" + o.der_int(ss),
                 b"\x30\x06\x02\x02\x00\x01\x02\x00", b"\x30\x08\x02\x02\x00\x7f\x02\x02\x00\x01",
                 b"\x30\x08\x02\x02\xff\x80\x02\x02\x00\x81", b"\x30\x03\x02\x01\x01", b"\x1f" + tag[1:],
                 bytes([0x30, len(o.der_int(rr))]) + o.der_int(rr)]
    for j, t in enumerate(malformed):
        sch("malformed %d" % j, msg, t, xy(q_), want=MALFORMED)
        if j % 3 == 0:
            sch("malformed %d, bad key" % j, msg, t, bad_xy, want=MALFORMED)
    # well-formed tags whose numbers are out of range
    big = rng.getrandbits(384) | 1 << 383
    for name, a, b in (("r in [2^256, 2^384)", (1 << 256) + 12345, ss), ("s in [2^256, 2^384)", rr, big % o.N or 1),
                       ("r = 2^384", 1 << 384, ss), ("s >= 2^384", rr, (1 << 400) + 7), ("r = N", o.N, ss),
                       ("r negative", -rr, ss), ("s negative", rr, -1), ("r = 0", 0, ss), ("s = 0", rr, 0)):
        sch("foreign %s" % name, msg, o.der_encode_sig(a, b), xy(q_), want=REJECT)
        if name.startswith("r ="):
            sch("foreign %s, bad key" % name, msg, o.der_encode_sig(a, b), bad_xy, want=BAD_KEY)
    # extra bytes inside the SEQUENCE after S are ignored too
    body = o.der_int(rr) + o.der_int(ss) + b"\x05\x00"
    sch("extra field inside", msg, b"\x30" + bytes([len(body)]) + body, xy(q_), want=ACCEPT)
    return out


def main():
    vecs = build()
    assert len(vecs) <= 400, len(vecs)
    path = os.path.join(HERE, "p384_edges.json")
    with open(path, "w") as f:
        json.dump(vecs, f, indent=0, sort_keys=True)
        f.write("\n")
    counts = {}
    for v in vecs:
        counts[(v["kind"], v["status"])] = counts.get((v["kind"], v["status"]), 0) + 1
    print(len(vecs), "vectors", sorted(counts.items()), hashlib.sha256(open(path, "rb").read()).hexdigest()[:16])


if __name__ == "__main__":
    main()
