"""Makes tests/golden/sign_edges.json: four (d, e) pairs whose deterministic
(RFC 6979) signature has a SHORT r or s -- 31 value bytes after the leading
zero byte is stripped -- once with and once without the 0x00 pad DER then puts
back (top bit of the first remaining byte set / clear).  These are the length
cases of the batch signer's DER encoder that random inputs hit once in 256.

Search: d = SHA256("sign-edges") mod N, e_i = SHA256("e%d" % i), i = 0, 1, ...
with oracle.ecdsa_sign; the first hit of each case is kept.

    python tests/golden/make_sign_edges.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import p256 as o  # noqa: E402


def case_of(r, s):
    for name, v in (("r", r), ("s", s)):
        b = v.to_bytes(32, "big")
        if b[0] == 0 and b[1] != 0:
            return "%s31_%s" % (name, "pad" if b[1] & 0x80 else "nopad")
    return None


def main():
    d = int.from_bytes(hashlib.sha256(b"sign-edges").digest(), "big") % o.N
    want = ["r31_pad", "r31_nopad", "s31_pad", "s31_nopad"]
    found = {}
    i = 0
    while len(found) < len(want):
        e = hashlib.sha256(b"e%d" % i).digest()
        r, s = o.ecdsa_sign(d, e)
        c = case_of(r, s)
        if c in want and c not in found:
            found[c] = {"case": c, "i": i, "d": "%064x" % d, "e": e.hex(), "r": "%064x" % r,
                        "s": "%064x" % s, "tag": o.der_encode_sig(r, s).hex()}
        i += 1
    with open(os.path.join(HERE, "sign_edges.json"), "w") as f:
        json.dump([found[c] for c in want], f, indent=1)
        f.write("\n")
    print("searched", i, "digests")


if __name__ == "__main__":
    main()
