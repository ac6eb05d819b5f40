"""P-384 in plain Python integers: the restatement the P-384 class's tests
compare with.  Test infrastructure, not product code.

on_curve, hash_to_int and go_ecdsa_verify restate Go's crypto/ecdsa for a
384-bit order; ecdsa_sign is a deterministic signer for making vectors;
der_parse_sig48 is encoding/asn1's `struct { R, S *big.Int }` decode at width
48 (the rules of minbft_amd/csrc/der.cpp); scheme_status is
EcdsaSigCipher.Verify behind PublicAuthenScheme.VerifyAuthenticationTag with
the key given in the call.  rcb_add / rcb_dbl restate the complete formulas
the kernel runs (Renes-Costello-Batina, a = -3, homogeneous projective).
"""
import hashlib
import hmac

P = 2**384 - 2**128 - 2**96 + 2**32 - 1
N = 0xffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973
B = 0xb3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875ac656398d8a2ed19d2a85c8edd3ec2aef
GX = 0xaa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a385502f25dbf55296c3a545e3872760ab7
GY = 0x3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c00a60b1ce1d7e819d7a431d7c90ea0e5f
G = (GX, GY)

ACCEPT, REJECT, MALFORMED_DER, BAD_KEY = 0, 1, 2, 5

EMPTY_HASH = hashlib.sha256(b"").digest()
SPKI_PREFIX = bytes.fromhex("3076301006072a8648ce3d020106052b8104002203620004")


def on_curve(x, y):
    """elliptic.CurveParams.IsOnCurve (coordinates outside [0, p) are no point)."""
    if not (0 <= x < P and 0 <= y < P):
        return False
    return (y * y - (x * x * x - 3 * x + B)) % P == 0


def add(p1, p2):
    """Affine addition, None the point at infinity."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(p1):
    return None if p1 is None else (p1[0], (-p1[1]) % P)


def mul(k, p1):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p1)
    return acc


def pubkey(d):
    return mul(d % N, G)


def rcb_add(p1, p2):
    """Complete addition, algorithm 4 of Renes-Costello-Batina (a = -3),
    (X : Y : Z) with O = (0 : 1 : 0)."""
    (x1, y1, z1), (x2, y2, z2) = p1, p2
    t0, t1, t2 = x1 * x2 % P, y1 * y2 % P, z1 * z2 % P
    t3 = ((x1 + y1) * (x2 + y2) - t0 - t1) % P
    t4 = ((y1 + z1) * (y2 + z2) - t1 - t2) % P
    y3 = ((x1 + z1) * (x2 + z2) - t0 - t2) % P
    x3 = (y3 - B * t2) % P
    x3 = 3 * x3 % P
    z3 = (t1 - x3) % P
    x3 = (t1 + x3) % P
    y3 = (B * y3 - 3 * t2 - t0) % P
    y3 = 3 * y3 % P
    t0 = (3 * t0 - 3 * t2) % P
    t1 = t4 * y3 % P
    t2 = t0 * y3 % P
    y3 = (x3 * z3 + t2) % P
    x3 = (t3 * x3 - t1) % P
    z3 = (t4 * z3 + t3 * t0) % P
    return x3, y3, z3


def rcb_dbl(p1):
    """Complete doubling, algorithm 6 (a = -3)."""
    x, y, z = p1
    t0, t1, t2 = x * x % P, y * y % P, z * z % P
    t3 = 2 * x * y % P
    z3 = 2 * x * z % P
    y3 = (B * t2 - z3) % P
    y3 = 3 * y3 % P
    x3 = (t1 - y3) % P
    y3 = (t1 + y3) % P
    y3 = x3 * y3 % P
    x3 = x3 * t3 % P
    t2 = 3 * t2 % P
    z3 = (B * z3 - t2 - t0) % P
    z3 = 3 * z3 % P
    t0 = (3 * t0 - t2) % P
    t0 = t0 * z3 % P
    y3 = (y3 + t0) % P
    t0 = 2 * y * z % P
    z3 = t0 * z3 % P
    x3 = (x3 - z3) % P
    z3 = 4 * t0 * t1 % P
    return x3, y3, z3


def to_proj(p1):
    return (0, 1, 0) if p1 is None else (p1[0], p1[1], 1)


def to_affine(pr):
    x, y, z = pr
    if z % P == 0:
        return None
    zi = pow(z, -1, P)
    return x * zi % P, y * zi % P


def hash_to_int(md):
    """crypto/ecdsa hashToInt for a 384-bit order: the left-most 48 bytes, or
    the whole digest where it is shorter (no shift: 384 is a byte multiple)."""
    return int.from_bytes(md[:48], "big")


def e48(md):
    """The 48 big-endian bytes the prehashed entry points take for md."""
    return hash_to_int(md).to_bytes(48, "big")


def go_ecdsa_verify(q, e, r, s):
    """ecdsa.Verify(pub, hash, r, s) with e = hashToInt(hash) given as an
    integer in [0, 2^384); q a point on the curve."""
    if not (0 < r < N and 0 < s < N):
        return False
    w = pow(s, -1, N)
    u1, u2 = e * w % N, r * w % N
    pt = add(mul(u1, G), mul(u2, q))
    if pt is None:
        return False
    return pt[0] % N == r


def prehashed_status(x, y, e, r, s):
    """What the kernel answers for one item."""
    if not on_curve(x, y):
        return BAD_KEY
    return ACCEPT if go_ecdsa_verify((x, y), e, r, s) else REJECT


def _k_for(d, e, salt=b""):
    """A deterministic nonce in [1, N): HMAC-SHA-384 of the digest under the
    key (not RFC 6979; the vectors only need a fixed, well-spread k)."""
    c = 0
    while True:
        k = int.from_bytes(hmac.new(d.to_bytes(48, "big"), salt + e.to_bytes(48, "big") + bytes([c]),
                                    hashlib.sha384).digest(), "big") % N
        if k:
            return k
        c += 1


def ecdsa_sign(d, e, k=None):
    """(r, s) over e (an integer, e = hashToInt(hash)) under private key d."""
    c = 0
    while True:
        kk = k if k is not None else _k_for(d, e, bytes([c]))
        r = mul(kk, G)[0] % N
        s = pow(kk, -1, N) * (e + r * d) % N
        if r and s:
            return r, s
        assert k is None, "the given nonce yields r = 0 or s = 0"
        c += 1


class Asn1Error(Exception):
    pass


def _tag_len(b, off):
    if off >= len(b):
        raise Asn1Error("truncated")
    c = b[off]
    off += 1
    cls, compound, tag = c >> 6, bool(c & 0x20), c & 0x1F
    if tag == 0x1F:
        raise Asn1Error("high tag")
    if off >= len(b):
        raise Asn1Error("truncated")
    c = b[off]
    off += 1
    if not c & 0x80:
        return cls, compound, tag, c, off
    nb = c & 0x7F
    if nb == 0:
        raise Asn1Error("indefinite length")
    ln = 0
    for _ in range(nb):
        if off >= len(b):
            raise Asn1Error("truncated")
        if ln >= 1 << 23:
            raise Asn1Error("length too large")
        ln = ln << 8 | b[off]
        off += 1
        if ln == 0:
            raise Asn1Error("leading zeros")
    if ln < 0x80:
        raise Asn1Error("non-minimal length")
    return cls, compound, tag, ln, off


def _int_field(b, off):
    if off == len(b):
        raise Asn1Error("sequence truncated")
    cls, compound, tag, ln, off = _tag_len(b, off)
    if cls != 0 or tag != 2 or compound:
        raise Asn1Error("tags don't match")
    if ln > len(b) - off:
        raise Asn1Error("data truncated")
    v = b[off:off + ln]
    if ln == 0:
        raise Asn1Error("empty integer")
    if ln > 1 and ((v[0] == 0 and not v[1] & 0x80) or (v[0] == 0xFF and v[1] & 0x80)):
        raise Asn1Error("not minimally-encoded")
    return int.from_bytes(v, "big", signed=True), off + ln


def der_parse_sig(sig):
    """(r, s, consumed) as asn1.Unmarshal gives them (any integers)."""
    sig = bytes(sig)
    if not sig:
        raise Asn1Error("sequence truncated")
    cls, compound, tag, ln, off = _tag_len(sig, 0)
    if cls != 0 or tag != 16 or not compound:
        raise Asn1Error("tags don't match")
    if ln > len(sig) - off:
        raise Asn1Error("data truncated")
    inner = sig[off:off + ln]
    r, io = _int_field(inner, 0)
    s, io = _int_field(inner, io)
    return r, s, off + ln


def der_parse_sig48(sig):
    """mbft_der_parse_sig48: (r48, s48, consumed); a value outside (0, 2^384)
    goes on as zero (Verify rejects it either way)."""
    r, s, used = der_parse_sig(sig)
    w = lambda v: (v if 0 < v < 1 << 384 else 0).to_bytes(48, "big")  # noqa: E731
    return w(r), w(s), used


def der_int(v):
    b = v.to_bytes(v.bit_length() // 8 + 1, "big", signed=True) if v else b"\x00"
    ln = len(b)
    return b"\x02" + (bytes([ln]) if ln < 0x80 else b"\x81" + bytes([ln])) + b


def der_encode_sig(r, s):
    body = der_int(r) + der_int(s)
    ln = len(body)
    return b"\x30" + (bytes([ln]) if ln < 0x80 else b"\x81" + bytes([ln])) + body


def scheme_digest(msg):
    """md = m || SHA256("") (crypto.go:121)."""
    return bytes(msg) + EMPTY_HASH


def scheme_status(msg, tag, xy):
    """mbft_scheme_verify_p384_flat32 for one call."""
    try:
        r, s, _ = der_parse_sig(tag)
    except Asn1Error:
        return MALFORMED_DER
    x, y = int.from_bytes(xy[:48], "big"), int.from_bytes(xy[48:96], "big")
    return prehashed_status(x, y, hash_to_int(scheme_digest(msg)), r, s)


def pkix_encode(q):
    return SPKI_PREFIX + q[0].to_bytes(48, "big") + q[1].to_bytes(48, "big")
