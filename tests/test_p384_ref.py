"""tests/p384_ref.py, the Python restatement the P-384 class is tested against
(DESIGN.md §4.14), agrees with OpenSSL libcrypto's secp384r1 (ECDSA_do_verify,
NID 715, through ctypes as oracle/openssl_xcheck.py does for P-256): on every
vector of tests/golden/p384_edges.json that OpenSSL will take, on random
ones, on the scheme form's digests for short messages, and on the SPKI prefix.
The fixture file is what tests/golden/make_p384_edges.py writes.  No GPU."""
import ctypes
import json
import os
import random

import pytest

import p384_ref as o

HERE = os.path.dirname(os.path.abspath(__file__))
NID_SECP384R1 = 715


@pytest.fixture(scope="module")
def crypto():
    from oracle import openssl_xcheck
    lib = openssl_xcheck.load()
    assert lib is not None, "libcrypto is needed for this cross-check"
    lib.i2d_EC_PUBKEY.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_ubyte))]
    lib.i2d_EC_PUBKEY.restype = ctypes.c_int
    return lib


def _bn(lib, x):
    b = x.to_bytes(max(1, (x.bit_length() + 7) // 8), "big")
    return lib.BN_bin2bn(b, len(b), None)


def ossl_verify(lib, x, y, digest, r, s):
    """True / False, or None where OpenSSL refuses the key."""
    key = lib.EC_KEY_new_by_curve_name(NID_SECP384R1)
    assert key
    bx, by = _bn(lib, x), _bn(lib, y)
    try:
        if lib.EC_KEY_set_public_key_affine_coordinates(key, bx, by) != 1:
            return None
        sig = lib.ECDSA_SIG_new()
        assert lib.ECDSA_SIG_set0(sig, _bn(lib, r), _bn(lib, s)) == 1
        rc = lib.ECDSA_do_verify(digest, len(digest), sig, key)
        lib.ECDSA_SIG_free(sig)
        return rc == 1  # (an r or s out of range is an error there, false in Go)
    finally:
        lib.BN_free(bx)
        lib.BN_free(by)
        lib.EC_KEY_free(key)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "p384_edges.json")) as f:
        return json.load(f)


def test_fixture_is_the_generators(vectors):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_p384_edges", os.path.join(HERE, "golden", "make_p384_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.build() == vectors
    assert len(vectors) <= 400
    labels = " | ".join(v["label"] for v in vectors)
    for needle in ("Q = G", "Q = -G", "u1 = 0", "u1 G = u2 Q", "u1 G = -u2 Q", "e >= N", "r = N - 1", "s = 2^384 - 1",
                   "X = p + k", "(0, 0)", "valid 0 B", "valid 1 B", "valid 15 B", "valid 16 B", "valid 17 B",
                   "valid 23 B", "valid 100 B", "trailing", "malformed", "[2^256, 2^384)", ">= 2^384"):
        assert needle in labels, needle
    assert len({(v["x"], v["y"]) for v in vectors if v["kind"] == "prehashed" and v["status"] == 0}) >= 64


def test_fixture_vectors_against_libcrypto(crypto, vectors):
    taken = refused = 0
    for v in vectors:
        if v["kind"] == "prehashed":
            x, y, r, s = (int(v[k], 16) for k in "xyrs")
            digest = bytes.fromhex(v["e"])
        else:
            try:
                r, s, _ = o.der_parse_sig(bytes.fromhex(v["tag"]))
            except o.Asn1Error:
                assert v["status"] == o.MALFORMED_DER, v["label"]
                continue
            xy = bytes.fromhex(v["xy"])
            x, y = int.from_bytes(xy[:48], "big"), int.from_bytes(xy[48:], "big")
            digest = o.scheme_digest(bytes.fromhex(v["msg"]))
            assert o.hash_to_int(digest) == int.from_bytes(digest[:48], "big")
        if r < 0 or s < 0:  # (a BIGNUM made from bytes has no sign: OpenSSL cannot be asked)
            assert v["status"] in (o.REJECT, o.BAD_KEY), v["label"]
            continue
        got = ossl_verify(crypto, x, y, digest, r, s)
        if got is None:
            refused += 1
            assert v["status"] == o.BAD_KEY and not o.on_curve(x, y), v["label"]
        else:
            taken += 1
            assert o.on_curve(x, y) and v["status"] == (o.ACCEPT if got else o.REJECT), v["label"]
    assert taken + refused >= 270 and taken >= 200 and refused >= 30


def test_random_vectors_against_libcrypto(crypto):
    rng = random.Random(3840)
    keys = [(d, o.pubkey(d)) for d in (rng.randrange(1, o.N) for _ in range(8))]
    n = accepted = 0
    for t in range(208):
        d, q = keys[t % 8]
        digest = rng.randbytes(rng.choice((48, 48, 48, 64, 33, 32, 20, 1)))
        e = o.hash_to_int(digest)
        r, s = o.ecdsa_sign(d, e)
        kind = t % 4
        if kind == 1:
            digest = bytes([digest[0] ^ 1]) + digest[1:]
        elif kind == 2:
            r = rng.randrange(1, o.N)
        elif kind == 3 and t % 8 == 3:
            q = keys[(t + 1) % 8][1]
        want = o.go_ecdsa_verify(q, o.hash_to_int(digest), r, s)
        assert ossl_verify(crypto, q[0], q[1], digest, r, s) == want, t
        n += 1
        accepted += want
    assert n >= 200 and 60 <= accepted <= 140


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 23, 47, 48, 100])
def test_scheme_digest_against_libcrypto(crypto, length):
    """e for md = m || SHA256(""): the whole of md as an integer for messages
    under 16 bytes, md[0:48] from there on -- what libcrypto signs under."""
    rng = random.Random(length)
    msg = rng.randbytes(length)
    md = o.scheme_digest(msg)
    e = o.hash_to_int(md)
    assert e == (int.from_bytes(md, "big") if length < 16 else int.from_bytes(md[:48], "big"))
    assert o.e48(md) == (md.rjust(48, b"\0") if length < 16 else md[:48])
    d = rng.randrange(1, o.N)
    q = o.pubkey(d)
    r, s = o.ecdsa_sign(d, e)
    assert ossl_verify(crypto, q[0], q[1], md, r, s) is True
    assert o.scheme_status(msg, o.der_encode_sig(r, s), o.pkix_encode(q)[24:]) == o.ACCEPT
    if length:
        other = bytes([msg[0] ^ 0x80]) + msg[1:]
        assert ossl_verify(crypto, q[0], q[1], o.scheme_digest(other), r, s) is False
        assert o.scheme_status(other, o.der_encode_sig(r, s), o.pkix_encode(q)[24:]) == o.REJECT


def test_spki_prefix_is_libcryptos(crypto):
    q = o.pubkey(0x384)
    key = crypto.EC_KEY_new_by_curve_name(NID_SECP384R1)
    bx, by = _bn(crypto, q[0]), _bn(crypto, q[1])
    try:
        assert crypto.EC_KEY_set_public_key_affine_coordinates(key, bx, by) == 1
        buf = ctypes.POINTER(ctypes.c_ubyte)()
        n = crypto.i2d_EC_PUBKEY(key, ctypes.byref(buf))
        assert n == 120
        der = bytes(buf[:n])
    finally:
        crypto.BN_free(bx)
        crypto.BN_free(by)
        crypto.EC_KEY_free(key)
    assert der == o.pkix_encode(q)
    assert der[:23] == bytes.fromhex("3076301006072a8648ce3d020106052b8104002203620004")[:23] and der[23] == 4
