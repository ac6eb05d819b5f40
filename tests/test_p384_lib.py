"""The P-384 class's host-only entry points through the library (DESIGN.md
§4.14): mbft_der_parse_sig48 accepts exactly the vectors of
tests/golden/der.json that mbft_der_parse_sig accepts, with the same
`consumed`, and gives the reference's values at width 48; mbft_pkix_parse_p384
accepts the 120-byte SPKI of a point on the curve and nothing else.  No GPU."""
import ctypes

import numpy as np
import pytest

import p384_ref as o
from golden_util import load


@pytest.fixture(scope="module")
def lib():
    from minbft_amd import build, _lib
    build.build()
    return _lib.load()


def parse(lib, fn, width, sig):
    r = np.full(width + 8, 0xEE, dtype=np.uint8)
    s = np.full(width + 8, 0xEE, dtype=np.uint8)
    used = ctypes.c_size_t(12345)
    buf = (ctypes.c_uint8 * max(1, len(sig))).from_buffer_copy(bytes(sig) or b"\0")
    ok = fn(buf, len(sig), ctypes.c_void_p(r.ctypes.data), ctypes.c_void_p(s.ctypes.data), ctypes.byref(used))
    assert (r[width:] == 0xEE).all() and (s[width:] == 0xEE).all()
    return ok, bytes(r[:width]), bytes(s[:width]), used.value


def test_der48_follows_der32_on_the_golden_set(lib):
    vecs = load("der.json")
    sigs = [bytes.fromhex(v["sig"]) for v in vecs]
    sigs += [bytes.fromhex(v["tag"]) for v in o_fixtures() if v["kind"] == "scheme"]
    accepted = 0
    for sig in sigs:
        ok32, r32, s32, used32 = parse(lib, lib.mbft_der_parse_sig, 32, sig)
        ok48, r48, s48, used48 = parse(lib, lib.mbft_der_parse_sig48, 48, sig)
        assert ok48 == ok32, sig.hex()
        try:
            want = o.der_parse_sig48(sig)
        except o.Asn1Error:
            want = None
        assert (want is not None) == bool(ok48), sig.hex()
        if not ok48:
            assert r48 == bytes(48) and s48 == bytes(48)
            continue
        accepted += 1
        assert used48 == used32 and (r48, s48, used48) == want, sig.hex()
        # where the value fits 32 bytes the two widths hold the same number
        for a32, a48 in ((r32, r48), (s32, s48)):
            if int.from_bytes(a48, "big") < 1 << 256:
                assert a48 == bytes(16) + a32
            else:
                assert a32 == bytes(32)
    assert accepted >= 50
    assert sum(v["ok"] for v in vecs) == sum(parse(lib, lib.mbft_der_parse_sig48, 48, bytes.fromhex(v["sig"]))[0] for v in vecs)


def o_fixtures():
    import p384_ops_util
    return p384_ops_util.fixtures()


def test_der48_widths(lib):
    fn = lib.mbft_der_parse_sig48
    big = (1 << 383) + 0x1234
    for r, s in ((1, 1), ((1 << 256) + 5, big), ((1 << 384) - 1, 1), (1 << 384, 7), (7, (1 << 500) + 1), (-5, 9), (0, 3)):
        sig = o.der_encode_sig(r, s)
        ok, r48, s48, used = parse(lib, fn, 48, sig + b"rest")
        assert ok == 1 and used == len(sig)
        assert (r48, s48, used) == o.der_parse_sig48(sig + b"rest")
        w = lambda v: v if 0 < v < 1 << 384 else 0  # noqa: E731
        assert (int.from_bytes(r48, "big"), int.from_bytes(s48, "big")) == (w(r), w(s))
    assert parse(lib, fn, 48, b"")[0] == 0
    assert fn(None, 0, ctypes.c_void_p(np.zeros(48, np.uint8).ctypes.data),
              ctypes.c_void_p(np.zeros(48, np.uint8).ctypes.data), None) == 0


def pkix(lib, der, ctx=None):
    out = np.full(104, 0xEE, dtype=np.uint8)
    buf = (ctypes.c_uint8 * max(1, len(der))).from_buffer_copy(bytes(der) or b"\0")
    rc = lib.mbft_pkix_parse_p384(ctx, buf, len(der), ctypes.c_void_p(out.ctypes.data))
    assert (out[96:] == 0xEE).all()
    return rc, bytes(out[:96])


def test_pkix_parse_p384(lib):
    ERR_ARG, ERR_KEY = -1, -4
    q = o.pubkey(0xC0FFEE)
    der = o.pkix_encode(q)
    assert len(der) == 120
    rc, xy = pkix(lib, der)
    assert rc == 0 and xy == der[24:]
    for d in (1, o.N - 1, 2):
        q2 = o.pubkey(d)
        assert pkix(lib, o.pkix_encode(q2)) == (0, o.pkix_encode(q2)[24:])
    untouched = bytes([0xEE]) * 96
    # another length, another curve's SPKI, a compressed point, a prefix byte changed
    p256 = bytes.fromhex("3059301306072a8648ce3d020106082a8648ce3d030107034200") + b"\x04" + bytes(64)
    bad_form = [der[:-1], der + b"\0", b"", p256, der[:23] + b"\x02" + der[24:], der[:23] + b"\x03" + der[24:]]
    bad_form += [der[:i] + bytes([der[i] ^ 1]) + der[i + 1:] for i in range(24)]
    for b in bad_form:
        assert pkix(lib, b) == (ERR_KEY, untouched), b.hex()
    # the right form, no point of the curve
    x, y = q
    for bx, by in ((x, (y + 1) % o.P), (0, 0), (o.P, y), (x, o.P), ((1 << 384) - 1, y), (x, x)):
        b = der[:24] + bx.to_bytes(48, "big") + by.to_bytes(48, "big")
        assert not o.on_curve(bx, by)
        assert pkix(lib, b) == (ERR_KEY, untouched), (hex(bx), hex(by))
    out = np.zeros(96, dtype=np.uint8)
    assert lib.mbft_pkix_parse_p384(None, None, 120, ctypes.c_void_p(out.ctypes.data)) == ERR_ARG
    buf = (ctypes.c_uint8 * 120).from_buffer_copy(der)
    assert lib.mbft_pkix_parse_p384(None, buf, 120, None) == ERR_ARG
