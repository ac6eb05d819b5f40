"""The batch signer's host-compilable device code (minbft_amd/csrc/sign_dev.h,
der_enc_dev.h) compiled for the HOST into tests/libsign_check.so
(tests/csrc/sign_check.cpp) and checked against the oracle: the RFC 6979
nonce (with the product's q = N and with a q that makes the retry branch
common), the DER encoder over every length pair, and the window recoding with
the property the kernel's no-degenerate-addition argument rests on
(sign_kernels.hip).  The GPU run of the same code is compared with the oracle
in tests/test_gpu_sign.py."""
import ctypes
import hashlib
import hmac
import json
import os
import random

import numpy as np
import pytest

from oracle import p256 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIES = 4  # kSignTries


@pytest.fixture(scope="module")
def lib():
    from __graft_entry__ import build_sign_check
    lib = ctypes.CDLL(build_sign_check())
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.sign_check_nonce.argtypes = [vp, vp, vp, i, vp, vp]
    lib.sign_check_der.argtypes = [vp, vp, i, vp, vp]
    lib.sign_check_recode.argtypes = [vp, i, i, vp]
    lib.sign_check_pick.argtypes = [vp, i, vp, i, vp]
    lib.sign_check_window_entries.argtypes = [i, i]
    return lib


def _b32(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=np.uint8).copy()


def _nonces(lib, ds, es, q):
    n = len(ds)
    d, e, qb = _b32(ds), np.frombuffer(b"".join(es), dtype=np.uint8).copy(), _b32([q])
    k = np.zeros(32 * n, dtype=np.uint8)
    tries = np.zeros(n, dtype=np.int32)
    assert lib.sign_check_nonce(d.ctypes.data, e.ctypes.data, qb.ctypes.data, n, k.ctypes.data,
                                tries.ctypes.data) == 0
    return [int.from_bytes(bytes(k[32 * i:32 * i + 32]), "big") for i in range(n)], tries.tolist()


def _model_k(d, h1, q):
    """oracle.rfc6979_k generalised to a group order q (2^255 <= q < 2^256) and
    capped at TRIES candidates: (k, candidates drawn), or (0, 0)."""
    mac = lambda k, m: hmac.new(k, m, hashlib.sha256).digest()  # noqa: E731
    x = d.to_bytes(32, "big")
    hv = (int.from_bytes(h1, "big") % q).to_bytes(32, "big")
    v, k = b"\x01" * 32, b"\x00" * 32
    k = mac(k, v + b"\x00" + x + hv)
    v = mac(k, v)
    k = mac(k, v + b"\x01" + x + hv)
    v = mac(k, v)
    for t in range(1, TRIES + 1):
        v = mac(k, v)
        kk = int.from_bytes(v, "big")
        if 1 <= kk < q:
            return kk, t
        k = mac(k, v + b"\x00")
        v = mac(k, v)
    return 0, 0


def test_nonce_rfc6979_vectors(lib):
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))["rfc6979_p256_sha256"]
    d = int(kat["d"], 16)
    hs = [hashlib.sha256(v["msg"].encode()).digest() for v in kat["vectors"]]
    ks, tries = _nonces(lib, [d] * len(hs), hs, o.N)
    assert ks == [int(v["k"], 16) for v in kat["vectors"]]
    assert tries == [1] * len(hs)


def test_nonce_random_against_oracle(lib):
    rng = random.Random(6979)
    ds = [rng.randrange(1, o.N) for _ in range(256)]
    # e below, at and above N: bits2octets' conditional subtraction
    es = [rng.randbytes(32) for _ in range(250)] + [
        (0).to_bytes(32, "big"), (o.N - 1).to_bytes(32, "big"), o.N.to_bytes(32, "big"),
        (o.N + 1).to_bytes(32, "big"), (2 ** 256 - 1).to_bytes(32, "big"), b"\xff" * 16 + b"\x00" * 16]
    ks, _ = _nonces(lib, ds, es, o.N)
    assert ks == [o.rfc6979_k(d, e) for d, e in zip(ds, es)]


def test_nonce_retry_branch(lib):
    """q = 2^255 + 1 rejects about half of the candidates, so the retry step
    (K = HMAC_K(V || 00), V = HMAC_K(V)) and the candidate cap are exercised."""
    q = 2 ** 255 + 1
    rng = random.Random(255)
    ds = [rng.randrange(1, q) for _ in range(512)]
    es = [rng.randbytes(32) for _ in range(512)]
    want = [_model_k(d, e, q) for d, e in zip(ds, es)]
    assert sum(1 for _, t in want if t == 0 or t >= 2) >= 100
    assert sum(1 for _, t in want if t == 0 or t >= 3) >= 20
    ks, tries = _nonces(lib, ds, es, q)
    assert ks == [k for k, _ in want]
    assert tries == [t for _, t in want]


def _der(lib, rs, ss):
    n = len(rs)
    r, s = _b32(rs), _b32(ss)
    tags = np.full(72 * n, 0xAA, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint8)
    assert lib.sign_check_der(r.ctypes.data, s.ctypes.data, n, tags.ctypes.data, lens.ctypes.data) == 0
    out = []
    for i in range(n):
        slot = bytes(tags[72 * i:72 * i + 72])
        assert slot[lens[i]:] == bytes(72 - lens[i])  # the rest of the slot is zeroed
        out.append(slot[:lens[i]])
    return out


def test_der_every_length_pair(lib):
    rng = random.Random(690)

    def value(nbytes, top):
        lead = rng.randrange(0x80, 0x100) if top else rng.randrange(1, 0x80)
        return int.from_bytes(bytes([lead]) + rng.randbytes(nbytes - 1), "big")

    rs, ss = [], []
    for lr in range(1, 33):
        for ls in range(1, 33):
            for tr in (False, True):
                for ts in (False, True):
                    rs.append(value(lr, tr))
                    ss.append(value(ls, ts))
    for a in (1, o.N - 1):
        for b in (1, o.N - 1):
            rs.append(a)
            ss.append(b)
    got = _der(lib, rs, ss)
    for r, s, tag in zip(rs, ss, got):
        assert tag == o.der_encode_sig(r, s), (hex(r), hex(s))
        assert o.der_parse_sig(tag) == (r, s, b"")


def test_der_fixture_pairs(lib):
    edges = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_edges.json")))
    assert sorted(x["case"] for x in edges) == ["r31_nopad", "r31_pad", "s31_nopad", "s31_pad"]
    got = _der(lib, [int(x["r"], 16) for x in edges], [int(x["s"], 16) for x in edges])
    assert [t.hex() for t in got] == [x["tag"] for x in edges]


def _digits(lib, ks, W):
    n = len(ks)
    k = _b32(ks)
    dg = np.zeros((n, 64), dtype=np.int32)
    assert lib.sign_check_recode(k.ctypes.data, n, W, dg.ctypes.data) == 0
    return dg


@pytest.mark.parametrize("W", [4, 5, 6])
def test_recoding(lib, W):
    rng = random.Random(W)
    ks = [1, 2, o.N - 1, o.N - 2, 2 ** 255, (2 ** 256 - 1) % o.N] + [rng.randrange(1, o.N) for _ in range(10000)]
    S = (256 + W - 1) // W
    dg = _digits(lib, ks, W)
    assert not dg[:, S:].any()
    for k, row in zip(ks, dg.tolist()):
        m = 0  # the accumulator holds m G before window j
        for j in range(S):
            d = row[j]
            top = j == S - 1
            if top:
                assert 0 <= d <= lib.sign_check_window_entries(W, j) == 1 << (256 - (S - 1) * W)
            else:
                assert -(1 << (W - 1)) < d <= 1 << (W - 1) == lib.sign_check_window_entries(W, j)
            c = d << (W * j)
            if d != 0 and m != 0:
                # a kept addition m G + c G is never a doubling or a cancellation
                assert abs(m) < (1 << (W * j)) <= abs(c)
                assert (m - c) % o.N != 0 and (m + c) % o.N != 0
            assert (m == 0) == all(x == 0 for x in row[:j])  # "still at infinity" <=> digits so far zero
            m += c
        assert m == k


def test_masked_pick(lib):
    """Every |digit| picks its own entry; 0 picks entry 1 (the dummy operand)."""
    for count in (2, 8, 16, 32):
        win = (np.arange(16 * count, dtype=np.uint64) * 2654435761 % (2 ** 32)).astype(np.uint32)
        mags = np.arange(0, count + 1, dtype=np.uint32)
        out = np.zeros((count + 1, 16), dtype=np.uint32)
        assert lib.sign_check_pick(win.ctypes.data, count, mags.ctypes.data, count + 1, out.ctypes.data) == 0
        ent = win.reshape(count, 16)
        assert (out[0] == ent[0]).all()
        for m in range(1, count + 1):
            assert (out[m] == ent[m - 1]).all()
