"""The software USIG's host-compilable device code (minbft_amd/csrc/
sha256_dev.h sha256_usig_chain, sign_dev.h usig_ui_write) compiled for the
HOST into tests/libusig_check.so (tests/csrc/usig_check.cpp) and checked
against the oracle: the signed digest SHA256(SHA256(m) || epoch_le64 ||
counter_le64) and the UI bytes counter_be64 || epoch_be64 || DER.  Epoch and
counter have eight distinct bytes each, so that a little-/big-endian mix-up in
either place cannot pass.  The GPU run of the same code is compared with the
oracle in tests/test_gpu_usig_gen.py."""
import ctypes
import random

import numpy as np
import pytest

from oracle import p256 as o

EPOCH = 0x0102030405060708
FIRST = 0x1112131415161718
LENGTHS = [0, 55, 56, 63, 64, 119, 120]


@pytest.fixture(scope="module")
def lib():
    from __graft_entry__ import build_usig_check
    lib = ctypes.CDLL(build_usig_check())
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    lib.usig_check_digest.argtypes = [vp, vp, i, u64, u64, vp]
    lib.usig_check_ui.argtypes = [vp, vp, i, u64, u64, vp, vp]
    return lib


def _messages():
    rng = random.Random(0x0516)
    msgs = [rng.randbytes(n) for n in LENGTHS]
    prep = o.authen_prepare(rng.randrange(2 ** 64), rng.randrange(2 ** 32), rng.randrange(2 ** 64),
                            rng.randbytes(33))
    com = o.authen_commit(rng.randrange(2 ** 32), rng.randrange(2 ** 64), rng.randrange(2 ** 32),
                          rng.randrange(2 ** 64), rng.randbytes(7), rng.randrange(2 ** 64))
    assert (len(prep), len(com)) == (59, 70)
    return msgs + [prep, com]


def _digests(lib, msgs, epoch, first):
    n = len(msgs)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs])
    data = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
    e = np.zeros(32 * n, dtype=np.uint8)
    assert lib.usig_check_digest(data.ctypes.data, off.ctypes.data, n, epoch, first, e.ctypes.data) == 0
    return [bytes(e[32 * i:32 * i + 32]) for i in range(n)]


def test_slot_size(lib):
    from minbft_amd import _lib
    assert lib.usig_check_slot() == _lib.UI_SLOT == 88


def test_digest_chain(lib):
    msgs = _messages()
    got = _digests(lib, msgs, EPOCH, FIRST)
    assert got == [o.usig_digest(m, EPOCH, FIRST + i) for i, m in enumerate(msgs)]
    # the byte orders matter: the swapped reading is another digest
    swapped = int.from_bytes(EPOCH.to_bytes(8, "little"), "big")
    assert got[0] != o.usig_digest(msgs[0], swapped, FIRST)
    # counter 1 and the carry into the second byte
    for first in (1, 255, 256, 2 ** 32 - 1, 2 ** 64 - len(msgs)):
        assert _digests(lib, msgs, EPOCH, first) == [o.usig_digest(m, EPOCH, first + i)
                                                     for i, m in enumerate(msgs)]


def test_ui_assembly(lib):
    rng = random.Random(88)
    # r / s of every shape the DER encoder distinguishes: top bit set or not,
    # short values, the extremes
    vals = [1, 0x7F, 0x80, o.N - 1, 2 ** 255, 2 ** 255 - 1, 2 ** 247, 2 ** 248 - 1]
    rs = [(a, b) for a in vals for b in vals] + [(rng.randrange(1, o.N), rng.randrange(1, o.N))
                                                 for _ in range(64)]
    n = len(rs)
    r = np.frombuffer(b"".join(a.to_bytes(32, "big") for a, _ in rs), dtype=np.uint8).copy()
    s = np.frombuffer(b"".join(b.to_bytes(32, "big") for _, b in rs), dtype=np.uint8).copy()
    uis = np.full(88 * n, 0xAA, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint8)
    assert lib.usig_check_ui(r.ctypes.data, s.ctypes.data, n, EPOCH, FIRST, uis.ctypes.data,
                             lens.ctypes.data) == 0
    for i, (a, b) in enumerate(rs):
        slot, n_ui = bytes(uis[88 * i:88 * i + 88]), int(lens[i])
        want = o.ui_marshal(FIRST + i, o.make_cert(EPOCH, o.der_encode_sig(a, b)))
        assert slot[:n_ui] == want, i
        assert slot[n_ui:] == bytes(88 - n_ui)  # the rest of the slot is zeroed
        # and it parses back as the reference's verifier reads it
        assert int.from_bytes(slot[:8], "big") == FIRST + i
        assert int.from_bytes(slot[8:16], "big") == EPOCH
        assert o.der_parse_sig(slot[16:n_ui]) == (a, b, b"")


def test_whole_ui_against_oracle(lib):
    """Digest chain + oracle signature + UI assembly == oracle.usig_create_ui
    for every message (the kernel's data flow with the signer replaced)."""
    d = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF0 % o.N
    msgs = _messages()
    es = _digests(lib, msgs, EPOCH, FIRST)
    sigs = [o.ecdsa_sign(d, e) for e in es]
    n = len(msgs)
    r = np.frombuffer(b"".join(a.to_bytes(32, "big") for a, _ in sigs), dtype=np.uint8).copy()
    s = np.frombuffer(b"".join(b.to_bytes(32, "big") for _, b in sigs), dtype=np.uint8).copy()
    uis = np.full(88 * n, 0x55, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint8)
    assert lib.usig_check_ui(r.ctypes.data, s.ctypes.data, n, EPOCH, FIRST, uis.ctypes.data,
                             lens.ctypes.data) == 0
    for i, m in enumerate(msgs):
        assert bytes(uis[88 * i:88 * i + int(lens[i])]) == o.usig_create_ui(d, m, EPOCH, FIRST + i)
