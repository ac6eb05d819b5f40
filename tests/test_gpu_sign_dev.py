"""The batch signer's device-only paths (minbft_amd/csrc/sign_rs_dev.h,
sign_dev.h, der_enc_dev.h) on the GPU with INJECTED inputs, through the
test-only harness tests/csrc/sign_dev_check.hip, against big integers.

Through the kernels a nonce comes out of HMAC, so the end-to-end tests
(tests/test_gpu_sign.py, tests/test_gpu_usig_gen.py) cannot choose it.  Here
sign_comb is handed the scalars at which its selects change state, sign_r the
x in [N, p) that no real nonce reaches, sign_s and sign_loop the candidates
whose s is exactly 0, and the device builds of the nonce generator, the DER
encoder and the masked pick the inputs of tests/test_sign_host.py.  The comb
runs over a table made in Python (tests/comb_layout.py), so none of this
depends on the product's table build; tests/test_gpu_tables.py pins that."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

from comb_layout import entries, last_bits, steps, structured_scalars, table_bytes
from oracle import p256 as o
from test_gpu_field import (N, OPS, P, R, RINV, RNINV, SUB2X_OUT, golden_module, limbs, normalized, push_up,
                            rnd_value, run, value)
from test_gpu_sign import EDGE_E
from test_sign_host import _model_k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [4, 5, 6]
OPS.update({"fe_inv": 14, "fn_inv": 39})


@pytest.fixture(scope="module")
def dev(lib):
    path = os.path.join(ROOT, "tests", "libsign_dev_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_sign_dev_check
        build_sign_dev_check()
    h = ctypes.CDLL(path)
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    h.sign_dev_tries.argtypes = []
    h.sign_dev_table_entries.argtypes = [i]
    h.sign_dev_table_entries.restype = u64
    h.sign_dev_comb.argtypes = [vp, i, vp, u64, i, vp]
    h.sign_dev_r_of_point.argtypes = [vp, i, vp]
    h.sign_dev_rs_of_k.argtypes = [vp, i, vp, u64, i, vp]
    h.sign_dev_loop.argtypes = [vp, vp, vp, i, vp, u64, i, u64, u64, vp, vp, vp, vp, vp]
    h.sign_dev_nonce.argtypes = [vp, vp, vp, i, vp, vp]
    h.sign_dev_der.argtypes = [vp, vp, i, vp, vp]
    h.sign_dev_pick.argtypes = [vp, i, vp, i, vp]
    for W in WINDOWS:
        assert h.sign_dev_table_entries(W) == entries(W)
    return h


@pytest.fixture(scope="module")
def field(lib):
    path = os.path.join(ROOT, "tests", "libfield_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_test_harness
        build_test_harness()
    h = ctypes.CDLL(path)
    h.field_check_run.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]
    h.field_check_run.restype = ctypes.c_int
    return h


@pytest.fixture(scope="module")
def tables():
    """The generator's table for each signer window, made in Python."""
    return {W: np.frombuffer(table_bytes(o.G, W), dtype=np.uint32).copy() for W in WINDOWS}


_KG = {}


def kG(k):
    """o.scalar_mult(k, G), computed once per scalar and never changed."""
    if k not in _KG:
        _KG[k] = o.scalar_mult(k, o.G)
    return _KG[k]


def words8(v):
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def from_words8(w):
    return sum(int(x) << (32 * j) for j, x in enumerate(w))


def _b32(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=np.uint8).copy()


# ------------------------------------------------------------------ a. comb
def digit_states(k, W, mg):
    """The named states of sign_comb's select logic that the scalar k runs
    through, from the Python recoding."""
    dig = mg.signed_digits(k, W)
    S, L = steps(W), last_bits(W)
    assert len(dig) == S
    st = set()
    if not any(dig[:-1]) and dig[-1]:
        st.add("inf_until_last")
    nz = [j for j, d in enumerate(dig) if d]
    if any(d == 0 for d in dig[nz[0]:nz[-1]]):
        st.add("zero_after_nonzero")
    if any(d < 0 for d in dig):
        st.add("negative")
    if dig[-1] == 1 << L:
        st.add("top_2^L")
    if any(d == 1 << (W - 1) for d in dig[:-1]):
        st.add("tie")
    if len(nz) > 1 and nz[0] >= S // 2:
        st.add("inf_past_half")
    return st


STATES = {"inf_until_last", "zero_after_nonzero", "negative", "top_2^L", "tie"}


def comb_lanes(W, mg):
    """The lanes of the comb launch: wave 0 holds every single named case
    beside members of the 2^(W j) families and random scalars; then all cases
    once more, dealt round-robin over the waves so that neighbours of a
    family (windows j, j + 1 ...) sit in different waves and every wave holds
    a cross-section."""
    cases = structured_scalars(W, mg.scalar_edge_values(random.Random(0x45444745)))
    single = [c for c in cases if not c[0].startswith(("pow", "rnd"))]
    family = [c for c in cases if c[0].startswith("pow")]
    rnd = [c for c in cases if c[0].startswith("rnd")]
    assert len(rnd) == 200 and len(single) < 40
    wave0 = single + family[1::7]
    wave0 += rnd[:64 - len(wave0)]
    assert len(wave0) == 64
    random.Random(W).shuffle(wave0)
    nw = -(-len(cases) // 64)
    dealt = [None] * (nw * 64)
    for i, c in enumerate(cases):
        dealt[(i % nw) * 64 + i // nw] = c
    return cases, wave0 + [c for c in dealt if c is not None]


@pytest.mark.parametrize("W", WINDOWS)
def test_comb_structured_scalars(dev, tables, W):
    """sign_comb over the scalars that drive its selects through every state
    (comb_layout.structured_scalars): the affine point equals k G, Z != 0, and
    X, Y, Z are normalized and inside ec_madd's documented output bounds
    (X < 2^257 + 2^234, Y and Z < 2^258) -- the chain feeds ec_madd its own
    outputs up to 64 times.  A wrong select shows as a wrong point for one
    nonce in 2^(2W) or rarer, which byte parity over random items never meets."""
    mg = golden_module()
    cases, lanes = comb_lanes(W, mg)
    S, L = steps(W), last_bits(W)
    # the case list really contains every named state, and wave 0 mixes them
    seen = set().union(*(digit_states(k, W, mg) for _, k in cases))
    assert seen >= STATES | {"inf_past_half"}, seen
    assert set().union(*(digit_states(k, W, mg) for _, k in lanes[:64])) >= STATES
    by = dict(cases)
    assert mg.signed_digits(by["top_only"], W) == [0] * (S - 1) + [1]
    assert mg.signed_digits(by["top_largest"], W) == [0] * (S - 1) + [o.N >> (W * (S - 1))]
    assert mg.signed_digits(by["N-1"], W)[-1] == 1 << L
    assert mg.signed_digits(by["carry_through"], W)[0] == -1 and mg.signed_digits(by["carry_through"], W)[-1] > 0
    assert mg.signed_digits(by[f"pow{S - 2}-1"], W) == [-1] + [0] * (S - 3) + [1, 0]  # a carry chain
    assert mg.signed_digits(by[f"pow{S - 2}+1"], W) == [1] + [0] * (S - 3) + [1, 0]   # a zero run
    for j in (0, S // 2, S - 2):
        assert mg.signed_digits(by[f"tie@{j}"], W)[j] == 1 << (W - 1)
        assert mg.signed_digits(by[f"tie+1@{j}"], W)[j] == 1 - (1 << (W - 1))
    n = len(lanes)
    kin = np.array([words8(k) for _, k in lanes], dtype=np.uint32)
    out = np.zeros((n, 27), dtype=np.uint32)
    tab = tables[W]
    assert dev.sign_dev_comb(kin.ctypes.data, n, tab.ctypes.data, tab.size, W, out.ctypes.data) == 0
    bad = []
    for (name, k), row in zip(lanes, out):
        X, Y, Z = row[0:9], row[9:18], row[18:27]
        Xv, Yv, Zv = value(X) * RINV % P, value(Y) * RINV % P, value(Z) * RINV % P
        if Zv == 0:
            bad.append((name, "Z == 0"))
            continue
        zi = pow(Zv, -1, P)
        ok = (Xv * zi * zi % P, Yv * zi * zi * zi % P) == kG(k) and value(X) < SUB2X_OUT and \
            value(Y) < (1 << 258) and value(Z) < (1 << 258) and all(normalized(t) for t in (X, Y, Z))
        if not ok:
            bad.append((name, hex(k)))
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------ b. r_of_point
def test_r_of_point(dev):
    """sign_r on pure field inputs X = x z^2 R, Z = z R pushed up to
    ec_madd's output bounds, for x that no real nonce reaches: exactly x mod N
    as canonical words -- 0 for x in {0, N}, x - N for x in (N, p)."""
    rng = random.Random(0x50F9)
    xs = [0, 1, N - 1, N, N + 1, P - N - 1, P - 2, P - 1]
    xs += [rng.randrange(N, P) for _ in range(100)] + [rng.randrange(N) for _ in range(100)]
    inp = []
    for i, x in enumerate(xs):
        z = rng.randrange(1, P)
        X = push_up(x * z * z * R % P, P, SUB2X_OUT, rng, pick=i % 3)
        Z = push_up(z * R % P, P, 1 << 258, rng, pick=(i // 3) % 3)
        inp.append(limbs(X) + limbs(Z))
    inp = np.array(inp, dtype=np.uint32)
    out = np.zeros((len(xs), 8), dtype=np.uint32)
    assert dev.sign_dev_r_of_point(inp.ctypes.data, len(xs), out.ctypes.data) == 0
    got = [from_words8(w) for w in out]
    bad = [(hex(x), hex(g)) for x, g in zip(xs, got) if g != x % N]
    assert not bad, (len(bad), bad[:5])
    assert got[0] == 0 and got[3] == 0 and got[7] == P - 1 - N


# ------------------------------------------------------------ c. inversions
def test_fermat_inversions(field):
    """fe_inv and fn_inv (fixed-exponent Fermat, device only; Montgomery in
    and out) on the Montgomery forms of 1, 2 and -1, adversarial limb patterns
    and representatives pushed up to 2^258: congruent to the Montgomery form of
    the inverse, below the fe_mul / fn_mul output bound 2^258, normalized; and
    0 gives 0."""
    rng = random.Random(0x1F17)
    cases = []
    for op, mod in (("fe_inv", P), ("fn_inv", N)):
        vals = [v * R % mod for v in (1, 2, mod - 1)]
        vals += [rnd_value(rng, 1 << 258) for _ in range(300)]
        vals += [push_up(rng.randrange(1, mod), mod, 1 << 258, rng, pick=0) for _ in range(100)]
        vals += [push_up(rnd_value(rng, mod) or 1, mod, 1 << 258, rng) for _ in range(100)]
        vals += [0, mod - 1, (1 << 258) - 1]
        cases += [(op, [v]) for v in vals]
    res = run(field, cases)
    bad = []
    for (op, (a,)), (o0, _, _, _) in zip(cases, res):
        mod, rinv = (P, RINV) if op == "fe_inv" else (N, RNINV)
        v = value(o0)
        if a % mod == 0:
            ok = v == 0 if a == 0 else v % mod == 0
        else:
            ok = v % mod == pow(a * rinv % mod, -1, mod) * R % mod
        if not (ok and v < (1 << 258) and normalized(o0)):
            bad.append((op, hex(a), hex(v)))
    assert not bad, (len(bad), bad[:5])


# -------------------------------------------------------------- d. rs_of_k
def ref_rs(k, d, e):
    r = kG(k)[0] % N
    return r, pow(k, -1, N) * (e + r * d) % N


def e_for_s(k, d, s):
    """The e below N for which the candidate k gives exactly s under d."""
    r = kG(k)[0] % N
    return (s * k - r * d) % N


def test_rs_of_k(dev, tables):
    """sign_comb + sign_r + sign_s with k, d and e chosen independently
    (1, 2, N - 1, N - 2 and random; e also 0, N - 1, N, N + 1, 2^256 - 1)
    against r = x(k G) mod N, s = k^-1 (e + r d) mod N, and with e crafted so
    that s is exactly 0 (e = -r d mod N, and that plus N where it stays below
    2^256), 1 and N - 1."""
    rng = random.Random(0xD5)
    small = [1, 2, N - 1, N - 2]
    cases = []
    for i in range(64):
        k = small[i % 4] if i % 3 == 0 else rng.randrange(1, N)
        d = small[(i // 4) % 4] if i % 5 < 2 else rng.randrange(1, N)
        e = EDGE_E[i % len(EDGE_E)] if i % 2 == 0 else rng.randrange(1 << 256)
        cases.append((k, d, e, None))
    assert {c[0] for c in cases} >= set(small) and {c[1] for c in cases} >= set(small)
    assert {c[2] for c in cases} >= set(EDGE_E)
    plus_n = 0
    for i in range(24):
        k = small[i % 4] if i % 6 == 0 else rng.randrange(1, N)
        d = small[(i // 4) % 4] if i % 5 == 0 else rng.randrange(1, N)
        for s in (0, 0, 1, N - 1):
            e = e_for_s(k, d, s)
            cases.append((k, d, e, s))
            if e + N < (1 << 256):
                cases.append((k, d, e + N, s))
                plus_n += s == 0
    # some -r d mod N fall below 2^256 - N (about 2^-32 of all: crafted)
    for i in range(4):
        k, d = rng.randrange(1, N), rng.randrange(1, N)
        r = kG(k)[0] % N
        e = rng.randrange((1 << 256) - N)
        d = (-e) * pow(r, -1, N) % N   # so that -r d == e (mod N)
        assert d and e_for_s(k, d, 0) == e
        cases += [(k, d, e, 0), (k, d, e + N, 0)]
        plus_n += 1
    assert plus_n >= 4
    for W in WINDOWS:
        inp = np.array([words8(k) + words8(d) + words8(e) for k, d, e, _ in cases], dtype=np.uint32)
        out = np.zeros((len(cases), 16), dtype=np.uint32)
        tab = tables[W]
        assert dev.sign_dev_rs_of_k(inp.ctypes.data, len(cases), tab.ctypes.data, tab.size, W,
                                    out.ctypes.data) == 0
        bad = []
        for (k, d, e, s_want), row in zip(cases, out):
            want = ref_rs(k, d, e)
            assert s_want is None or want[1] == s_want
            got = (from_words8(row[:8]), from_words8(row[8:]))
            if got != want:
                bad.append((W, hex(k), hex(d), hex(e), [hex(x) for x in got]))
        assert not bad, (len(bad), bad[:5])


# ----------------------------------------------------------------- e. loop
EPOCH = 0x0102030405060708
FIRST = 0xFFFFFFFE  # the counters of one launch cross 2^32


def test_candidate_loop(dev, tables):
    """sign_loop over crafted candidate lists served by a list-backed nonce
    source, and the two tails the kernels run after it.  A bad candidate is
    one whose s is exactly 0 under the lane's (d, e); k and N - k share r, so
    a lane's bad candidates alternate between the two.  Lanes of one wave
    leave the loop on different iterations: a good first candidate (1 drawn,
    0 discarded), [bad, good] (2, 1), [bad, bad, good] (3, 2), [bad, bad, bad,
    good] (4, 3), kSignTries bad ones and a good fifth that must never be
    drawn (false, r = s = 0, both slots zero, both lengths 0), and a list that
    ends after one bad candidate (false)."""
    tries = dev.sign_dev_tries()
    assert tries == 4
    rng = random.Random(0x100B)
    shapes = [(0, True), (1, True), (2, True), (3, True), (tries, True), (1, False)]
    lanes = []
    for i in range(128):
        nbad, has_good = shapes[(i + i // 64) % len(shapes)]
        kb, d = rng.randrange(1, N), rng.randrange(1, N)
        e = e_for_s(kb, d, 0)
        if e + N < (1 << 256) or (i % 16 == 5):
            # an e at or above N (the second case by choosing d for a small e)
            if e + N >= (1 << 256):
                e = rng.randrange((1 << 256) - N)
                d = (-e) * pow(kG(kb)[0] % N, -1, N) % N
            e += N
        good = rng.randrange(1, N)
        assert ref_rs(kb, d, e)[1] == 0 and ref_rs(N - kb, d, e)[1] == 0 and all(ref_rs(good, d, e))
        lst = [kb if j % 2 == 0 else N - kb for j in range(nbad)] + ([good] if has_good else [])
        lanes.append((lst, d, e, good, nbad, has_good))
    assert all({(l[4], l[5]) for l in lanes[w * 64:w * 64 + 64]} == set(shapes) for w in range(2))
    assert any(l[2] >= N for l in lanes)
    n = len(lanes)
    cand = np.zeros((n, tries + 1, 8), dtype=np.uint32)
    count = np.zeros(n, dtype=np.uint32)
    de = np.zeros((n, 16), dtype=np.uint32)
    for i, (lst, d, e, _, _, _) in enumerate(lanes):
        assert len(lst) <= tries + 1
        for j, k in enumerate(lst):
            cand[i, j] = words8(k)
        count[i] = len(lst)
        de[i] = words8(d) + words8(e)
    for W in WINDOWS:
        res = np.zeros((n, 20), dtype=np.uint32)
        tags = np.zeros((n, 72), dtype=np.uint8)
        uis = np.zeros((n, 88), dtype=np.uint8)
        tl = np.zeros(n, dtype=np.uint8)
        ul = np.zeros(n, dtype=np.uint8)
        tab = tables[W]
        assert dev.sign_dev_loop(cand.ctypes.data, count.ctypes.data, de.ctypes.data, n, tab.ctypes.data,
                                 tab.size, W, FIRST, EPOCH, res.ctypes.data, tags.ctypes.data,
                                 tl.ctypes.data, uis.ctypes.data, ul.ctypes.data) == 0
        for i, (lst, d, e, good, nbad, has_good) in enumerate(lanes):
            ret, drawn, discards = (int(x) for x in res[i, :3])
            r, s = from_words8(res[i, 4:12]), from_words8(res[i, 12:20])
            tag, ui = bytes(tags[i]), bytes(uis[i])
            ctx = (W, i, nbad, has_good)
            if has_good and nbad < tries:
                want = ref_rs(good, d, e)
                der = o.der_encode_sig(*want)
                head = (FIRST + i).to_bytes(8, "big") + EPOCH.to_bytes(8, "big")
                assert (ret, drawn, discards) == (1, nbad + 1, nbad), ctx
                assert (r, s) == want, ctx
                assert tag == der + bytes(72 - len(der)) and int(tl[i]) == len(der), ctx
                assert ui == head + der + bytes(72 - len(der)) and int(ul[i]) == 16 + len(der), ctx
            else:
                # exhausted: kSignTries drawn (the good fifth never), or the list ran out
                assert (ret, drawn, discards) == (0, nbad, nbad), ctx
                assert (r, s) == (0, 0), ctx
                assert tag == bytes(72) and ui == bytes(88) and int(tl[i]) == 0 and int(ul[i]) == 0, ctx


# ---------------------------------------------------------------- f. nonce
def _nonces(dev, ds, es, q):
    n = len(ds)
    d, e, qb = _b32(ds), np.frombuffer(b"".join(es), dtype=np.uint8).copy(), _b32([q])
    k = np.zeros(32 * n, dtype=np.uint8)
    tries = np.zeros(n, dtype=np.int32)
    assert dev.sign_dev_nonce(d.ctypes.data, e.ctypes.data, qb.ctypes.data, n, k.ctypes.data,
                              tries.ctypes.data) == 0
    return [int.from_bytes(bytes(k[32 * i:32 * i + 32]), "big") for i in range(n)], tries.tolist()


def test_nonce_rfc6979_vectors(dev):
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))["rfc6979_p256_sha256"]
    d = int(kat["d"], 16)
    hs = [hashlib.sha256(v["msg"].encode()).digest() for v in kat["vectors"]]
    ks, tries = _nonces(dev, [d] * len(hs), hs, o.N)
    assert ks == [int(v["k"], 16) for v in kat["vectors"]]
    assert tries == [1] * len(hs)


def test_nonce_random_against_oracle(dev):
    rng = random.Random(6979)
    ds = [rng.randrange(1, o.N) for _ in range(256)]
    # e below, at and above N: bits2octets' conditional subtraction
    es = [rng.randbytes(32) for _ in range(250)] + [
        (0).to_bytes(32, "big"), (o.N - 1).to_bytes(32, "big"), o.N.to_bytes(32, "big"),
        (o.N + 1).to_bytes(32, "big"), (2 ** 256 - 1).to_bytes(32, "big"), b"\xff" * 16 + b"\x00" * 16]
    ks, _ = _nonces(dev, ds, es, o.N)
    assert ks == [o.rfc6979_k(d, e) for d, e in zip(ds, es)]


def test_nonce_retry_branch(dev):
    """q = 2^255 + 1 rejects about half of the candidates, so Rfc6979::retry()
    and the candidate cap run on the device, lanes of one wave drawing
    different numbers of candidates; q = 1 rejects every candidate."""
    q = 2 ** 255 + 1
    rng = random.Random(255)
    ds = [rng.randrange(1, q) for _ in range(512)]
    es = [rng.randbytes(32) for _ in range(512)]
    want = [_model_k(d, e, q) for d, e in zip(ds, es)]
    assert sum(1 for _, t in want if t == 0 or t >= 2) >= 100
    assert sum(1 for _, t in want if t == 0 or t >= 3) >= 20
    assert sum(1 for _, t in want if t == 0) >= 10
    ks, tries = _nonces(dev, ds, es, q)
    assert ks == [k for k, _ in want]
    assert tries == [t for _, t in want]
    ks, tries = _nonces(dev, ds[:128], es[:128], 1)
    assert ks == [0] * 128 and tries == [0] * 128


# --------------------------------------------------------- g. der and pick
def _der(dev, rs, ss):
    n = len(rs)
    r, s = _b32(rs), _b32(ss)
    tags = np.zeros(72 * n, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint8)
    assert dev.sign_dev_der(r.ctypes.data, s.ctypes.data, n, tags.ctypes.data, lens.ctypes.data) == 0
    out = []
    for i in range(n):
        slot = bytes(tags[72 * i:72 * i + 72])
        assert slot[lens[i]:] == bytes(72 - lens[i])  # the rest of the slot (0xAA before) is zeroed
        out.append(slot[:lens[i]])
    return out


def test_der_every_length_pair(dev):
    """der_encode_sig on the device over all 4096 (length, top bit)
    combinations of r and s -- down to one byte each -- the 1 / N - 1 pairs
    and the sign_edges.json pairs, one launch."""
    rng = random.Random(690)

    def val(nbytes, top):
        lead = rng.randrange(0x80, 0x100) if top else rng.randrange(1, 0x80)
        return int.from_bytes(bytes([lead]) + rng.randbytes(nbytes - 1), "big")

    rs, ss = [], []
    for lr in range(1, 33):
        for ls in range(1, 33):
            for tr in (False, True):
                for ts in (False, True):
                    rs.append(val(lr, tr))
                    ss.append(val(ls, ts))
    assert len(rs) == 4096
    for a in (1, o.N - 1):
        for b in (1, o.N - 1):
            rs.append(a)
            ss.append(b)
    edges = json.load(open(os.path.join(ROOT, "tests", "golden", "sign_edges.json")))
    assert sorted(x["case"] for x in edges) == ["r31_nopad", "r31_pad", "s31_nopad", "s31_pad"]
    rs += [int(x["r"], 16) for x in edges]
    ss += [int(x["s"], 16) for x in edges]
    got = _der(dev, rs, ss)
    for r, s, tag in zip(rs, ss, got):
        assert tag == o.der_encode_sig(r, s), (hex(r), hex(s))
    assert [t.hex() for t in got[-4:]] == [x["tag"] for x in edges]


def test_masked_pick(dev):
    """sign_pick in the build where its "+v" asm and mask select run: every
    |digit| 0 .. count picks its own entry (0 picks entry 1, the dummy
    operand), the digits interleaved across the lanes of each wave."""
    for count in (2, 8, 16, 32):
        win = (np.arange(16 * count, dtype=np.uint64) * 2654435761 % (2 ** 32)).astype(np.uint32)
        mags = np.array([(7 * i) % (count + 1) for i in range(4 * 64)], dtype=np.uint32)
        assert set(mags[:64].tolist()) == set(range(count + 1)) and len(set(mags[:count + 1].tolist())) == count + 1
        out = np.zeros((len(mags), 16), dtype=np.uint32)
        assert dev.sign_dev_pick(win.ctypes.data, count, mags.ctypes.data, len(mags), out.ctypes.data) == 0
        ent = win.reshape(count, 16)
        for m, row in zip(mags.tolist(), out):
            assert (row == ent[max(m, 1) - 1]).all(), (count, m)
