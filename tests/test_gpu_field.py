"""Field / group primitives of the verifier (minbft_amd/csrc/fe29.h, ecc.h)
on the GPU vs Python big integers, through the test-only harness
tests/csrc/field_check.hip: every result is checked for its value mod p AND
for the representation bounds the kernels rely on (normalized 29-bit limbs,
value below the documented bound).  The inputs include adversarial limb
patterns -- top limbs 2^24 - 1 / 2^25 - 1 over arbitrary low limbs -- which
is where the unnormalized fold of fe_sub / fe_neg once went negative (a
madd in the comb-table build produced 3 wrong entries of one key's table;
found by tests/test_gpu_configs.py::test_c4_adversarial_gpu_share).

Also a library-level regression: that key's table entries (window 0, digits
30855, 61710, 61711 at W = 16) are hit by crafted valid signatures.

The second half covers what runs only on the device and was checked only
through accept / reject statuses: the mod-N arithmetic and u1 / u2
(scalars), the comb's signed recoding, the whole-wave inversion mod N
(scalar_dev.h), the joins of two Chudnovsky points and their wave-uniform
forms (ecc.h), and the accept test x_matches_r -- each at the documented
input bounds, with non-canonical representatives."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
R = 1 << 261
RINV = pow(R, -1, P)
MASK = (1 << 29) - 1
OPS = {"mul": 0, "sqr": 1, "sub": 2, "neg": 3, "add": 4, "mul2": 5, "canon": 6, "mulsmall8": 7,
       "madd": 8, "dbl": 9, "sub2x": 10, "muladd_p5b": 11, "muladd_p2b": 12, "sub5": 13,
       "chud_p": 16, "chud_n": 17, "aff_chud_p": 18, "aff_chud_n": 19,
       "chud_lazy_p": 20, "chud_lazy_n": 21, "chud_last_p": 22, "chud_last_n": 23, "norm_lazy": 24}
# the borrowed-limb constants of fe29.h (5p and 2p with every low limb in
# [2^29 - 1, 2^30)), as limb lists
P5B = [0x3ffffffb, 0x3ffffffe, 0x3ffffffe, 0x200009fe, 0x1fffffff, 0x1fffffff, 0x2013ffff,
       0x3f5fffff, 0x04fffffe]
P2B = [0x3ffffffe, 0x3ffffffe, 0x3ffffffe, 0x200003fe, 0x1fffffff, 0x1fffffff, 0x2007ffff,
       0x3fbfffff, 0x01fffffe]


def limbs(v):
    out = [(v >> (29 * i)) & MASK for i in range(8)]
    out.append(v >> 232)
    assert out[8] < (1 << 32)
    return out


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def normalized(l):
    return all(int(x) <= MASK for x in l[:8])


@pytest.fixture(scope="module")
def harness(lib):
    path = os.path.join(ROOT, "tests", "libfield_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_test_harness
        build_test_harness()
    h = ctypes.CDLL(path)
    h.field_check_run.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]
    h.field_check_run.restype = ctypes.c_int
    return h


def run(h, cases):
    """cases: list of (op, [up to 6 values]) -> list of 4 limb lists each."""
    n = len(cases)
    op = np.array([OPS[c[0]] for c in cases], dtype=np.uint32)
    inp = np.zeros((n, 54), dtype=np.uint32)
    for i, (_, vals) in enumerate(cases):
        for k, v in enumerate(vals):
            inp[i, 9 * k: 9 * k + 9] = v if isinstance(v, list) else limbs(v)  # a list: raw limbs
    out = np.zeros((n, 36), dtype=np.uint32)
    rc = h.field_check_run(op.ctypes.data, inp.ctypes.data, out.ctypes.data, n)
    assert rc == 0
    return [(out[i, 0:9], out[i, 9:18], out[i, 18:27], out[i, 27:36]) for i in range(n)]


def rnd_value(rng: random.Random, bound: int) -> int:
    """Mostly uniform below `bound`, plus adversarial top-limb patterns."""
    kind = rng.randrange(8)
    if kind == 0:
        return bound - 1 - rng.randrange(1 << 40)
    if kind == 1:
        v = (((1 << 24) - 1) << 232) | rng.randrange(1 << 232)
    elif kind == 2:
        v = (((1 << 25) - 1) << 232) | rng.randrange(1 << 232)
    elif kind == 3:
        v = (rng.randrange(1 << 26) << 232) | (MASK * sum(1 << (29 * i) for i in range(8)))
    elif kind == 4:
        v = rng.randrange(1 << 30)
    else:
        return rng.randrange(bound)
    return v % bound


SUB_OUT = (1 << 257) + (1 << 233)
SUB2X_OUT = (1 << 257) + (1 << 234)


def test_field_ops(harness):
    rng = random.Random(0xF1E1D)
    cases = []
    for _ in range(4000):
        cases.append(("mul", [rnd_value(rng, 1 << 258), rnd_value(rng, 1 << 258)]))
        cases.append(("sqr", [rnd_value(rng, 1 << 258)]))
        cases.append(("sub", [rnd_value(rng, 1 << 260), rnd_value(rng, 1 << 258)]))
        cases.append(("neg", [rnd_value(rng, 1 << 258)]))
        cases.append(("add", [rnd_value(rng, 1 << 258), rnd_value(rng, 1 << 258)]))
        cases.append(("mul2", [rnd_value(rng, 1 << 258) for _ in range(4)]))
        cases.append(("canon", [rnd_value(rng, 1 << 261)]))
        cases.append(("mulsmall8", [rnd_value(rng, 1 << 258)]))
        cases.append(("sub2x", [rnd_value(rng, 1 << 258) for _ in range(3)]))
        cases.append(("sub5", [rnd_value(rng, 1 << 258), rnd_value(rng, 1 << 258)]))
    # the exact failing input of the table build: 16p - y with top limb 2^24-1
    cases.append(("neg", [value([368789281, 165341017, 273952230, 529450281, 285790751,
                                 332211330, 153921400, 536458868, 16777215])]))
    res = run(harness, cases)
    bad = []
    for (op, vals), (o0, _, _, _) in zip(cases, res):
        v = value(o0)
        a = vals[0]
        b = vals[1] if len(vals) > 1 else 0
        if op == "mul":
            ok = v % P == a * b * RINV % P and v < (1 << 258)
        elif op == "sqr":
            ok = v % P == a * a * RINV % P and v < (1 << 258)
        elif op == "sub":
            ok = v % P == (a - b) % P and v < SUB_OUT
        elif op == "neg":
            ok = v % P == (-a) % P and v < SUB_OUT
        elif op == "add":
            ok = v == a + b
        elif op == "mul2":
            ok = v % P == (a * b + vals[2] * vals[3]) * RINV % P and v < (1 << 258)
        elif op == "sub5":
            ok = v % P == (a - b) % P and v < 5 * P + (1 << 258)
        elif op == "sub2x":
            ok = v % P == (a - b - 2 * vals[2]) % P and v < (1 << 257) + (1 << 234)
        elif op == "canon":
            ok = v == a % P
        else:
            ok = v % P == 8 * a % P and v < (1 << 257)
        if not (ok and normalized(o0)):
            bad.append((op, [hex(x) for x in vals], hex(v)))
    assert not bad, bad[:5]


def test_group_ops(harness):
    from oracle import p256 as o
    rng = random.Random(0x6A0)
    pts = [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(48)]
    cases, want = [], []
    pushed = [0, 0]   # dbl, madd cases at the bounds
    for i in range(3000):
        p1, p2 = pts[rng.randrange(48)], pts[rng.randrange(48)]
        if p1[0] == p2[0]:
            continue
        z = rng.randrange(1, P)
        X, Y, Z = p1[0] * z * z % P, p1[1] * z * z * z % P, z
        # Montgomery form, sometimes a non-canonical representative < 2^257,
        # and every third case representatives up to ec_madd's own output
        # bounds (X < 2^257 + 2^234, Y and Z < 2^258): the signer's comb feeds
        # ec_madd its outputs up to 64 times
        m = [x * R % P for x in (X, Y, Z)]
        if i % 3 == 0:
            m = [push_up(x, P, lim, rng, pick=0 if i % 4 < 2 else None)
                 for x, lim in zip(m, (SUB2X_OUT, 1 << 258, 1 << 258))]
            pushed[i % 2] += 1
        else:
            m = [x + P if rng.randrange(4) == 0 else x for x in m]
        x2, y2 = p2[0] * R % P, p2[1] * R % P
        if i % 2:
            cases.append(("madd", m + [x2, y2]))
            want.append(o.point_add(p1, p2))
        else:
            cases.append(("dbl", m))
            want.append(o.point_add(p1, p1))
    assert min(pushed) > 400
    res = run(harness, cases)
    bad = 0
    for (op, _), w, (X, Y, Z, _) in zip(cases, want, res):
        Xv, Yv, Zv = value(X) * RINV % P, value(Y) * RINV % P, value(Z) * RINV % P
        zi = pow(Zv, -1, P)
        got = (Xv * zi * zi % P, Yv * zi * zi * zi % P)
        if got != w or max(value(X), value(Y), value(Z)) >= (1 << 258) or not all(
                normalized(t) for t in (X, Y, Z)):
            bad += 1
    assert bad == 0


def test_table_build_regression(lib):
    """Crafted valid signatures whose u2 hits window-0 digits 30855, 61710
    and 61711 of the key that exposed the fold bug (W = 16), plus random ones."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    d = int.from_bytes(hashlib.sha256(b"c4 key 3").digest(), "big") % (o.N - 1) + 1
    q = o.pubkey(d)
    rng = random.Random(3)
    e_l, r_l, s_l = [], [], []
    for digit in [30855, 61710, 61711] * 3 + [rng.randrange(1, 1 << 16) for _ in range(7)]:
        while True:
            u1 = rng.randrange(1, o.N)
            u2 = ((rng.randrange(1, o.N >> 16) << 16) | digit) % o.N
            pt = o.point_add(o.scalar_mult(u1, o.G), o.scalar_mult(u2, q))
            r = pt[0] % o.N
            if r == 0:
                continue
            s = r * pow(u2, -1, o.N) % o.N
            e = u1 * s % o.N
            if s:
                break
        assert o.go_ecdsa_verify(q, e.to_bytes(32, "big"), r, s)
        e_l.append(e.to_bytes(32, "big"))
        r_l.append(r.to_bytes(32, "big"))
        s_l.append(s.to_bytes(32, "big"))
    arr = lambda l: np.frombuffer(b"".join(l), dtype=np.uint8).reshape(-1, 32)  # noqa: E731
    xy = np.frombuffer(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), dtype=np.uint8)
    with Authenticator(0) as a:
        a.set_key_window(16)
        slots, valid = a.register_points(xy[None, :])
        st = a.verify_prehashed(arr(e_l), arr(r_l), arr(s_l),
                                np.full(len(e_l), slots[0], dtype=np.uint32))
    assert (st == 0).all(), st


def test_chudnovsky_ops(harness):
    """The verifier's accumulator form (X, Y, ZZ = Z^2, ZZZ = Z^3) with the
    alternating Y sign and signed digits: ec_madd_chud and
    ec_add_affine_chud against big-integer point addition, every
    coordinate's bound and limb normalization checked."""
    from oracle import p256 as o
    rng = random.Random(0xC4D)
    pts = [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(48)]
    cases, want = [], []
    for i in range(3000):
        p1, p2 = pts[rng.randrange(48)], pts[rng.randrange(48)]
        if p1[0] == p2[0]:
            continue
        s_neg, t_neg, affine = rng.randrange(2) == 1, rng.randrange(2) == 1, i % 3 == 0
        z = 1 if affine else rng.randrange(1, P)
        X, Y = p1[0] * z * z % P, p1[1] * z * z * z % P
        m = [X * R % P, Y * R % P, z * z * R % P, z * z * z * R % P]
        if not affine:
            # non-canonical representatives up to the kernel's bounds: X up
            # to fe_sub_2x's 2^257 + 2^234, Y / ZZ / ZZZ up to 2^258
            lim = [SUB2X_OUT, 1 << 258, 1 << 258, 1 << 258]
            for k in range(4):
                top = (lim[k] - 1 - m[k]) // P
                pick = rng.randrange(4)
                m[k] += P * (top if pick == 0 else (rng.randrange(top + 1) if pick == 1 else 0))
        if s_neg:
            m[1] = (P - m[1] % P) % P + (P * rng.randrange(3) if not affine else 0)
        add_s2 = s_neg != t_neg
        op = ("aff_chud_n" if add_s2 else "aff_chud_p") if affine else \
             ("chud_n" if add_s2 else "chud_p")
        cases.append((op, m + [p2[0] * R % P, p2[1] * R % P]))
        w = o.point_add(p1, (p2[0], (P - p2[1]) % P) if t_neg else p2)
        # the sign the result's Y is stored in: the affine first addition
        # flips the accumulator's (-s Y3), the mixed addition takes the
        # digit's (t Y3, ecc.h ec_madd_chud)
        yneg = (not s_neg) if affine else t_neg
        want.append((w[0], (P - w[1]) % P if yneg else w[1]))
    res = run(harness, cases)
    bad = []
    for (op, _), w, (X, Y, ZZ, ZZZ) in zip(cases, want, res):
        Xv, Yv = value(X) * RINV % P, value(Y) * RINV % P
        zz, zzz = value(ZZ) * RINV % P, value(ZZZ) * RINV % P
        # consistent Chudnovsky point: ZZ^3 == ZZZ^2, x = X / ZZ, y = Y / ZZZ
        got = (Xv * pow(zz, -1, P) % P, Yv * pow(zzz, -1, P) % P)
        ok = got == w and pow(zz, 3, P) == pow(zzz, 2, P) and \
            max(value(X), value(Y), value(ZZ), value(ZZZ)) < (1 << 258) and \
            all(normalized(t) for t in (X, Y, ZZ, ZZZ))
        if not ok:
            bad.append(op)
    assert not bad, bad[:10]


def test_mul_add_bounds(harness):
    """fe_mul_add with the borrowed-limb constants at the bounds ec_madd_chud
    feeds it (fe29.h): H = x2 ZZ / R + (5p - X) with X up to 2^257 + 2^234
    (fe_sub_2x output) and ZZ < 2^258; R" = y2 ZZZ / R + (5p - Y) with y2
    canonical, ZZZ and Y < 2^258, ZZ / ZZZ also in their lazy form (limbs
    0..5 up to 2^32); and the older R' = (2p - y2) ZZZ / R + Y form.  Checks
    the value, normalization, that kP5B - X / Y and kP2B - y2 never borrow
    (every limb >= 0, < 2^30), and the documented output bound
    a b / R + p (1 + 2^-26) + w."""
    rng = random.Random(0x3ADD)
    cases = []
    for i in range(6000):
        x2 = rnd_value(rng, P)
        zz = rnd_value(rng, 1 << 258)
        X = rnd_value(rng, SUB2X_OUT if i % 2 else 1 << 258)
        cases.append(("muladd_p5b", [x2, lazy_limbs(zz, rng) if i % 3 else zz, X]))
        y2 = rnd_value(rng, P)
        zzz = rnd_value(rng, 1 << 258)
        Y = rnd_value(rng, 1 << 258)
        cases.append(("muladd_p2b", [y2, zzz, Y]))
    # the extremes themselves (the lazy extreme: every lazy limb at 2^32 - 1
    # where the value allows, lazy_limbs' greedy pick)
    top = (1 << 258) - 1
    cases.append(("muladd_p5b", [P - 1, top, SUB2X_OUT - 1]))
    cases.append(("muladd_p5b", [P - 1, top, top]))
    cases.append(("muladd_p5b", [P - 1, lazy_limbs(top, random.Random(1), greedy=True), top]))
    cases.append(("muladd_p2b", [P - 1, top, top]))
    cases.append(("muladd_p2b", [0, top, top]))
    res = run(harness, cases)
    bad = []
    for (op, (a, b, c)), (o0, _, _, _) in zip(cases, res):
        v = value(o0)
        b = value(b) if isinstance(b, list) else b
        if op == "muladd_p5b":
            wl = [k - x for k, x in zip(P5B, limbs(c))]
            aa, w = a, value(wl)
            want = (a * b * RINV + 5 * P - c) % P
        else:
            al = [k - x for k, x in zip(P2B, limbs(a))]
            wl = limbs(c)
            aa, w = value(al), c
            want = ((2 * P - a) * b * RINV + c) % P
            assert all(0 <= x < (1 << 30) for x in al), (hex(a), al)
        assert all(0 <= x < (1 << 30) for x in wl), (op, hex(c), wl)
        bound = aa * b // R + P + (P >> 26) + 1 + w
        if not (v % P == want and normalized(o0) and v < bound):
            bad.append((op, hex(a), hex(b), hex(c), hex(v)))
    assert not bad, bad[:5]


def lazy_limbs(v: int, rng: random.Random, greedy: bool = False) -> list:
    """A lazy representation of v (mont_reduce_p<.., 6>: limbs 0..5 below
    2^32, the rest normalized) with high bits set where v allows it
    (greedy: as many units moved down as fit)."""
    l = [(v >> (29 * k)) & MASK for k in range(8)] + [v >> 232]
    for k in range(5, -1, -1):  # move units of limb k+1 into limb k (+2^29 each)
        while l[k + 1] > 0 and l[k] + (1 << 29) < (1 << 32) and (greedy or rng.random() < 0.6):
            l[k + 1] -= 1
            l[k] += 1 << 29
    assert sum(x << (29 * k) for k, x in enumerate(l)) == v and all(x < (1 << 32) for x in l[:6])
    return l


def test_chudnovsky_lazy_and_last(harness):
    """The verifier's forms of ec_madd_chud: ZZ carried with lazy low limbs
    (fe29.h mont_reduce_p<.., LAZY = 6>, limbs 0..5 up to 2^32 - 1 from the
    one-mad carry) in and out, and the chain's final addition (LAST: X3 and
    ZZ3 only).  Against big-integer point addition; X, Y, ZZZ normalized,
    ZZ's lazy limbs below 2^32 and its value below 2^258, and fe_norm_lazy
    restoring the normalized form of the same value."""
    from oracle import p256 as o
    rng = random.Random(0x1A2)
    pts = [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(32)]
    cases, want = [], []
    for i in range(2400):
        p1, p2 = pts[rng.randrange(32)], pts[rng.randrange(32)]
        if p1[0] == p2[0]:
            continue
        s_neg, t_neg = rng.randrange(2) == 1, rng.randrange(2) == 1
        z = rng.randrange(1, P)
        X, Y = p1[0] * z * z % P, p1[1] * z * z * z % P
        m = [X * R % P, Y * R % P, z * z * R % P, z * z * z * R % P]
        lim = [SUB2X_OUT, 1 << 258, 1 << 258, 1 << 258]
        for k in range(4):
            top = (lim[k] - 1 - m[k]) // P
            m[k] += P * (top if i % 3 == 0 else rng.randrange(top + 1))
        if s_neg:
            m[1] = (P - m[1] % P) % P + P * rng.randrange(3)
        add_s2 = s_neg != t_neg
        kind = "last" if i % 4 == 0 else "lazy"
        op = f"chud_{kind}_" + ("n" if add_s2 else "p")
        zz = lazy_limbs(m[2], rng, greedy=i % 5 == 0)
        zzz = lazy_limbs(m[3], rng, greedy=i % 7 == 0)
        cases.append((op, [m[0], m[1], zz, zzz, p2[0] * R % P, p2[1] * R % P]))
        w = o.point_add(p1, (p2[0], (P - p2[1]) % P) if t_neg else p2)
        # Y3 is stored with the digit's sign (ecc.h ec_madd_chud: t Y3)
        want.append((kind, w[0], (P - w[1]) % P if t_neg else w[1], m[2]))
    res = run(harness, cases)
    bad = []

    def lazy_ok(l):
        return all(int(x) < (1 << 32) for x in l[:6]) and all(int(x) <= MASK for x in l[6:8]) and \
            value(l) < (1 << 258)

    for (op, inp), (kind, wx, wy, zz_in), (X, Y, ZZ, ZZZ) in zip(cases, want, res):
        Xv, zz = value(X) * RINV % P, value(ZZ) * RINV % P
        ok = Xv * pow(zz, -1, P) % P == wx and lazy_ok(ZZ) and normalized(X)
        if kind == "lazy":
            Yv, zzz = value(Y) * RINV % P, value(ZZZ) * RINV % P
            ok = ok and Yv * pow(zzz, -1, P) % P == wy and pow(zz, 3, P) == pow(zzz, 2, P) and \
                normalized(Y) and lazy_ok(ZZZ) and value(Y) < (1 << 258)
        if not ok:
            bad.append(op)
    assert not bad, bad[:10]
    # fe_norm_lazy: same value, normalized limbs
    vals = [rng.randrange(1 << 258) for _ in range(400)]
    res = run(harness, [("norm_lazy", [lazy_limbs(v, rng), 0, 0, 0, 0, 0]) for v in vals])
    assert all(value(r[0]) == v and normalized(r[0]) for v, r in zip(vals, res))


# ---------------------------------------------------------------------------
# The verifier's scalar side (scalar_dev.h), the joins of partial sums and the
# accept test: mod-N arithmetic, u1 / u2, the comb's recoding, the whole-wave
# inversion, ec_add_chud_x / _full, the wave-uniform forms, x_matches_r.
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
RNINV = pow(R, -1, N)
GROUP_OPS = {"add_full": 0, "add_x_same": 1, "add_x_diff": 2, "madd_p": 3, "madd_n": 4,
             "aff_p": 5, "aff_n": 6}
FN_OPS = {"fn_mul": 32, "fn_canon": 33, "fn_csub1": 34, "fn_to_mont": 35, "fn_from_mont": 36,
          "scalars": 37, "x_matches": 38}
OPS.update(FN_OPS)


@pytest.fixture(scope="module")
def harness2(harness):
    h = harness
    vp, i = ctypes.c_void_p, ctypes.c_int
    h.comb_check_run.argtypes = [vp, vp, i]
    h.modinv_wave_check_run.argtypes = [vp, vp, i]
    h.group_check_run.argtypes = [vp, vp, vp, i, i]
    for f in (h.comb_check_run, h.modinv_wave_check_run, h.group_check_run):
        f.restype = i
    return h


def words(v):
    """8 LE words of v < 2^256, in a 9-limb slot (raw, not limbs)."""
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)] + [0]


def from_words(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w[:8]))


def push_up(v, mod, bound, rng, pick=None):
    """A representative of v (mod `mod`) below `bound`: the value itself, the
    largest one, or a random one."""
    top = (bound - 1 - v) // mod
    pick = rng.randrange(3) if pick is None else pick
    return v + mod * (top if pick == 0 else (rng.randrange(top + 1) if pick == 1 else 0))


def golden_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_mod_n_ops(harness2):
    """fn_mul, fn_canon, fn_csub, fn_to_mont, fn_from_mont (fe29.h) run only
    on the device.  fn_mul on inputs up to 2^259 (adversarial limb patterns):
    value mod N, the documented bound a b / 2^261 + N and normalized limbs --
    a bound that fails makes the next fn_csub leave a non-canonical u.
    fn_canon at every multiple of N it must remove (k N - 1, k N, k N + 1,
    k = 0..4, and 2^258 - 1): exactly v mod N.  fn_csub(., 1) below 2N."""
    rng = random.Random(0xF0D)
    cases = []
    for _ in range(3000):
        cases.append(("fn_mul", [rnd_value(rng, 1 << 259), rnd_value(rng, 1 << 259)]))
        cases.append(("fn_canon", [rnd_value(rng, 1 << 258)]))
        cases.append(("fn_csub1", [rnd_value(rng, 2 * N)]))
        cases.append(("fn_to_mont", [rnd_value(rng, 1 << 256)]))
        cases.append(("fn_from_mont", [rnd_value(rng, 1 << 258)]))
    top = (1 << 259) - 1
    cases += [("fn_mul", [top, top]), ("fn_mul", [top, 0]), ("fn_mul", [N - 1, N - 1]),
              ("fn_mul", [(1 << 258) - 1, (1 << 256) - 1])]
    for k in range(5):
        cases += [("fn_canon", [k * N + d]) for d in (-1, 0, 1) if k * N + d >= 0]
    cases += [("fn_canon", [(1 << 258) - 1]), ("fn_canon", [(1 << 258) - (1 << 232)])]
    cases += [("fn_csub1", [v]) for v in (0, 1, N - 1, N, N + 1, 2 * N - 1)]
    cases += [("fn_to_mont", [v]) for v in (0, 1, N - 1, N, (1 << 256) - 1)]
    cases += [("fn_from_mont", [v]) for v in (0, 1, N - 1, N, (1 << 258) - 1)]
    res = run(harness2, cases)
    bad = []
    for (op, vals), (o0, _, _, _) in zip(cases, res):
        v, a = value(o0), vals[0]
        if op == "fn_mul":
            ok = v % N == a * vals[1] * RNINV % N and v < a * vals[1] // R + N + 1
        elif op == "fn_canon":
            ok = v == a % N
        elif op == "fn_csub1":
            ok = v == (a - N if a >= N else a)
        elif op == "fn_to_mont":
            ok = v % N == a * R % N and v < (1 << 258)
        else:
            ok = v % N == a * RNINV % N and v < a // R + N + 1
        if not (ok and normalized(o0)):
            bad.append((op, [hex(x) for x in vals], hex(v)))
    assert not bad, (len(bad), bad[:5])


def test_scalars_canonical(harness2):
    """scalars() (u1 = e w, u2 = r w): e and r anywhere below 2^256 (0, N - 1,
    N, 2^256 - 1 among them: Go reduces e, and r + N enters elsewhere), w ANY
    representative below 2^258 of a Montgomery-form value, the bound the
    single conditional subtraction rests on.  Both outputs exactly
    e w 2^-261 mod N as canonical words: a non-canonical u (u + N) recodes
    into other comb digits and rejects a valid signature on the GPU alone."""
    rng = random.Random(0x5CA1)
    fixed = [0, 1, N - 1, N, N + 1, (1 << 256) - 1, 1 << 255]
    cases = []
    for i in range(3000):
        e = fixed[i % 7] if i % 5 == 0 else rnd_value(rng, 1 << 256)
        r = fixed[(i // 7) % 7] if i % 3 == 0 else rnd_value(rng, 1 << 256)
        w = push_up(rng.randrange(N) * R % N, N, 1 << 258, rng, pick=i % 3)
        cases.append(("scalars", [e, r, w]))
    wmax = push_up(rng.randrange(N), N, 1 << 258, rng, pick=0)   # the largest representative
    assert (1 << 258) - N <= wmax < (1 << 258)
    cases += [("scalars", [(1 << 256) - 1, (1 << 256) - 1, (1 << 258) - 1]),
              ("scalars", [(1 << 256) - 1, N - 1, wmax]), ("scalars", [0, 0, (1 << 258) - 1])]
    res = run(harness2, cases)
    bad = []
    for (_, (e, r, w)), (o0, o1, _, _) in zip(cases, res):
        assert w < (1 << 258)
        u1, u2 = from_words(o0), from_words(o1)
        if u1 != e * w * RNINV % N or u2 != r * w * RNINV % N:
            bad.append((hex(e), hex(r), hex(w), hex(u1), hex(u2)))
    assert not bad, (len(bad), bad[:5])


def test_comb_recoding(harness2):
    """comb_digit / shr_words over whole scalars at every window 4..29: the
    loop every verify form runs, against make_golden.signed_digits.  The
    scalars include the recoding's corners (tests/golden/scalar_edges.json's
    u: a carry into the top window -> digit 2^L, the table's last entry; a
    window exactly 2^(W-1); all ones plus a carry -> a zero digit that still
    carries).  Every index must lie inside its window's entry count: one
    past it reads the next window's (or the next key's) first entry."""
    mg = golden_module()
    rng = random.Random(0xD161)
    us = [u for _, u in mg.scalar_edge_values(random.Random(0x45444745))]
    us += [0, N - 2, (1 << 256) - 1, 1 << 255, (1 << 255) + 1, N - (1 << 200)]
    us += [rng.randrange(1 << 256) for _ in range(24)]
    us += [rnd_value(rng, 1 << 256) for _ in range(8)]
    cases = [(u, W) for u in us for W in range(4, 30)]
    inp = np.array([words(u)[:8] + [W] for u, W in cases], dtype=np.uint32)
    out = np.zeros((len(cases), 64), dtype=np.uint32)
    assert harness2.comb_check_run(inp.ctypes.data, out.ctypes.data, len(cases)) == 0
    bad = []
    for (u, W), row in zip(cases, out.tolist()):
        dig = mg.signed_digits(u, W)
        S = len(dig)
        L = 256 - (S - 1) * W
        want = []
        for k, d in enumerate(dig):
            assert abs(d) <= (1 << (L if k == S - 1 else W - 1))
            want.append((0 if d == 0 else abs(d) - 1) | (1 << 30 if d < 0 else 0) | (1 << 31 if d == 0 else 0))
        # (a zero digit's sign is not read: all ones plus a carry reports it
        # negative, since that is what carries)
        got = [x & ~(1 << 30) if x >> 31 else x for x in row[:S]]
        if got != want or any(x != 0xFFFFFFFF for x in row[S:]):
            bad.append((hex(u), W))
    assert not bad, (len(bad), bad[:5])
    # the named corners are present
    assert any(mg.signed_digits(u, 29)[-1] == 1 << 24 for u in us)
    assert any(0 in mg.signed_digits(u, 8)[1:-1] and u == (1 << 255) - 1 for u in us)


def test_modinv_wave(harness2):
    """modinv_n_var_wave (the roots of the batched s^-1, one value per wave,
    the 2x2 matrix split over lane quads with DPP broadcasts): every one of
    the 64 lanes returns pow(x, -1, N) and true; 0 returns false.  A lane
    quad out of step would hand one lane another lane's half of the update."""
    rng = random.Random(0x1A7E)
    xs = [1, 2, 3, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2] + [1 << k for k in range(1, 256, 15)] + \
         [1 << 255, (1 << 255) - 1] + [rng.randrange(1, N) for _ in range(40)] + \
         [rnd_value(rng, N) or 1 for _ in range(8)]
    xs.append(0)
    inp = np.array([words(x)[:8] for x in xs], dtype=np.uint32)
    out = np.zeros((len(xs), 64, 9), dtype=np.uint32)
    assert harness2.modinv_wave_check_run(inp.ctypes.data, out.ctypes.data, len(xs)) == 0
    bad = []
    for x, lanes in zip(xs, out):
        assert (lanes == lanes[0]).all(), hex(x)
        got, ok = from_words(lanes[0]), int(lanes[0][8])
        if x == 0:
            if ok != 0:
                bad.append((hex(x), ok))
        elif ok != 1 or got != pow(x, -1, N):
            bad.append((hex(x), ok, hex(got)))
    assert not bad, bad[:5]


def run_group(h, cases, wide):
    """cases: (op, [8 values or limb lists]) -> per case (wide: per case and
    lane) the 37 output words."""
    n = len(cases)
    op = np.array([GROUP_OPS[c[0]] for c in cases], dtype=np.uint32)
    inp = np.zeros((n, 72), dtype=np.uint32)
    for i, (_, vals) in enumerate(cases):
        for k, v in enumerate(vals):
            inp[i, 9 * k: 9 * k + 9] = v if isinstance(v, list) else limbs(v)
    out = np.zeros((n, 64, 37) if wide else (n, 37), dtype=np.uint32)
    assert h.group_check_run(op.ctypes.data, inp.ctypes.data, out.ctypes.data, n, 1 if wide else 0) == 0
    return out


CHUD_LIM = [SUB2X_OUT, 1 << 258, 1 << 258, 1 << 258]


def chud_rep(pt, z, rng, yneg=False, pick=None):
    """(X, Y, ZZ, ZZZ) of the affine point with Z = z, Montgomery form, each
    coordinate a representative up to the bound the joins take as inputs
    (X < 2^257 + 2^234, the others < 2^258); yneg: Y holds -Y."""
    y = (P - pt[1]) % P if yneg else pt[1]
    m = [pt[0] * z * z % P, y * z * z * z % P, z * z % P, z * z * z % P]
    return [push_up(v * R % P, P, lim, rng, pick) for v, lim in zip(m, CHUD_LIM)]


def other_point(pts, p1, rng):
    while True:
        p2 = pts[rng.randrange(len(pts))]
        if p2[0] != p1[0]:
            return p2


def test_chud_joins(harness2):
    """ec_add_chud_full (k_verify_split's joins of partial comb sums, TRUE Y)
    and ec_add_chud_x (k_verify_pairs' x-only join, Y under the caller's sign
    convention, both same_sign values) on two Chudnovsky points whose
    coordinates are non-canonical representatives up to their documented
    bounds -- where the fold of fe_sub once went negative.  The affine result
    against big-integer addition; for the full form the true Y and
    ZZ^3 == ZZZ^2; outputs inside the bounds the next join level takes as
    inputs; true returned.  b = a and b = -a under another Z return false
    (the caller then takes the exact path)."""
    from oracle import p256 as o
    rng = random.Random(0x101A)
    pts = [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(48)]
    cases, want = [], []
    planned = 3000
    for i in range(planned):
        p1 = pts[rng.randrange(48)]
        p2 = other_point(pts, p1, rng)
        pick = 0 if i % 4 == 0 else None
        if i % 2 == 0:
            a = chud_rep(p1, rng.randrange(1, P), rng, pick=pick)
            b = chud_rep(p2, rng.randrange(1, P), rng, pick=pick)
            cases.append(("add_full", a + b))
        else:
            sa, sb = rng.randrange(2) == 1, rng.randrange(2) == 1
            a = chud_rep(p1, rng.randrange(1, P), rng, yneg=sa, pick=pick)
            b = chud_rep(p2, rng.randrange(1, P), rng, yneg=sb, pick=pick)
            cases.append(("add_x_same" if sa == sb else "add_x_diff", a + b))
        want.append(o.point_add(p1, p2))
    ndeg = 0
    for i in range(60):   # degenerate: the same point, or its negative, under another Z
        p1 = pts[rng.randrange(48)]
        neg = i % 2 == 1
        a = chud_rep(p1, rng.randrange(1, P), rng)
        b = chud_rep(p1, rng.randrange(1, P), rng, yneg=neg)
        cases.append((("add_full", "add_x_same", "add_x_diff")[i % 3], a + b))
        want.append(None)
        ndeg += 1
    assert len(cases) == planned + ndeg
    out = run_group(harness2, cases, wide=False)
    bad, seen = [], {"add_full": 0, "add_x_same": 0, "add_x_diff": 0, None: 0}
    for (op, _), w, row in zip(cases, want, out):
        X, Y, ZZ, ZZZ, ret = row[0:9], row[9:18], row[18:27], row[27:36], int(row[36])
        if w is None:
            seen[None] += 1
            if ret != 0:
                bad.append((op, "degenerate", ret))
            continue
        seen[op] += 1
        zz = value(ZZ) * RINV % P
        ok = ret == 1 and zz != 0 and value(X) * RINV * pow(zz, -1, P) % P == w[0] and \
            value(X) < SUB2X_OUT and value(ZZ) < (1 << 258) and normalized(X) and normalized(ZZ)
        if ok and op == "add_full":
            zzz = value(ZZZ) * RINV % P
            ok = value(Y) * RINV * pow(zzz, -1, P) % P == w[1] and pow(zz, 3, P) == pow(zzz, 2, P) and \
                value(Y) < (1 << 258) and value(ZZZ) < (1 << 258) and normalized(Y) and normalized(ZZZ)
        if not ok:
            bad.append((op, ret))
    assert not bad, (len(bad), bad[:10])
    assert sum(seen.values()) == planned + ndeg and seen["add_full"] == planned // 2 and \
        seen["add_x_same"] > 300 and seen["add_x_diff"] > 300 and seen[None] == ndeg


def test_wide_forms_match_sequential(harness2):
    """ec_madd_chud_wide, ec_add_affine_chud_wide and ec_add_chud_full_wide
    (k_verify_split: one item per wave, the products of each dependency level
    in different 16-lane groups) against ecc.h's promise "the same results
    bit for bit": one case per 64-lane block, every lane's outputs equal and
    limb for limb those of the sequential form on the same inputs (which the
    tests above pin against big integers).  A wrong operand select in one
    lane group, or a broadcast from the wrong group's first lane, differs."""
    from oracle import p256 as o
    rng = random.Random(0x51DE)
    pts = [o.scalar_mult(rng.randrange(1, o.N), o.G) for _ in range(32)]
    cases = []
    planned = 900
    for i in range(planned):
        p1 = pts[rng.randrange(32)]
        p2 = other_point(pts, p1, rng)
        pick = 0 if i % 4 == 0 else None
        kind = i % 3
        if kind == 0:
            a = chud_rep(p1, rng.randrange(1, P), rng, pick=pick)
            b = chud_rep(p2, rng.randrange(1, P), rng, pick=pick)
            cases.append(("add_full", a + b))
        elif kind == 1:
            a = chud_rep(p1, rng.randrange(1, P), rng, yneg=rng.randrange(2) == 1, pick=pick)
            cases.append((("madd_p", "madd_n")[rng.randrange(2)],
                          a + [p2[0] * R % P, p2[1] * R % P, 0, 0]))
        else:
            y1 = p1[1] if rng.randrange(2) else P - p1[1]
            cases.append((("aff_p", "aff_n")[rng.randrange(2)],
                          [p1[0] * R % P, y1 * R % P, 0, 0, p2[0] * R % P, p2[1] * R % P, 0, 0]))
    for i in range(12):   # degenerate full additions: false in both forms
        p1 = pts[i]
        cases.append(("add_full", chud_rep(p1, rng.randrange(1, P), rng) +
                      chud_rep(p1, rng.randrange(1, P), rng, yneg=i % 2 == 1)))
    assert len(cases) == planned + 12
    seq = run_group(harness2, cases, wide=False)
    wide = run_group(harness2, cases, wide=True)
    bad = []
    for k, ((op, _), s_row, w_rows) in enumerate(zip(cases, seq, wide)):
        want_ret = 0 if k >= planned else 1
        if int(s_row[36]) != want_ret or not (w_rows[:, 36] == want_ret).all():
            bad.append((op, k, "ret"))
        elif want_ret and not (w_rows == s_row[None, :]).all():
            bad.append((op, k, np.nonzero((w_rows != s_row[None, :]).any(axis=1))[0][:4].tolist()))
    assert not bad, (len(bad), bad[:10])


def test_x_matches_r(harness2):
    """The line that decides accept (x_matches_r, verify_finish's merged
    product r ZZ + X (p - 1), then the same with r + N entering as un-carried
    limbs) on pure field inputs X = x z^2 R, ZZ = z^2 R at their bounds, for
    any x in [0, p): true exactly when r == x mod N -- r = x - N for x >= N,
    up to x = p - 1, r = p - N - 1 -- and false for r +- 1, for r = x - N + 1,
    for r = p - N with x = 0 and every r = x + p - N >= p - N (Go does not try
    r + N there: a wrap mod p must not accept), and for r = x + N - p (a
    verifier that subtracted N would accept).  r always in [1, N)."""
    rng = random.Random(0xACCE)
    xs = [0, 1, 2, N - 2, N - 1, N, N + 1, P - N - 2, P - N - 1, P - N, P - N + 1, P - 2, P - 1,
          2 * N - P - 1, 2 * N - P, 2 * N - P + 1]
    xs += [rng.randrange(N, P) for _ in range(150)]
    xs += [rng.randrange(P - N) for _ in range(150)]
    xs += [rng.randrange(P) for _ in range(300)]
    xs += [rnd_value(rng, P) for _ in range(100)]
    cases, meta = [], []

    def add(x, r, name):
        if not 1 <= r < N:
            return
        z = rng.randrange(1, P)
        X = push_up(x * z * z * R % P, P, 1 << 258, rng)
        ZZ = push_up(z * z * R % P, P, 1 << 258, rng)
        cases.append(("x_matches", [X, ZZ, words(r)]))
        meta.append((x, r, name))

    for x in xs:
        rt = x % N
        add(x, rt, "true")
        add(x, rt + 1, "r_plus_1")
        add(x, rt - 1, "r_minus_1")
        add(x, x - N + 1, "x_minus_N_plus_1")
        add(x, x + P - N, "wraps_mod_p")        # r + N == x + p: only below 2N - p is r < N
        add(x, x + N - P, "x_plus_N_minus_p")   # r == x + N (mod p)
        add(x, rng.randrange(1, N), "random_r")
    res = run(harness2, cases)
    names = {m[2] for m in meta}
    assert names == {"true", "r_plus_1", "r_minus_1", "x_minus_N_plus_1", "wraps_mod_p",
                     "x_plus_N_minus_p", "random_r"}
    assert (0, P - N, "wraps_mod_p") in meta and (P - 1, P - N - 1, "true") in meta
    bad = []
    for (x, r, name), (o0, _, _, _) in zip(meta, res):
        want = x % N == r
        assert want == (name == "true") or name == "random_r", (hex(x), hex(r), name)
        if int(o0[0]) != int(want):
            bad.append((name, hex(x), hex(r), int(o0[0])))
    assert not bad, (len(bad), bad[:10])
