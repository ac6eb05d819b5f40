"""The vectors and the model of the P-384 arithmetic checks, shared by the host
run (tests/test_p384_host.py, tests/p384_host_check) and the device run
(tests/test_gpu_p384_field.py, tests/libp384_check.so): both execute the
operation table of tests/csrc/p384_check_ops.inc, and check(op, operands,
results) compares one answer with Python integers.  The vectors are built once
(cases()) and never changed."""
import functools
import json
import os
import random

import p384_ref as o

HERE = os.path.dirname(os.path.abspath(__file__))
R = 1 << 392
P, N = o.P, o.N
RI_P, RI_N = pow(R, -1, P), pow(R, -1, N)
OPS = {"mul": (2, 1), "sqr": (1, 1), "add": (2, 1), "sub": (2, 1), "dbl": (1, 1), "tpl": (1, 1), "canon": (1, 1),
       "tomont": (1, 1), "frommont": (1, 1), "inv": (1, 1), "eq": (2, 1), "words": (1, 1), "nmul": (2, 1),
       "ninv": (1, 1), "nreduce": (1, 1), "u1u2": (3, 2), "padd": (6, 3), "pdbl": (3, 3), "finish": (3, 1),
       "oncurve": (2, 1), "item": (5, 1), "shamir": (4, 3)}
ALL_ONES_LIMBS = sum(((1 << 28) - 1) << (28 * i) for i in range(14))  # 2^392 - 1: every limb all ones


def fixtures():
    with open(os.path.join(HERE, "golden", "p384_edges.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def item_statuses():
    return {tuple(int(v[k], 16) for k in "ersxy"): v["status"] for v in fixtures() if v["kind"] == "prehashed"}


def field_values(rng, count):
    """0, 1, p - 1, p - 2, values whose limbs are all ones, and random elements."""
    special = [0, 1, 2, P - 1, P - 2, P, P + 1, 2 * P - 1, (1 << 384) - 1, 1 << 384, (1 << 385) - 1,
               ALL_ONES_LIMBS >> 7, ALL_ONES_LIMBS >> 4, (1 << 364) - 1, ((1 << 28) - 1) << 28 * 7, R % P, R * R % P]
    return special + [rng.randrange(P) for _ in range(count)] + [rng.getrandbits(385) for _ in range(count // 2)]


@functools.lru_cache(maxsize=None)
def cases():
    """[(op, operands)]: every operation's vectors, in one fixed order."""
    rng = random.Random(1384)
    out = []
    vals = field_values(rng, 24)
    mulvals = [v for v in vals if v < 1 << 388]
    for a in mulvals:
        b = rng.choice(mulvals)
        out.append(("mul", (a, b)))
        out.append(("sqr", (a,)))
    out += [("mul", (a, b)) for a in (P - 1, ALL_ONES_LIMBS >> 4, (1 << 388) - 1) for b in (P - 1, ALL_ONES_LIMBS >> 4, (1 << 388) - 1)]
    for a in vals:
        b = rng.choice(vals)
        out.append(("add", (a, b)))
        out.append(("sub", (a, b)))        # b < 2^388.9 = 32 p holds for every value above
        out.append(("dbl", (a,)))
        out.append(("tpl", (a,)))
        out.append(("canon", (a,)))
        out.append(("eq", (a, b)))
        out.append(("eq", (a, a + P if a + P < R else a)))
        out.append(("tomont", (a,)))
        out.append(("frommont", (a,)))
    out += [("sub", (a, b)) for a in (0, 1, P - 1, (1 << 391) - 1) for b in (0, 1, P - 1, 32 * P - 1, ALL_ONES_LIMBS >> 4)]
    out += [("canon", (v,)) for v in (ALL_ONES_LIMBS, R - P, 255 * P, 255 * P - 1, 256 * P + 5)]
    for a in [1, 2, P - 1, P - 2, R % P, ALL_ONES_LIMBS >> 7] + [rng.randrange(1, P) for _ in range(6)]:
        out.append(("inv", (a,)))
    for a in [0, 1, P - 1, P, N, N - 1, (1 << 384) - 1, 0xFFFFFFF << 28 * 6] + [rng.getrandbits(384) for _ in range(8)]:
        out.append(("words", (a,)))
        out.append(("nreduce", (a,)))
    svals = [0, 1, N - 1, N - 2, N, N + 1, (1 << 384) - 1, (1 << 385) - 1, ALL_ONES_LIMBS >> 7] + [rng.randrange(N) for _ in range(16)]
    for a in svals:
        out.append(("nmul", (a, rng.choice(svals))))
    for a in [1, 2, N - 1, N - 2, R % N] + [rng.randrange(1, N) for _ in range(6)]:
        out.append(("ninv", (a,)))
    for e in (0, 1, N - 1, N, N + 1, (1 << 384) - 1, rng.getrandbits(384), rng.getrandbits(384)):
        for s in (1, N - 1, rng.randrange(1, N)):
            out.append(("u1u2", (e, rng.choice((1, N - 1, rng.randrange(1, N))), s)))
    # the complete addition: (P, P), (P, -P), (P, O), (O, P), (O, O), distinct points, any projective scale
    pts = [o.G, o.mul(2, o.G), o.mul(rng.randrange(1, N), o.G), o.mul(N - 1, o.G)]
    inf = (0, 1, 0)

    def proj(pt, scale=True):
        if pt is None:
            return (0, rng.randrange(1, P) if scale else 1, 0)
        z = rng.randrange(1, P) if scale else 1
        return (pt[0] * z % P, pt[1] * z % P, z)

    for a in pts:
        for b, sc in ((a, True), (a, False), (o.neg(a), True), (o.neg(a), False), (None, True), (pts[2], True)):
            out.append(("padd", proj(a, sc) + proj(b, sc)))
            out.append(("padd", proj(b, sc) + proj(a, sc)))
        out.append(("pdbl", proj(a)))
        out.append(("pdbl", proj(a, False)))
    out.append(("padd", inf + inf))
    out.append(("padd", proj(None) + proj(None)))
    out.append(("pdbl", inf))
    out.append(("pdbl", proj(None)))
    # the finish on an injected (X, Z): x = r, x = r + N with r + N < p, x = r + N read mod p, Z = 0
    for r in (1, 5, P - N - 1, rng.randrange(1, P - N)):
        for x in (r, r + N, r + 1, (r + N + 1) % P):
            z = rng.randrange(1, P)
            out.append(("finish", (x * z % P, z, r)))
        out.append(("finish", (r, 0, r)))
    for r in (P - N, P - N + 1, N - 1, rng.randrange(P - N, N)):  # r + N >= p: only x = r holds
        z = rng.randrange(1, P)
        out.append(("finish", (r * z % P, z, r)))
        out.append(("finish", ((r + N) % P * z % P, z, r)))
    # points and whole items
    for v in fixtures():
        if v["kind"] == "prehashed":
            e, r, s, x, y = (int(v[k], 16) for k in "ersxy")
            out.append(("oncurve", (x, y)))
            out.append(("item", (e, r, s, x, y)))
    q = pts[2]
    for u1, u2 in ((0, 0), (1, 0), (0, 1), (1, 1), (N - 1, N - 1), (N - 1, 1), (rng.randrange(N), rng.randrange(N)),
                   ((1 << 384) - 1, (1 << 383) + 1)):
        out.append(("shamir", (u1, u2, q[0], q[1])))
    out.append(("shamir", (5, 5, *o.neg(o.G))))
    out.append(("shamir", (5, 7, *o.G)))
    return tuple(out)


def _same_point(got, want_affine, what):
    x, y, z = got
    assert max(got) < P, what
    if want_affine is None:
        assert z == 0 and y != 0 and x == 0, what
    else:
        assert z != 0 and (x - want_affine[0] * z) % P == 0 and (y - want_affine[1] * z) % P == 0, what


def check(op, a, got):
    """got: the operation's results as integers."""
    what = (op, [hex(v) for v in a], [hex(v) for v in got])
    g = got[0]
    if op in ("mul", "sqr"):
        b = a[1] if op == "mul" else a[0]
        assert g % P == a[0] * b * RI_P % P and g < a[0] * b // R + P + 1, what
        assert a[0] * b >= 1 << 776 or g < 1 << 385, what
    elif op == "add":
        assert g == a[0] + a[1], what
    elif op == "sub":
        assert g % P == (a[0] - a[1]) % P and g < (1 << 384) + (1 << 137), what
    elif op == "dbl":
        assert g == 2 * a[0], what
    elif op == "tpl":
        assert g == 3 * a[0], what
    elif op == "canon":
        assert g == a[0] % P, what
    elif op == "tomont":
        assert g % P == a[0] * R % P and g < 1 << 385, what
    elif op == "frommont":
        assert g % P == a[0] * RI_P % P and g < a[0] // R + P + 1, what
    elif op == "inv":
        assert g % P == pow(a[0], -1, P) * R * R % P and g < 1 << 385, what
    elif op == "eq":
        assert g == int(a[0] % P == a[1] % P), what
    elif op == "words":
        assert g == a[0], what
    elif op == "nmul":
        assert g % N == a[0] * a[1] * RI_N % N and g < a[0] * a[1] // R + N + 1, what
    elif op == "ninv":
        assert g % N == pow(a[0], -1, N) * R * R % N and g < 1 << 385, what
    elif op == "nreduce":
        assert g == a[0] % N, what
    elif op == "u1u2":
        w = pow(a[2], -1, N)
        assert tuple(got) == (a[0] * w % N, a[1] * w % N), what
    elif op == "padd":
        assert tuple(got) == o.rcb_add(a[:3], a[3:]), what  # the same formulas: the same coordinates
        _same_point(got, o.add(o.to_affine(a[:3]), o.to_affine(a[3:])), what)
    elif op == "pdbl":
        assert tuple(got) == o.rcb_dbl(a), what
        pt = o.to_affine(a)
        _same_point(got, o.add(pt, pt), what)
    elif op == "finish":
        x, z, r = a
        want = z % P != 0 and (x * pow(z, -1, P) % P) % N == r
        assert g == int(want), what
    elif op == "oncurve":
        assert g == int(o.on_curve(*a)), what
    elif op == "item":
        assert g == item_statuses()[tuple(a)], what  # (the fixture's status: tests/test_p384_ref.py checks those)
    elif op == "shamir":
        u1, u2, qx, qy = a
        _same_point(got, o.add(o.mul(u1, o.G), o.mul(u2, (qx, qy))), what)
    else:
        raise AssertionError(op)


def finish_cases_cover():
    """The injected finishes hold an accepted x = r + N."""
    n = 0
    for op, a in cases():
        if op == "finish" and a[1] and a[2] < P - N and a[0] * pow(a[1], -1, P) % P == a[2] + N:
            n += 1
    return n
