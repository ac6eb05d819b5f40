"""The key memory budget's plan (minbft_amd/csrc/key_plan.h): the modelled cost
of a class, the use-count bins, the ladder rule and rebalance_plan -- plain
C++, driven through the stand-alone program tests/key_budget_check (built by
__graft_entry__.build() from tests/csrc/key_budget_check.cpp) and compared with
models written here.  No GPU."""
import math
import os
import random
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "key_budget_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"

NBINS = 496


def T(t):
    return 0x100 | t


def S(t):
    return 0x200 | t


CLASSES = [0] + [T(t) for t in range(2, 9)] + [S(t) for t in range(2, 10)] + list(range(4, 30))


def class_bytes(cls):
    if cls == 0:
        return 64
    if cls >= 0x200:
        return 64 << ((cls & 0xFF) - 1)
    if cls >= 0x100:
        return 64 << (cls & 0xFF)
    s = -(-256 // cls)
    return 64 * (((s - 1) << (cls - 1)) + (1 << (256 - (s - 1) * cls)))


def class_cost(cls):
    """The modelled reductions of u2 Q, restated from the issue of the
    classes: a doubling 8, an addition 10."""
    if cls not in CLASSES:
        return 0
    if cls == 0:
        return 256 * 8 + 86 * 10
    if cls >= 0x100:
        return 18 * -(-256 // (cls & 0xFF)) - 8
    return 10 * -(-256 // cls)


def use_bin(u):
    if u < 16:
        return u
    e = u.bit_length() - 1
    return 16 + 8 * (e - 4) + ((u >> (e - 3)) & 7)


def bin_low(b):
    if b < 16:
        return b
    e, m = 4 + (b - 16) // 8, (b - 16) % 8
    return (8 + m) << (e - 3)


def ladder_ok(cls):
    if not 1 <= len(cls) <= 8 or any(c not in CLASSES for c in cls):
        return False
    b, c = [class_bytes(x) for x in cls], [class_cost(x) for x in cls]
    if any(b[j] >= b[j + 1] or c[j] <= c[j + 1] for j in range(len(cls) - 1)):
        return False
    g = [Fraction(c[j] - c[j + 1], b[j + 1] - b[j]) for j in range(len(cls) - 1)]
    return all(g[j] > g[j + 1] for j in range(len(g) - 1))


def plan_model(hist, cls, avail, min_uses):
    """rung per bin, bytes, excess, and the ordered steps with the index of
    the one that did not fit (None: all were taken)."""
    b, c = [class_bytes(x) for x in cls], [class_cost(x) for x in cls]
    rung = [0] * NBINS
    total = sum(hist) * b[0]
    if total > avail:
        return rung, total, total - avail, [], None
    steps = [(k, j) for k in range(NBINS) if hist[k] and bin_low(k) >= max(min_uses, 1) for j in range(len(cls) - 1)]
    steps.sort(key=lambda s: (-bin_low(s[0]) * Fraction(c[s[1]] - c[s[1] + 1], b[s[1] + 1] - b[s[1]]), -s[0], s[1]))
    blocked = None
    for i, (k, j) in enumerate(steps):
        more = hist[k] * (b[j + 1] - b[j])
        if total + more > avail:
            blocked = i
            break
        assert rung[k] == j
        total += more
        rung[k] = j + 1
    return rung, total, 0, steps, blocked


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as ge
    return ge.build_key_budget_check()


def run(prog, lines):
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")[:-1]


def bin_points():
    pts = list(range(41))
    for k in range(4, 64):
        pts += [2 ** k - 1, 2 ** k, 2 ** k + 2 ** (k - 3) - 1, 2 ** k + 2 ** (k - 3)]
    pts.append(2 ** 64 - 1)
    rng = random.Random(11)
    pts += [min(2 ** 64 - 1, int(2 ** rng.uniform(0, 64))) for _ in range(10000)]
    return pts


def check_bins(prog):
    pts = bin_points()
    got = [int(x) for x in run(prog, ["bin %d" % u for u in pts])]
    assert got == [use_bin(u) for u in pts]
    # monotone over the sorted points, the whole range of bins reached
    order = sorted(range(len(pts)), key=lambda i: pts[i])
    assert all(got[order[i]] <= got[order[i + 1]] for i in range(len(order) - 1))
    assert got[pts.index(0)] == 0 and got[pts.index(2 ** 64 - 1)] == NBINS - 1
    lows = [int(x) for x in run(prog, ["low %d" % b for b in range(NBINS)])]
    assert lows == [bin_low(b) for b in range(NBINS)]
    assert all(lows[b] < lows[b + 1] for b in range(NBINS - 1))
    back = [int(x) for x in run(prog, ["bin %d" % u for u in lows])]
    assert back == list(range(NBINS))
    # a bin's least count is its least: the count before it lies in the bin before
    prev = [int(x) for x in run(prog, ["bin %d" % (u - 1) for u in lows[1:]])]
    assert prev == list(range(NBINS - 1))


def test_use_bins(prog):
    check_bins(prog)


def test_class_cost(prog):
    codes = list(range(0, 40)) + list(range(0x100, 0x10C)) + list(range(0x200, 0x20C)) + [0x300, 0xFFFFFFFF]
    out = [int(x) for x in run(prog, ["cost %d" % c for c in codes])]
    assert out == [class_cost(c) for c in codes]
    # the documented figures: the ladder 2,908; 64 columns at t = 4; 16 windows at W = 16
    assert class_cost(0) == 2908 and class_cost(T(4)) == class_cost(S(4)) == 18 * 64 - 8 and class_cost(16) == 160
    assert all(class_cost(c) > 0 for c in CLASSES)


EIGHT = [0, S(2), S(3), S(4), S(5), S(7), S(9), 8]
GOOD_LADDERS = [[0, S(5), S(9), 16], [0, S(2), S(3)], [0], [16], EIGHT]
BAD_LADDERS = [
    [S(5), 0],                 # bytes descending
    [0, S(5), T(4)],           # equal bytes
    [0, S(9), 4],              # window 4 costs more than signed 9: dominated
    [0, T(2), S(4)],           # the second step gains more per byte than the first: not convex
    [0, 3], [0, 30], [0, T(9)], [0, S(10)], [0, 0x300],   # unknown codes
    [],                        # no rung
    EIGHT + [12],              # nine
    [0, 0],
]


def test_ladder_rule(prog):
    rng = random.Random(13)
    cases = GOOD_LADDERS + BAD_LADDERS
    for _ in range(400):
        cases.append(sorted(rng.sample(CLASSES, rng.randrange(1, 6)), key=class_bytes))
    for _ in range(50):
        cases.append(rng.sample(CLASSES, rng.randrange(1, 10)))
    out = [int(x) for x in run(prog, ["ladder %d %s" % (len(c), " ".join(map(str, c))) for c in cases])]
    assert out == [int(ladder_ok(c)) for c in cases]
    assert all(ladder_ok(c) for c in GOOD_LADDERS) and not any(ladder_ok(c) for c in BAD_LADDERS)
    assert sum(out[len(GOOD_LADDERS) + len(BAD_LADDERS):]) > 20   # the random ones hit both answers


def plan_cases():
    rng = random.Random(17)
    ladders = [[0], [S(4)], [0, S(5)], [0, 8], [0, S(3), S(6), 8], [0, S(5), S(9), 16], EIGHT]
    cases = []
    for i in range(300):
        cls = ladders[i % len(ladders)]
        kind = i % 5
        hist = [0] * NBINS
        if kind == 1:
            hist[rng.randrange(NBINS)] = rng.randrange(1, 1000)         # one bin
        elif kind != 0:                                                   # (kind 0: empty)
            for _ in range(rng.randrange(1, 40)):
                hist[min(NBINS - 1, int(rng.expovariate(1 / 60.0)))] += rng.choice([1, 1, 2, 17, 1000, 250000])
        rung0 = sum(hist) * class_bytes(cls[0])
        top = sum(hist) * class_bytes(cls[-1])
        avail = rng.choice([0, rung0 - 1 if rung0 else 0, rung0, rung0 + 1, rung0 + class_bytes(cls[-1]),
                            rng.randrange(rung0, top + 1), (rung0 + top) // 2, top - 1, top, top + 12345, 2 ** 64 - 1])
        cases.append((hist, cls, max(avail, 0), [0, 1, 100][i % 3]))
    return cases


def check_plans(prog, cases):
    cmds = []
    for hist, cls, avail, mu in cases:
        nz = [(b, h) for b, h in enumerate(hist) if h]
        cmds.append("plan %d %s %d %d %d" % (len(cls), " ".join(map(str, cls)), avail, mu, len(nz)))
        cmds += ["%d %d" % bh for bh in nz]
    out = run(prog, cmds)
    assert len(out) == 2 * len(cases)
    seen = set()
    for k, (hist, cls, avail, mu) in enumerate(cases):
        nbytes, excess, bbin, brung = (int(x) for x in out[2 * k].split())
        rung = [int(ch) for ch in out[2 * k + 1]]
        want, wbytes, wexcess, steps, blocked = plan_model(hist, cls, avail, mu)
        assert rung == want and (nbytes, excess) == (wbytes, wexcess), (k, cls, avail, mu)
        assert (bbin, brung) == (steps[blocked] if blocked is not None else (-1, -1))
        # the invariants, from the answer alone
        b = [class_bytes(x) for x in cls]
        assert nbytes == sum(h * b[r] for h, r in zip(hist, rung))
        if excess:
            assert not any(rung) and excess == sum(hist) * b[0] - avail
        else:
            assert nbytes <= avail
        assert all(rung[i] <= rung[i + 1] for i in range(NBINS - 1) if hist[i] and hist[i + 1])
        live = [i for i in range(NBINS) if hist[i]]
        assert all(rung[i] <= rung[j] for i, j in zip(live, live[1:]))
        assert rung[0] == 0 and all(rung[i] == 0 for i in range(NBINS) if not hist[i] or bin_low(i) < mu)
        if bbin >= 0:   # the next step in the order does not fit
            assert rung[bbin] == brung and nbytes + hist[bbin] * (b[brung + 1] - b[brung]) > avail
        elif not excess:  # nothing was left to take: every eligible bin is at the top
            assert all(rung[i] == len(cls) - 1 for i in live if bin_low(i) >= max(mu, 1))
        seen.add((bool(excess), bbin >= 0, max(rung) if rung else 0))
    return seen


def test_plan_against_model(prog):
    seen = check_plans(prog, plan_cases())
    # over budget, blocked part way, and everything promoted all occur
    assert any(s[0] for s in seen) and any(s[1] for s in seen) and any(not s[0] and not s[1] and s[2] for s in seen)


def test_plan_by_hand(prog):
    """Three bins under {0, signed 3, window 8}: the order of the steps is the
    weights', and the walk stops at the first step that does not fit even where
    a later, smaller one would."""
    cls = [0, S(3), 8]
    b, c = [class_bytes(x) for x in cls], [class_cost(x) for x in cls]
    assert (b, c) == ([64, 256, 270336], [2908, 1540, 320])
    hist = [0] * NBINS
    hist[use_bin(1000)], hist[use_bin(10)], hist[use_bin(1)] = 2, 100, 5
    base = 107 * 64
    # g_0 = 1368 / 192 = 7.1, g_1 = 1220 / 270080 = 0.0045: the three first steps come before any second one
    room = base + 2 * 192 + 100 * 192
    cases = [(hist, cls, room - 1, 0), (hist, cls, room, 0), (hist, cls, room + 5 * 192, 0), (hist, cls, room + 5 * 192, 2),
             (hist, cls, room + 5 * 192 + 2 * 270080, 0)]
    check_plans(prog, cases)
    rungs = [plan_model(*cs)[0] for cs in cases]
    pick = lambda r: (r[use_bin(1000)], r[use_bin(10)], r[use_bin(1)])  # noqa: E731
    assert [pick(r) for r in rungs] == [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 1, 0), (2, 1, 1)]


def test_key_budget_under_sanitizers(prog, tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run as a program over the bins and the plans."""
    exe = str(tmp_path / "key_budget_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    check_bins(exe)
    check_plans(exe, plan_cases())
    assert [int(x) for x in run(exe, ["ladder 0", "ladder 9 " + " ".join(map(str, EIGHT + [12])), "cost 4294967295"])] \
        == [0, 0, 0]
    assert math.log2(class_bytes(29)) < 38   # the 128-bit weights' headroom (key_plan.h)
