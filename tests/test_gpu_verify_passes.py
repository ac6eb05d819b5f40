"""The verifier kernels' second and later grid-stride passes.

k_verify (under a MBFT_VERIFY_BPC cap), k_verify_slow, k_verify_ladder and
k_verify_keys walk their work in a grid-stride loop over a grid capped by the
CU count; on a 256-CU GPU a second pass starts past 131,072 queued items (the
ladder, the inline keys), past a queue of 128 x sblocks items (the exact path)
or never without the cap (k_verify).  Two routes reach those passes here:

* the harness (tests/csrc/launch_check.hip: verify_check_run,
  verify_keys_check_run) runs mbft_launch::verify's large form and
  mbft_launch::verify_keys on a grid of ONE or THREE blocks -- what
  MBFT_VERIFY_BPC does to the plan -- so a few hundred items stride, whatever
  the CU count, and hands back the statuses, BOTH queues and the guard lines.
  A case states its pass count from the product's grid rules (verify_plan.h,
  through the harness's accessors) before it looks at a result; then every
  status, each queue as a set (nothing lost, nothing twice), each length word
  and every guard;
* the product's own grids through the C-ABI at sizes taken from the same rules
  and the device's CU count (about 262,000 items on 256 CUs): three ladder
  passes per queued class, three inline-key passes, two exact-path passes, and
  a child process under MBFT_VERIFY_BPC=1.

Every expectation is the oracle's: the golden fixtures' verdicts (confirmed
by the C oracle in one batch), crypto/ecdsa.Verify restated (o.go_ecdsa_verify)
for the degenerate rows, and for the exact queue's members a model of the fast
path's comb in big integers (window 8: an item queues where the accumulator
meets +- the entry it is about to add in the key phase).

Degenerate rows (bench.craft_degenerate, key window 8) are taken as they are
(accept) and with e, r and s doubled mod N: u1 and u2 stay, so the addition is
still degenerate and the item still queues, but x(R) no longer matches r -- a
REJECTING queued item (a flipped digest changes u1 and leaves the exact path).

Item i takes vector (a i + b) mod m with gcd(a, m) = 1, so a lane meets another
kind of item in every pass.

Times of the C-ABI cases on an MI355X (256 CUs, n = 262,353 where the size
follows from the CU count), measured once, are in each test's docstring; every
harness case runs in under 0.1 s, the module's vectors (crafting, the oracle's
verdicts, the model's tables) take 2 to 4 s once.
"""
import ctypes
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from golden_util import prehashed_arrays
from test_gpu_inline_keys import crafted  # noqa: F401  (its bad points)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPT, REJECT, BAD_KEY = 0, 1, 5
UNTOUCHED = 0xEEEEEEEE
W8, TFREE, TEETH4, STEETH5 = 8, 0, 0x100 | 4, 0x200 | 5
QUEUED = (TFREE, TEETH4, STEETH5)
WG = 8               # generator window
D_KEY = 0x5EED0F     # the key of the degenerate and zero-window rows
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


# --------------------------------------------------- the fast path's comb, modelled
def _jdbl(p):
    X, Y, Z = p
    ZZ = Z * Z % P
    M = 3 * (X - ZZ) * (X + ZZ) % P
    YY = Y * Y % P
    S = 4 * X * YY % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - 8 * YY * YY) % P, 2 * Y * Z % P


def _jadd(p, q):
    """p + q in Jacobian coordinates; None where x(p) == x(q), q = +-p: the
    addition the unchecked mixed addition cannot do."""
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    A, B = Z1 * Z1 % P, Z2 * Z2 % P
    U1, U2 = X1 * B % P, X2 * A % P
    H = (U2 - U1) % P
    if H == 0:
        return None
    S1, S2 = Y1 * Z2 * B % P, Y2 * Z1 * A % P
    R = (S2 - S1) % P
    HH = H * H % P
    HHH, V = H * HH % P, U1 * HH % P
    X3 = (R * R - HHH - 2 * V) % P
    return X3, (R * (V - X3) - S1 * HHH) % P, H * Z1 * Z2 % P


def _comb_table(q):
    """tab[j][k] = k 2^(8 j) q, k = 1 .. 128 (256 in the last window)."""
    tab, base = [], (q[0], q[1], 1)
    for j in range(32):
        row = [None, base, _jdbl(base)]
        while len(row) <= (256 if j == 31 else 128):
            row.append(_jadd(row[-1], base))
        tab.append(row)
        for _ in range(8):
            base = _jdbl(base)
    return tab


def _entry(tab, j, d):
    X, Y, Z = tab[j][abs(d)]
    return (X, -Y % P, Z) if d < 0 else (X, Y, Z)


def _queues_exact(digits, tab_g, tab_q, u1, u2):
    """k_verify's comb_verify_fast at windows 8 / 8: u1 G over the signed
    digits (zero digits skipped, never degenerate), then u2 Q's entries one by
    one: the item takes the exact path where the accumulator equals +- the
    entry to add (the mixed addition leaves ZZ == 0 for good)."""
    acc = None
    for j, d in enumerate(digits(u1, 8)):
        if d:
            acc = _entry(tab_g, j, d) if acc is None else _jadd(acc, _entry(tab_g, j, d))
            assert acc is not None
    for j, d in enumerate(digits(u2, 8)):
        if d:
            nxt = _entry(tab_q, j, d) if acc is None else _jadd(acc, _entry(tab_q, j, d))
            if nxt is None:
                return True
            acc = nxt
    return False


# ------------------------------------------------------------------ the vectors
def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)


def _int(a):
    return int.from_bytes(bytes(a), "big")


class Vectors:
    """Every vector the cases draw from, in one table: xy (64 B big-endian),
    e, r, s; exp: the status under a valid key; in_range: r, s in [1, N);
    degen8: the item takes the exact path under a window-8 key (None: not
    modelled, never put under one); sets: name -> row indices."""


@pytest.fixture(scope="module")
def vec(lib):
    from oracle import c_oracle
    from oracle import p256 as o
    bench = _bench()
    v = Vectors()
    parts, v.sets, at = [], {}, 0
    for name, fname in (("prehashed", "prehashed.json"), ("ladder", "ladder_edges.json"),
                        ("teeth", "teeth_edges.json"), ("steeth", "steeth_edges.json")):
        xy, e, r, s, exp, _ = prehashed_arrays(fname)
        parts.append((xy, e, r, s, np.where(exp == 1, ACCEPT, REJECT).astype(np.uint8)))
        v.sets[name] = np.arange(at, at + len(exp))
        at += len(exp)
    # the degenerate rows under one key at window 8: as they are, and doubled
    q = o.pubkey(D_KEY)
    qxy = np.concatenate([_b32(q[0]), _b32(q[1])])
    rows = bench.craft_degenerate(D_KEY, 8, 48, 0xDE8)
    rows = [(e_, r_, s_, True) for e_, r_, s_ in rows] + \
           [(2 * e_ % N, 2 * r_ % N, 2 * s_ % N, False) for e_, r_, s_ in rows]
    for e_, r_, s_, want in rows:
        assert o.go_ecdsa_verify(q, e_.to_bytes(32, "big"), r_, s_) == want
    # zero key windows: u2 = v 2^8 (the first window), or with window 3 zero too
    import random
    rng = random.Random(0x2E80)
    zrows = []
    for j in range(12):
        k = rng.randrange(1, N)
        u2 = rng.randrange(1, N >> 8) << 8
        if j % 2:
            u2 &= ~(0xFF << 24)
        rr = o.scalar_mult(k, o.G)[0] % N
        iu = pow(u2, -1, N)
        zrows.append((rr * ((k * iu - D_KEY) % N) % N, rr, rr * iu % N, True))
    own = rows + zrows
    parts.append((np.tile(qxy, (len(own), 1)), np.stack([_b32(x[0]) for x in own]),
                  np.stack([_b32(x[1]) for x in own]), np.stack([_b32(x[2]) for x in own]),
                  np.array([ACCEPT if x[3] else REJECT for x in own], dtype=np.uint8)))
    v.sets["degen"] = np.arange(at, at + len(rows))
    v.sets["zerowin"] = np.arange(at + len(rows), at + len(own))
    v.xy, v.e, v.r, v.s, v.exp = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(5))
    m = len(v.exp)
    rs = [(_int(v.r[i]), _int(v.s[i])) for i in range(m)]
    v.in_range = np.array([0 < r_ < N and 0 < s_ < N for r_, s_ in rs])
    # one batch through the C oracle: every verdict above
    got = c_oracle.verify_prehashed_batch(v.xy, v.e, v.r, v.s, np.arange(m, dtype=np.uint32), nthreads=8)
    assert (got == v.exp).all(), np.nonzero(got != v.exp)[0][:10]
    assert (v.exp[~v.in_range] == REJECT).all() and 5 <= (~v.in_range).sum()
    # the exact queue's members under window-8 keys, by the model
    tabs = {}

    def table(key):
        if key not in tabs:
            tabs[key] = _comb_table((_int(key[:32]), _int(key[32:])))
        return tabs[key]

    tab_g = _comb_table(o.G)
    v.degen8 = np.zeros(m, dtype=bool)
    v.modelled = np.zeros(m, dtype=bool)
    for name in ("prehashed", "ladder", "degen", "zerowin"):
        for i in v.sets[name]:
            v.modelled[i] = True
            if v.in_range[i]:
                w = pow(rs[i][1], -1, N)
                v.degen8[i] = _queues_exact(bench.signed_digits, tab_g, table(bytes(v.xy[i])),
                                            _int(v.e[i]) * w % N, rs[i][0] * w % N)
    assert v.degen8[v.sets["degen"]].all()          # both halves still queue
    assert not v.degen8[v.sets["zerowin"]].any()    # a zero digit is the fast path's own
    assert (v.exp[v.sets["degen"]] == ACCEPT).sum() == 48 == (v.exp[v.sets["degen"]] == REJECT).sum()
    # ordinary window-8 items: golden vectors, in range or not, that stay on the fast path
    plain = np.concatenate([v.sets["prehashed"], v.sets["ladder"]])
    v.sets["plain8"] = plain[~v.degen8[plain]]
    v.sets["golden8"] = plain
    v.sets["out_of_range"] = plain[~v.in_range[plain]]
    return v


# ------------------------------------------------------------------ the harness
@pytest.fixture(scope="module")
def harness(lib):
    path = os.path.join(ROOT, "tests", "liblaunch_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_launch_check
        build_launch_check()
    h = ctypes.CDLL(path)
    vp, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    h.verify_check_run.argtypes = [vp, vp, vp, I, vp, vp, vp, vp, L, I, L, vp, vp, vp, vp, vp]
    h.verify_check_run.restype = I
    h.verify_keys_check_run.argtypes = [vp, vp, vp, vp, L, I, L, I, vp, vp]
    h.verify_keys_check_run.restype = I
    for f, nargs in ((h.verify_check_device_cus, 0), (h.verify_check_large_blocks, 3),
                     (h.verify_check_slow_blocks, 3), (h.verify_check_ladder_blocks, 2)):
        f.argtypes = [L] * nargs
        f.restype = L
    h.verify_check_keys_blocks.argtypes = [L, ctypes.c_ulong, L]
    h.verify_check_keys_blocks.restype = L
    return h


@pytest.fixture(scope="module")
def ncu(harness):
    n = harness.verify_check_device_cus()
    assert n >= 1
    return n


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _le_words(xy_be):
    """64 B big-endian X || Y -> 16 little-endian words (plain affine x, y)."""
    return np.ascontiguousarray(np.concatenate([xy_be[:, 31::-1], xy_be[:, :31:-1]], axis=1)).view(np.uint32)


class Batch:
    """Items for verify_check_run: vi the vector of each, cls its key's class,
    bad 0 (a valid slot), 1 (a slot whose key is invalid) or 2 (a slot past the
    last).  A key slot per distinct (point, class, invalid)."""

    def __init__(self, vec, vi, cls, bad=None):
        self.vec, self.vi = vec, np.asarray(vi, dtype=np.int64)
        self.cls = np.asarray(cls, dtype=np.uint32)
        self.bad = np.zeros(len(self.vi), dtype=np.int64) if bad is None else np.asarray(bad, dtype=np.int64)
        assert len(self.vi) == len(self.cls) == len(self.bad)
        w8 = self.cls == W8
        assert vec.modelled[self.vi[w8]].all()

    def expect(self):
        v, ok = self.vec, self.bad == 0
        rng = v.in_range[self.vi]
        status = np.where(~ok, BAD_KEY, np.where(rng, v.exp[self.vi], REJECT)).astype(np.uint8)
        ladder = np.nonzero(ok & rng & np.isin(self.cls, QUEUED))[0]
        exact = np.nonzero(ok & rng & (self.cls == W8) & v.degen8[self.vi])[0]
        return status, exact, ladder

    def run(self, h, grid_blocks):
        v, n = self.vec, len(self.vi)
        keys, slot = {}, np.zeros(n, dtype=np.uint32)
        for i in range(n):
            k = (bytes(v.xy[self.vi[i]]), int(self.cls[i]), int(self.bad[i] == 1))
            slot[i] = keys.setdefault(k, len(keys))
        slot[self.bad == 2] = len(keys) + 7
        kxy = _le_words(np.stack([np.frombuffer(k[0], dtype=np.uint8) for k in keys]))
        kcls = np.array([k[1] for k in keys], dtype=np.uint32)
        kinv = np.array([k[2] for k in keys], dtype=np.uint8)
        e, r, s = (np.ascontiguousarray(a[self.vi]) for a in (v.e, v.r, v.s))
        st = np.zeros(n, dtype=np.uint8)
        qlen = np.zeros(2, dtype=np.uint32)
        sq, lq = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        guards = ctypes.c_int(-1)
        rc = h.verify_check_run(_ptr(kxy), _ptr(kcls), _ptr(kinv), len(keys), _ptr(e), _ptr(r), _ptr(s), _ptr(slot),
                                n, WG, grid_blocks, _ptr(st), _ptr(qlen), _ptr(sq), _ptr(lq), ctypes.byref(guards))
        assert rc == 0, rc
        return st, qlen, sq, lq, guards.value, bool(np.isin(kcls, QUEUED).any())

    def check(self, h, grid_blocks, what=""):
        """Statuses, both queues as sets, both length words, every guard."""
        want, exact, ladder = self.expect()
        st, qlen, sq, lq, guards, table_free = self.run(h, grid_blocks)
        n = len(want)
        bad = np.nonzero(st != want)[0]
        assert not len(bad), (what, len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]])
        for name, length, queue, members in (("exact", int(qlen[0]), sq, exact), ("ladder", int(qlen[1]), lq, ladder)):
            if name == "ladder" and not table_free:
                # no key of a queued class: no reset, no kernel, the word is nobody's
                assert length == UNTOUCHED and not len(members), (what, name, length)
                length = 0
            assert length == len(members), (what, name, length, len(members))
            got = queue[:length]
            assert len(np.unique(got)) == length, (what, name, "an index twice")
            assert set(got.tolist()) == set(members.tolist()), (what, name)
            assert (queue[length:] == UNTOUCHED).all(), (what, name, "a word past the length")
        assert guards == 15, (what, "guards", guards)
        return st


def _walk(idx, count, b=0):
    """idx[(a i + b) mod m] for i < count: a the smallest of a few primes with
    gcd(a, m) = 1, so consecutive passes of a lane meet different vectors."""
    m = len(idx)
    a = next(a for a in (7, 11, 13, 17, 19, 23) if math.gcd(a, m) == 1)
    return idx[(a * np.arange(count) + b) % m]


def _passes(items, per_pass):
    return -(-items // per_pass)


def _harness_grids(h, ncu, B):
    """The grids mbft_launch::verify launches for a plan of B blocks, no cap."""
    v = h.verify_check_large_blocks(B, 0, ncu)
    return v, h.verify_check_slow_blocks(B, v, ncu), h.verify_check_ladder_blocks(B, ncu)


BS = (1, 3)


# -------------------------------------------------------------------- k_verify
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", ["exact", "+1", "+64", "2x+65", "4x+77"])
def test_k_verify_passes(harness, ncu, vec, B, shape):
    """Golden vectors (every kind: crafted joins, comb collisions, range edges,
    zero windows) under window-8 keys on a grid of B blocks: one pass exactly,
    a second pass of one lane, of one wave, a ragged third, a ragged fifth."""
    vb, _, _ = _harness_grids(harness, ncu, B)
    assert vb == B
    n, want = {"exact": (256 * B, 1), "+1": (256 * B + 1, 2), "+64": (256 * B + 64, 2),
               "2x+65": (2 * 256 * B + 65, 3), "4x+77": (4 * 256 * B + 77, 5)}[shape]
    assert _passes(n, 256 * vb) == want
    pool = np.concatenate([vec.sets["golden8"], vec.sets["zerowin"]])
    b = Batch(vec, _walk(pool, n, 3), np.full(n, W8))
    st = b.check(harness, B, shape)
    if n > 600:
        assert (st == ACCEPT).sum() > 100 and (st == REJECT).sum() > 100


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", ["dead_pass", "one_wave"])
def test_k_verify_dead_passes(harness, ncu, vec, B, shape):
    """The whole second pass dead (r or s out of range, invalid slots, slots
    past the last) and the third live: every wave returns from verify_one
    early and must take part again.  Or one wave of the second pass alone
    holds live lanes (three, the first not lane 0: the dead lanes adopt its
    table) and every other wave of that pass is dead."""
    vb, _, _ = _harness_grids(harness, ncu, B)
    per = 256 * vb
    n = 3 * per if shape == "dead_pass" else 2 * per + 65
    assert _passes(n, per) == 3
    vi = _walk(vec.sets["golden8"], n, 5)
    bad = np.zeros(n, dtype=np.int64)
    second = np.arange(per, 2 * per)
    live = np.zeros(0, dtype=np.int64)
    if shape == "one_wave":
        wave0 = per + 64 * (2 * B - 1)  # a wave in the middle of the pass
        live = wave0 + np.array([5, 6, 40])
    dead = np.setdiff1d(second, live)
    oor = vec.sets["out_of_range"]
    kinds = np.arange(len(dead)) % 3
    vi[dead[kinds == 0]] = oor[np.arange((kinds == 0).sum()) % len(oor)]
    bad[dead[kinds == 1]] = 1
    bad[dead[kinds == 2]] = 2
    # the live lanes: fast-path accepts
    acc = vec.sets["plain8"][(vec.exp[vec.sets["plain8"]] == ACCEPT)]
    vi[live] = acc[: len(live)]
    b = Batch(vec, vi, np.full(n, W8), bad)
    want, exact, _ = b.expect()
    assert (want[dead] != ACCEPT).all() and (want[live] == ACCEPT).all()
    assert not np.isin(exact, dead).any()
    b.check(harness, B, shape)


# ------------------------------------------------------------- the exact queue
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", ["one", "+1", "+2", "3x+63"])
def test_exact_queue_passes(harness, ncu, vec, B, shape):
    """nq degenerate items (accepting and rejecting) among ordinary ones:
    k_verify_slow serves a lane PAIR an item, so a pass holds 128 x sblocks;
    +1 leaves a second pass with one live pair, whose wave-mates are dead
    lanes reading slowq[0]."""
    vb, sb, _ = _harness_grids(harness, ncu, B)
    assert sb == B and sb <= vb
    per = 128 * sb
    nq, want = {"one": (per, 1), "+1": (per + 1, 2), "+2": (per + 2, 2), "3x+63": (3 * per + 63, 4)}[shape]
    assert _passes(2 * nq, 256 * sb) == want
    n = 2 * nq + 37
    rng = np.random.Generator(np.random.PCG64(nq))
    pos = np.sort(rng.choice(n, size=nq, replace=False))
    vi = _walk(vec.sets["plain8"], n, 1)
    vi[pos] = _walk(vec.sets["degen"], nq, 2)
    b = Batch(vec, vi, np.full(n, W8))
    _, exact, _ = b.expect()
    assert (exact == pos).all()
    st = b.check(harness, B, shape)
    assert (st[pos] == ACCEPT).sum() >= nq // 3 and (st[pos] == REJECT).sum() >= nq // 3


def test_zero_window_items_stay_on_the_fast_path(harness, vec):
    """Items whose u2 has zero key windows (u2 = v 2^8) are NOT queued:
    comb_step resolves a zero digit in the fast path (the spill planes)."""
    n = 256 * 2 + 40
    b = Batch(vec, _walk(vec.sets["zerowin"], n), np.full(n, W8))
    st, qlen, _, _, guards, _ = b.run(harness, 1)
    assert (st == ACCEPT).all() and int(qlen[0]) == 0 and guards == 15
    b.check(harness, 1)


# ------------------------------------------------------------ the ladder queue
CLASS_SET = {TFREE: "ladder", TEETH4: "teeth", STEETH5: "steeth"}


def _ladder_batch(vec, cls, mix, L):
    """Items until exactly L of them are queued for the ladder."""
    others = [c for c in QUEUED if c != cls]
    cycle = {"all": [cls], "half": [cls, W8],
             "all3": [cls, W8, others[0], "degen", others[1], cls, W8, cls]}[mix]
    pools = {c: np.concatenate([vec.sets[CLASS_SET[c]], vec.sets["prehashed"]]) for c in QUEUED}
    pools[W8] = vec.sets["golden8"]
    pools["degen"] = vec.sets["degen"]
    vi, kc, queued, i = [], [], 0, 0
    while queued < L:
        c = cycle[i % len(cycle)]
        pool = pools[c]
        j = int(_walk(pool, i + 1, 2)[i])
        c = W8 if c == "degen" else c
        vi.append(j)
        kc.append(c)
        queued += int(c in QUEUED and vec.in_range[j])
        i += 1
    return Batch(vec, vi, kc)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", ["one", "+1", "+64", "3x+17"])
@pytest.mark.parametrize("mix", ["all", "half", "all3"])
@pytest.mark.parametrize("cls", QUEUED, ids=["tfree", "teeth4", "steeth5"])
def test_ladder_queue_passes(harness, ncu, vec, cls, mix, shape, B):
    """The ladder queue at one pass exactly, plus a lane, plus a wave, and at
    three passes and 17: every key of one queued class; that class interleaved
    with window-8 keys; all three queued classes, window-8 keys and degenerate
    items in one batch (both queues at once)."""
    vb, sb, lb = _harness_grids(harness, ncu, B)
    assert lb == B
    per = 256 * lb
    L, want = {"one": (per, 1), "+1": (per + 1, 2), "+64": (per + 64, 2), "3x+17": (3 * per + 17, 4)}[shape]
    assert _passes(L, per) == want
    b = _ladder_batch(vec, cls, mix, L)
    _, exact, ladder = b.expect()
    assert len(ladder) == L
    if mix == "all3":
        assert len(exact) >= L // 10 and set(b.cls[ladder].tolist()) == set(QUEUED)
    b.check(harness, B, (cls, mix, shape))


# ----------------------------------------------------------------- inline keys
def _keys_items(vec, bad_points, n, per_pass):
    """Lane j of pass p has kind (j + p) mod 3: a valid key, a bad point, r or s
    out of range -- a lane that leaves the loop body early (`continue`) in one
    pass runs the ladder in the next."""
    i = np.arange(n)
    kind = (i % per_pass + i // per_pass) % 3
    good = np.concatenate([vec.sets["prehashed"], vec.sets["ladder"]])
    good = good[vec.in_range[good]]
    oor = vec.sets["out_of_range"]
    vi = _walk(good, n, 1)
    vi[kind == 2] = oor[np.arange((kind == 2).sum()) % len(oor)]
    xy = vec.xy[vi].copy()
    k1 = np.nonzero(kind == 1)[0]
    for t, j in enumerate(k1):
        x, y = bad_points[t % len(bad_points)]
        xy[j] = np.concatenate([_b32(x), _b32(y)])
    want = np.where(kind == 1, BAD_KEY, np.where(kind == 2, REJECT, vec.exp[vi])).astype(np.uint8)
    return xy, vec.e[vi].copy(), vec.r[vi].copy(), vec.s[vi].copy(), want


@pytest.mark.parametrize("lane_inv", [0, 1], ids=["planes", "lane_inv"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", ["exact", "+1", "+64", "2x+65", "4x+77"])
def test_inline_keys_passes(harness, vec, crafted, B, shape, lane_inv):  # noqa: F811
    n, want_passes = {"exact": (256 * B, 1), "+1": (256 * B + 1, 2), "+64": (256 * B + 64, 2),
                      "2x+65": (2 * 256 * B + 65, 3), "4x+77": (4 * 256 * B + 77, 5)}[shape]
    assert _passes(n, 256 * B) == want_passes
    xy, e, r, s, want = _keys_items(vec, crafted[5], n, 256 * B)
    assert {ACCEPT, REJECT, BAD_KEY} == set(want.tolist())
    st = np.zeros(n, dtype=np.uint8)
    guard = ctypes.c_int(-1)
    rc = harness.verify_keys_check_run(_ptr(e), _ptr(r), _ptr(s), _ptr(xy), n, WG, B, lane_inv, _ptr(st),
                                       ctypes.byref(guard))
    assert rc == 0, rc
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]])
    assert guard.value == 1


# ------------------------------------------- the product's grids through the C-ABI
def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _device_arrays(*arrays):
    torch, dev = _torch_dev()
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _poisoned_status(n):
    torch, dev = _torch_dev()
    return torch.full((n + 256,), 0xEE, dtype=torch.uint8, device=dev)


def _status(d_st, n):
    out = d_st.cpu().numpy()
    assert (out[n:] == 0xEE).all()
    return out[:n]


def _same(st, want, what):
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (what, len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]])


def _select_class(a, cls):
    if cls == TFREE:
        a.set_key_window(0)
    elif cls == TEETH4:
        a.set_key_teeth(4)
    elif cls == STEETH5:
        a.set_key_signed_teeth(5)
    else:
        a.set_key_window(cls)


def _register(a, vec, vi, cls):
    """One slot per distinct point of the vectors vi under class cls; the slot of each."""
    keys = {}
    which = np.array([keys.setdefault(bytes(vec.xy[j]), len(keys)) for j in vi])
    _select_class(a, cls)
    slots, valid = a.register_points(np.stack([np.frombuffer(k, dtype=np.uint8) for k in keys]))
    assert valid.all()
    return slots[which].astype(np.uint32)


@pytest.mark.parametrize("cls", QUEUED, ids=["tfree", "teeth4", "steeth5"])
def test_product_ladder_three_passes(lib, harness, ncu, vec, cls):
    """n = 2 cap + 3 x 64 + 17 items, every one queued (in range, a valid key
    of the class): k_verify_ladder's grid of 2 blocks per CU runs three passes,
    the last ragged.  Twice back to back without a synchronize: the queue's
    counter is reset per batch.
    Measured (both batches, on the stream): table-free 25 ms, compact 5 ms,
    signed compact 5 ms; the whole test with upload and registration 0.26 s,
    0.10 s and 0.09 s."""
    from minbft_amd.authenticator import Authenticator
    torch, _ = _torch_dev()
    blocks_of = lambda n: (n + 255) // 256  # noqa: E731
    cap = 256 * harness.verify_check_ladder_blocks(1 << 30, ncu)
    assert cap == 512 * ncu
    n = 2 * cap + 3 * 64 + 17
    assert n > 4096  # the large form
    assert _passes(n, 256 * harness.verify_check_ladder_blocks(blocks_of(n), ncu)) == 3
    pool = np.concatenate([vec.sets[CLASS_SET[cls]], vec.sets["prehashed"]])
    pool = pool[vec.in_range[pool]]
    vi = _walk(pool, n, 4)
    want = vec.exp[vi]
    assert (want == ACCEPT).sum() > n // 4 and (want == REJECT).sum() > n // 4
    with Authenticator(0) as a:
        slots = _register(a, vec, vi, cls)
        d_e, d_r, d_s, d_sl = _device_arrays(vec.e[vi], vec.r[vi], vec.s[vi], slots)
        outs = [_poisoned_status(n) for _ in range(2)]
        stream = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d_st in outs:  # (no synchronize inside this loop)
            a.verify_prehashed_device(d_e.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_sl.data_ptr(), n,
                                      d_st.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        torch.cuda.synchronize()
        print("ladder class %#x: n = %d, 3 passes, two batches in %.3f s" % (cls, n, time.perf_counter() - t0))
        for k, d_st in enumerate(outs):
            _same(_status(d_st, n), want, (cls, "batch %d" % k))


def test_product_inline_keys_three_passes(lib, harness, ncu, vec, crafted):  # noqa: F811
    """n = 2 cap + 209 through mbft_verify_prehashed_keys_device: k_verify_keys
    <false> (s^-1 from the planes) on its capped grid, three passes, valid,
    bad-key and out-of-range lanes rotating from pass to pass.
    Measured: 12 ms on the stream, the whole test 0.16 s."""
    from minbft_amd.authenticator import Authenticator
    torch, _ = _torch_dev()
    cap_blocks = harness.verify_check_keys_blocks(1 << 30, 4096, ncu)
    assert cap_blocks == 2 * ncu
    n = 2 * 256 * cap_blocks + 209
    assert n > 4096 and harness.verify_check_keys_blocks(n, 4096, ncu) == cap_blocks
    assert _passes(n, 256 * cap_blocks) == 3
    xy, e, r, s, want = _keys_items(vec, crafted[5], n, 256 * cap_blocks)
    with Authenticator(0) as a:
        d_e, d_r, d_s, d_xy = _device_arrays(e, r, s, xy)
        d_st = _poisoned_status(n)
        stream = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.verify_prehashed_keys_device(d_e.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_xy.data_ptr(), n,
                                       d_st.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        torch.cuda.synchronize()
        print("inline keys: n = %d, 3 passes, %.3f s" % (n, time.perf_counter() - t0))
        _same(_status(d_st, n), want, "inline")


def test_product_exact_queue_two_passes(lib, harness, ncu, vec):
    """8,192 degenerate items and nothing else: 32 blocks, so k_verify_slow's
    grid is 32 blocks (128 x 32 = 4,096 items a pass) and the queue takes two.
    Measured: both batches, host buffers in and out, 2 ms; the whole test 0.04 s."""
    from minbft_amd.authenticator import Authenticator
    n = 8192
    blocks = n // 256
    sb = harness.verify_check_slow_blocks(blocks, harness.verify_check_large_blocks(blocks, 0, ncu), ncu)
    assert sb == min(32, 4 * ncu)
    assert _passes(2 * n, 256 * sb) >= 2
    vi = _walk(vec.sets["degen"], n, 1)
    want = vec.exp[vi]
    with Authenticator(0) as a:
        slots = _register(a, vec, vi, W8)
        t0 = time.perf_counter()
        for k in range(2):  # (the queue's buffers reused)
            _same(a.verify_prehashed(vec.e[vi], vec.r[vi], vec.s[vi], slots), want, "batch %d" % k)
        print("exact queue: n = %d, two batches in %.3f s" % (n, time.perf_counter() - t0))


CAPPED_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.init()
from minbft_amd.authenticator import Authenticator
d = np.load(sys.argv[2])
with Authenticator(0) as a:
    a.set_key_window(8)
    s8, v8 = a.register_points(d["xy8"])
    a.set_key_window(0)
    s0, v0 = a.register_points(d["xy0"])
    assert v8.all() and v0.all()
    slots = np.where(d["tfree"], s0[d["which"]], s8[d["which"]]).astype(np.uint32)
    st = a.verify_prehashed(d["e"], d["r"], d["s"], slots)
np.save(sys.argv[3], st)
print("capped verify ok")
"""


def test_product_capped_grid_child(lib, harness, ncu, vec, tmp_path):
    """MBFT_VERIFY_BPC=1 (read once per process: a fresh child, as
    MBFT_SPLIT_WIDE in test_gpu_scalar_edges): n = 2 x 256 ncu + 300 items of
    window-8 keys, table-free keys and degenerate items.  k_verify's grid is
    ncu blocks (three passes), k_verify_slow's is clamped to it, the ladder's
    2 ncu blocks are more than it.  The child's statuses are the expectation
    and the uncapped parent's.
    Measured: 2.0 to 2.3 s, nearly all of it the child's start (n = 131,372)."""
    from minbft_amd.authenticator import Authenticator
    n = 2 * 256 * ncu + 300
    blocks = (n + 255) // 256
    vb = harness.verify_check_large_blocks(blocks, 1, ncu)
    assert vb == ncu and _passes(n, 256 * vb) == 3
    assert harness.verify_check_slow_blocks(blocks, vb, ncu) == vb < min(blocks, 4 * ncu)
    assert harness.verify_check_ladder_blocks(blocks, ncu) == 2 * ncu
    assert n > 4096
    i = np.arange(n)
    kind = i % 4  # 0, 1: window 8; 2: table-free; 3: degenerate (window 8)
    vi = _walk(vec.sets["golden8"], n, 6)
    lad = np.concatenate([vec.sets["ladder"], vec.sets["prehashed"]])
    vi[kind == 2] = _walk(lad, int((kind == 2).sum()), 1)
    vi[kind == 3] = _walk(vec.sets["degen"], int((kind == 3).sum()), 3)
    tfree = kind == 2
    want = np.where(vec.in_range[vi], vec.exp[vi], REJECT).astype(np.uint8)
    keys = {}
    which = np.array([keys.setdefault(bytes(vec.xy[j]), len(keys)) for j in vi])
    kxy = np.stack([np.frombuffer(k, dtype=np.uint8) for k in keys])
    with Authenticator(0) as a:
        a.set_key_window(8)
        s8, v8 = a.register_points(kxy)
        a.set_key_window(0)
        s0, v0 = a.register_points(kxy)
        assert v8.all() and v0.all()
        slots = np.where(tfree, s0[which], s8[which]).astype(np.uint32)
        parent = a.verify_prehashed(vec.e[vi], vec.r[vi], vec.s[vi], slots)
    _same(parent, want, "uncapped")
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npy")
    np.savez(inp, xy8=kxy, xy0=kxy, which=which, tfree=tfree, e=vec.e[vi], r=vec.r[vi], s=vec.s[vi])
    env = dict(os.environ, MBFT_VERIFY_BPC="1")
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-c", CAPPED_SCRIPT, ROOT, inp, outp],
                       env=env, capture_output=True, text=True)
    print("capped child: n = %d, %.1f s" % (n, time.perf_counter() - t0))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "capped verify ok" in p.stdout
    child = np.load(outp)
    _same(child, want, "capped")
    _same(child, parent, "capped vs uncapped")
