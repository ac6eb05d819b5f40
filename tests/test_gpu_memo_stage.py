"""The verified-call memo's two stages, k_memo_probe and k_memo_commit
(minbft_amd/csrc/memo.hip), through the library's launchers on INJECTED items,
slot words, descriptors, device count and a table image the test fabricates
(tests/csrc/memo_check.hip).  No context, no signature: the statuses "the
verifier" gave the compacted items are injected too.

Sizes 1, 63, 64, 65, 1,000 and 70,000: a partial wave, several blocks, more
waves than one atomic's worth.  The hash, bucket and tag are restated here
(as in tests/test_memo_plan.py, which compares them with the header's).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_HOST_SLOT = 0xFFFFFF00
SIZES = [1, 63, 64, 65, 1000, 70000]
ENTRIES = 1 << 16  # per generation: a 16 MiB image
EW = 32  # words an entry
GUARD = 70  # items past n in every array
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def harness(lib):
    from __graft_entry__ import build_memo_check
    h = ctypes.CDLL(build_memo_check())
    vp, cl = ctypes.c_void_p, ctypes.c_long
    h.memo_check_run.argtypes = [vp, vp, vp, vp, vp, cl, cl, cl, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64,
                                 ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    h.memo_check_run.restype = ctypes.c_int
    h.memo_check_probe_steps.restype = ctypes.c_int
    return h


def hashes(words):
    """memo_hash over the rows of an (n, 25) uint32 array."""
    h = np.full(len(words), 0x243F6A8885A308D3, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for k in range(25):
            h ^= words[:, k].astype(np.uint64)
            h *= np.uint64(0x9E3779B97F4A7C15)
            h = (h << np.uint64(27)) | (h >> np.uint64(37))
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def tags(h):
    return ((h >> np.uint64(32)).astype(np.uint32)) | np.uint32(2)


class Case:
    """n items (cap = n + GUARD in every array, the guard filled with a
    pattern), their tuples as 25 words, and who is a real valid key."""

    def __init__(self, n, rng, nslots=50, sprinkle=True):
        self.n, self.cap, self.nslots = n, n + GUARD, nslots
        c = self.cap
        self.e = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        self.r = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        self.s = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        self.slot = rng.integers(0, nslots, c).astype(np.uint32)
        self.valid = np.ones(nslots, dtype=np.uint8)
        if sprinkle:
            q = rng.random(c)
            self.slot[q < 0.05] = nslots + rng.integers(0, 1000, c).astype(np.uint32)[q < 0.05]
            m = (q >= 0.05) & (q < 0.10)
            self.slot[m] = (K_HOST_SLOT + rng.integers(0, 256, c)).astype(np.uint32)[m]
            self.slot[(q >= 0.10) & (q < 0.11)] = nslots
            self.valid[rng.integers(0, nslots, 5)] = 0
        self.forced = None

    def words(self):
        return np.concatenate([self.slot[:, None], self.e.view("<u4"), self.r.view("<u4"), self.s.view("<u4")], axis=1)

    def real(self):
        ok = self.slot < self.nslots
        ok[ok] &= self.valid[self.slot[ok]] != 0
        return ok

    def hash(self):
        return self.forced if self.forced is not None else hashes(self.words())


def empty_image():
    return np.zeros(2 * ENTRIES * EW, dtype=np.uint32)


def place(image, gen, P, h, tag, words25):
    """Write a ready (or, tag 1, busy) entry for the tuple into the first empty
    entry of its probe sequence in generation gen; False if there is none."""
    for j in range(P):
        at = (gen * ENTRIES + ((int(h) + j) & (ENTRIES - 1))) * EW
        if image[at] == 0:
            image[at] = tag
            image[at + 1:at + 26] = words25
            return True
    return False


def run(h, case, image, status, count=-1, probe=True, commit=False, status_c=None, compact=None):
    c = case.cap
    out = {
        "e_c": np.full((c, 32), 0xA5, dtype=np.uint8), "r_c": np.full((c, 32), 0xA6, dtype=np.uint8),
        "s_c": np.full((c, 32), 0xA7, dtype=np.uint8), "slot_c": np.full(c, 0xA8A8A8A8, dtype=np.uint32),
        "origin": np.full(c, 0xA9A9A9A9, dtype=np.uint32), "miss": np.zeros(1, dtype=np.uint32),
        "stats": np.zeros(4, dtype=np.uint64),
    }
    if compact is not None:
        out.update(compact)
    if status_c is None:
        status_c = np.zeros(c, dtype=np.uint8)
    hs = case.hash() if case.forced is not None else None
    p = lambda a: a.ctypes.data  # noqa: E731
    rc = h.memo_check_run(p(case.e), p(case.r), p(case.s), p(case.slot), p(status), case.n, c, count, p(case.valid),
                          case.nslots, p(hs) if hs is not None else None, p(image), ENTRIES, int(probe), int(commit),
                          p(out["e_c"]), p(out["r_c"]), p(out["s_c"]), p(out["slot_c"]), p(out["origin"]),
                          p(out["miss"]), p(status_c), p(out["stats"]))
    assert rc == 0, rc
    out["miss"] = int(out["miss"][0])
    return out


def check_compacted(case, out, want_miss, lim):
    """The compacted set is exactly the expected misses: origin restricted to
    the miss count is a permutation of them, every compacted item is its
    origin's, and nothing past the count was written."""
    m = out["miss"]
    assert m == len(want_miss)
    org = out["origin"][:m].astype(np.int64)
    assert np.array_equal(np.sort(org), np.sort(want_miss))
    assert (org < lim).all()
    assert np.array_equal(out["slot_c"][:m], case.slot[org])
    assert np.array_equal(out["e_c"][:m], case.e[org]) and np.array_equal(out["r_c"][:m], case.r[org])
    assert np.array_equal(out["s_c"][:m], case.s[org])
    assert (out["e_c"][m:] == 0xA5).all() and (out["r_c"][m:] == 0xA6).all() and (out["s_c"][m:] == 0xA7).all()
    assert (out["slot_c"][m:] == 0xA8A8A8A8).all() and (out["origin"][m:] == 0xA9A9A9A9).all()


@pytest.mark.parametrize("with_count", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_probe(harness, n, with_count):
    """Real valid items by class: 0 ready in the young generation, 1 ready in
    the old one (both hit), 2 a busy entry with the whole payload (a miss), 3
    absent (a miss).  Host-decided words, slots >= nslots and invalid slots
    never hit."""
    P = harness.memo_check_probe_steps()
    rng = np.random.default_rng(100 + n)
    case = Case(n, rng)
    w, hh = case.words(), hashes(case.words())
    tg, real = tags(hh), case.real()
    cls = rng.integers(0, 4, case.cap)
    image = empty_image()
    hit = np.zeros(case.cap, dtype=bool)
    # entries for EVERY item up to cap, the guard and the not-real ones too: an
    # item past the count or under no real key must not hit even where an entry waits
    for i in range(case.cap):
        if cls[i] == 3:
            continue
        gen = 1 if cls[i] == 1 else 0
        placed = place(image, gen, P, hh[i], 1 if cls[i] == 2 else tg[i], w[i])
        hit[i] = placed and cls[i] < 2 and real[i]
    before = image.copy()
    count = -1 if not with_count else max(0, n - 1 - n // 3)
    lim = n if count < 0 else count
    status = np.full(case.cap, 0xEE, dtype=np.uint8)
    out = run(harness, case, image, status, count=count)
    want = np.full(case.cap, 0xEE, dtype=np.uint8)
    want[:lim][hit[:lim]] = 0
    assert np.array_equal(status, want)  # hits accepted; misses and everything at or past the count untouched
    check_compacted(case, out, np.nonzero(~hit[:lim])[0], lim)
    assert np.array_equal(image, before)  # a probe writes nothing to the table
    assert list(out["stats"]) == [int(real[:lim].sum()), int(hit[:lim].sum()), 0, 0]
    if n >= 63:
        assert hit[:lim].any() and (~hit[:lim]).any()


def test_probe_one_bit_off_misses(harness):
    """For each of the 25 payload words, an entry that differs from the item
    in one bit of that word (the tag is the item's) misses; the untouched
    twin beside it hits."""
    P = harness.memo_check_probe_steps()
    rng = np.random.default_rng(7)
    bits = [0, 7, 19, 31]
    n = 2 * 25 * len(bits)
    case = Case(n, rng, sprinkle=False)
    w, hh = case.words(), hashes(case.words())
    tg = tags(hh)
    image = empty_image()
    want_hit = np.zeros(n, dtype=bool)
    for i in range(n):
        k, b, twin = (i // 2) % 25, bits[(i // 2) // 25], i % 2 == 1
        ent = w[i].copy()
        if not twin:
            ent[k] ^= np.uint32(1 << b)
        assert place(image, (i // 2) % 2, P, hh[i], tg[i], ent)
        want_hit[i] = twin
    status = np.full(case.cap, 0xEE, dtype=np.uint8)
    out = run(harness, case, image, status)
    assert np.array_equal(status[:n] == 0, want_hit)
    check_compacted(case, out, np.nonzero(~want_hit)[0], n)
    assert list(out["stats"]) == [n, n // 2, 0, 0]


def no_window_full(homes, P):
    """Order-independent and sufficient for no dropped insert: a run of P full
    entries [a, a + P) is filled from homes in [a - P + 1, a + P), so while
    every such span of 2P - 1 buckets holds fewer than P homes no run exists."""
    cnt = np.bincount(homes.astype(np.int64) & (ENTRIES - 1), minlength=ENTRIES)
    ring = np.concatenate([cnt, cnt[:2 * P - 2]])
    cs = np.concatenate([[0], np.cumsum(ring)])
    return int((cs[2 * P - 1:] - cs[:-(2 * P - 1)]).max()) < P


@pytest.mark.parametrize("with_count", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_commit_then_probe(harness, n, with_count):
    """An empty table: every item misses.  The commit scatters the injected
    statuses by origin and inserts only MBFT_ACCEPT items under real valid
    keys; a later probe of the same items hits exactly those."""
    P = harness.memo_check_probe_steps()
    rng = np.random.default_rng(200 + n)
    case = Case(n, rng)
    real, hh = case.real(), hashes(case.words())
    count = -1 if not with_count else max(0, n - 1 - n // 3)
    lim = n if count < 0 else count
    status_c = rng.integers(0, 11, case.cap).astype(np.uint8)
    status_c[rng.random(case.cap) < 0.5] = 0
    image = empty_image()
    status = np.full(case.cap, 0xEE, dtype=np.uint8)
    out = run(harness, case, image, status, count=count, commit=True, status_c=status_c)
    check_compacted(case, out, np.arange(lim), lim)
    org = out["origin"][:lim].astype(np.int64)
    want = np.full(case.cap, 0xEE, dtype=np.uint8)
    want[org] = status_c[:lim]
    assert np.array_equal(status, want)  # scattered by origin, nothing else written
    wanted = np.zeros(case.cap, dtype=bool)
    wanted[org] = (status_c[:lim] == 0) & real[org]
    lookups, hits, inserts, dropped = (int(x) for x in out["stats"])
    assert (lookups, hits) == (int(real[:lim].sum()), 0)
    assert inserts + dropped == int(wanted.sum())
    if no_window_full(hh[wanted], P):
        assert dropped == 0
    # the table: only the young generation written, every written entry ready and some wanted item's tuple
    ent = image.reshape(2 * ENTRIES, EW)
    assert not ent[ENTRIES:].any()
    used = np.nonzero(ent[:ENTRIES, 0])[0]
    assert len(used) == inserts and (ent[used, 0] > 1).all() and not ent[used, 26:].any()
    # the later probe of the same items (all n of them, no count)
    after = image.copy()
    status2 = np.full(case.cap, 0xEE, dtype=np.uint8)
    out2 = run(harness, case, image, status2)
    hit2 = status2[:n] == 0
    assert not (hit2 & ~wanted[:n]).any() and int(hit2.sum()) == inserts
    if dropped == 0:
        assert np.array_equal(hit2, wanted[:n])
    check_compacted(case, out2, np.nonzero(~hit2)[0], n)
    assert np.array_equal(image, after)


def test_forced_collisions(harness):
    """P + 1 distinct tuples on one hash: P inserted, 1 dropped, the counters
    exact; the later probe gives P hits and 1 miss.  Never an overwrite."""
    P = harness.memo_check_probe_steps()
    rng = np.random.default_rng(9)
    n = P + 1
    case = Case(n, rng, sprinkle=False)
    one = 0x1234567800000000 | (ENTRIES - 2)  # one hash for all; its sequence wraps the table's end
    case.forced = np.full(case.cap, one, dtype=np.uint64)
    image = empty_image()
    status = np.full(case.cap, 0xEE, dtype=np.uint8)
    out = run(harness, case, image, status, commit=True)
    assert list(out["stats"]) == [n, 0, P, 1]
    ent = image.reshape(2 * ENTRIES, EW)
    used = np.nonzero(ent[:, 0])[0]
    home = one & (ENTRIES - 1)
    assert sorted(used) == sorted((home + j) & (ENTRIES - 1) for j in range(P))
    w = case.words()
    stored = {tuple(ent[u, 1:26]) for u in used}
    assert len(stored) == P and stored <= {tuple(w[i]) for i in range(n)}
    status2 = np.full(case.cap, 0xEE, dtype=np.uint8)
    out2 = run(harness, case, image, status2)
    assert list(out2["stats"]) == [n, P, 0, 0] and int((status2[:n] == 0).sum()) == P and out2["miss"] == 1
    missed = int(out2["origin"][0])
    assert tuple(w[missed]) not in stored
    # a second commit of the one that was dropped: still no room, nothing overwritten
    before = image.copy()
    status3 = np.full(case.cap, 0xEE, dtype=np.uint8)
    out3 = run(harness, case, image, status3, commit=True)
    assert list(out3["stats"]) == [n, P, 0, 1] and np.array_equal(image, before)


def test_same_tuple_twice_in_one_commit(harness):
    """Afterwards it hits, whichever of the two landed (or both)."""
    rng = np.random.default_rng(10)
    n = 130
    case = Case(n, rng, sprinkle=False)
    for a in (case.e, case.r, case.s):
        a[1::2] = a[0::2][:len(a[1::2])]
    case.slot[1::2] = case.slot[0::2][:len(case.slot[1::2])]
    image = empty_image()
    status = np.full(case.cap, 0xEE, dtype=np.uint8)
    out = run(harness, case, image, status, commit=True)
    assert out["miss"] == n and int(out["stats"][2]) + int(out["stats"][3]) == n and int(out["stats"][3]) == 0
    status2 = np.full(case.cap, 0xEE, dtype=np.uint8)
    out2 = run(harness, case, image, status2)
    assert (status2[:n] == 0).all() and out2["miss"] == 0
