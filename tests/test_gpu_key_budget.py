"""The key memory budget through the C-ABI (include/minbft_gpu.h, DESIGN.md
§4.11): mbft_rebalance_keys against the Python plan of test_key_budget.py
computed from mbft_key_usage's counts, a fixed accept / reject mix read the
same before and after every rebalance, ageing and demotion with reuse of the
released storage, the over-budget plan, the error statuses, mbft_cold_keys,
and two engines on the one GPU.

About 200 client keys, key k the point (k + 2) G with the private key k + 2, so
that batches come from mbft_sign_prehashed; the generator at its default
window; the ladder {table-free, signed 3, signed 6, window 8}, one key pinned
at window 12.
"""
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays
from test_key_budget import NBINS, S, class_bytes, plan_model, use_bin

pytestmark = pytest.mark.gpu

ACCEPT, REJECT = 0, 1
ROLE_CLIENT = 3
LADDER = [0, S(3), S(6), 8]
PIN = 12
GOLD0 = 1000   # ids of the golden vectors' keys


def _chain(count, start=2):
    from oracle import p256 as o
    pts, p = [], o.scalar_mult(start, o.G)
    for _ in range(count):
        pts.append(p)
        p = o.point_add(p, o.G)
    return pts


def _xy(q):
    return q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


@pytest.fixture(scope="module")
def points():
    return _chain(200)


def _register(a, pts):
    a.add_role(ROLE_CLIENT)
    a.set_key_window(0)
    for k, q in enumerate(pts):
        a.set_public_key(ROLE_CLIENT, k, _xy(q))
    return np.array([a.key_slot(ROLE_CLIENT, k) for k in range(len(pts))], dtype=np.uint32)


def _load(a, slot_of, counts, seed):
    """counts[k] signatures of key k (private key k + 2) made by
    mbft_sign_prehashed and verified in one batch: all accepted."""
    key = np.repeat(np.arange(len(counts)), counts).astype(np.uint32)
    np.random.default_rng(seed).shuffle(key)
    priv = np.array([list((k + 2).to_bytes(32, "big")) for k in range(len(counts))], dtype=np.uint8)
    e = np.random.default_rng(seed + 1).integers(0, 256, size=(len(key), 32), dtype=np.uint8)
    r, s = a.sign_prehashed(priv, e, key)
    st = a.verify_prehashed(e, r, s, slot_of[key])
    assert (st == ACCEPT).all()
    return e, r, s, slot_of[key]


def _skewed(nk):
    c = np.zeros(nk, dtype=np.int64)
    c[0], c[1], c[2], c[3] = 3000, 2900, 1500, 800
    c[4:12], c[12:41], c[41:101] = 200, 30, 3
    return c


class Mix:
    """A fixed accept / reject mix: golden prehashed vectors under keys of
    their own (ids from GOLD0), copies of them tampered, and signed REQUESTs of
    three chain keys with tampered ones among them."""

    def __init__(self, a):
        from test_gpu_key_lifecycle import _call, _request
        xy, e, r, s, exp, labels = prehashed_arrays()
        pick = np.arange(0, len(labels), 6)
        xy, e, r, s, exp = xy[pick], e[pick], r[pick], s[pick], exp[pick]
        keys, inv = np.unique(xy, axis=0, return_inverse=True)
        for k, q in enumerate(keys):
            a.set_public_key(ROLE_CLIENT, GOLD0 + k, bytes(q))
        self.gold_ids = [GOLD0 + k for k in range(len(keys))]
        slots = np.array([a.key_slot(ROLE_CLIENT, i) for i in self.gold_ids], dtype=np.uint32)[inv.reshape(-1)]
        te = e.copy()
        te[:, 31] ^= 1
        self.e, self.r, self.s = np.concatenate([e, te]), np.concatenate([r, r]), np.concatenate([s, s])
        self.slots = np.concatenate([slots, slots])
        # (a vector that is a tampered one itself comes right again: the oracle says what the copies read)
        from oracle import p256 as o
        tam = [o.go_ecdsa_verify((int.from_bytes(q[:32], "big"), int.from_bytes(q[32:], "big")), bytes(te[j]),
                                 int.from_bytes(r[j], "big"), int.from_bytes(s[j], "big"))
               for j, q in enumerate(bytes(x) for x in xy)]
        self.want = np.concatenate([np.where(exp == 1, ACCEPT, REJECT), np.where(tam, ACCEPT, REJECT)])
        assert (self.want == ACCEPT).sum() >= 20 and (self.want == REJECT).sum() >= len(exp)
        msgs = [_request(2 + (j % 3) * 50, (j % 3) * 50, j, tamper=(j % 4 == 0)) for j in range(12)]
        self.calls = [_call(m) for m in msgs]
        self.call_want = [REJECT if m.op.endswith(b"!") else ACCEPT for m in msgs]

    def check(self, a, what):
        st = a.verify_prehashed(self.e, self.r, self.s, self.slots)
        assert np.array_equal(st, self.want), what
        assert [int(x) for x in a.verify_batch(self.calls)] == self.call_want, what


def _classes(a, ids):
    return {i: a.key_class(ROLE_CLIENT, i)[0] for i in ids}


def _model(a, ids, ladder, budget, min_uses=0):
    """The classes mbft_rebalance_keys must leave, from the getters alone:
    every ladder key at the rung the Python plan gives its use bin."""
    slot = {i: a.key_slot(ROLE_CLIENT, i) for i in ids}
    uses, _ = a.key_usage(n=max(slot.values()) + 1)
    now = _classes(a, ids)
    on = [i for i in ids if now[i] in ladder]
    pinned = sum(class_bytes(now[i]) for i in ids if now[i] not in ladder)
    hist = [0] * NBINS
    for i in on:
        hist[use_bin(int(uses[slot[i]]))] += 1
    rung, nbytes, excess, _, _ = plan_model(hist, ladder, max(budget - pinned, 0), min_uses)
    want = dict(now)
    for i in on:
        want[i] = ladder[rung[use_bin(int(uses[slot[i]]))]]
    bins = {use_bin(int(uses[slot[i]])) for i in on}
    return want, now, pinned, nbytes, excess, bins


def _rebalance_and_check(a, ids, ladder, budget, min_uses=0):
    want, before, pinned, nbytes, excess, bins = _model(a, ids, ladder, budget, min_uses)
    slot_of = np.array([a.key_slot(ROLE_CLIENT, i) for i in ids], dtype=np.uint32)
    uses = a.key_usage(slot_of)
    live = a.key_memory()[0]
    a.set_key_budget(budget)
    assert a.key_budget() == budget
    res = a.rebalance_keys(ladder, min_uses)
    assert res["rc"] == 0
    after = _classes(a, ids)
    assert after == want
    byt = [class_bytes(c) for c in ladder]
    assert res["promoted"] == sum(class_bytes(after[i]) > class_bytes(before[i]) for i in ids)
    assert res["demoted"] == sum(class_bytes(after[i]) < class_bytes(before[i]) for i in ids)
    assert res["keys_per_rung"] == [sum(after[i] == c for i in ids) for c in ladder]
    assert res["live_before"] == live and res["live_after"] == a.key_memory()[0] == pinned + nbytes
    assert res["pinned_bytes"] == pinned
    assert res["over_budget"] == (pinned + nbytes - budget if excess else 0)
    if not excess:
        assert a.key_memory()[0] <= budget
    assert sum(n * b for n, b in zip(res["keys_per_rung"], byt)) == nbytes
    u2 = a.key_usage(slot_of)
    assert np.array_equal(u2[0], uses[0]) and np.array_equal(u2[1], uses[1])   # use counts are kept
    return res, after, bins


def test_rebalance_matches_the_plan(lib, points):
    from minbft_amd.authenticator import Authenticator
    nk = len(points)
    with Authenticator(0) as a:
        slot_of = _register(a, points)
        mix = Mix(a)
        ids = list(range(nk)) + mix.gold_ids
        a.set_key_class(ROLE_CLIENT, 199, PIN)
        a.set_key_accounting(True)
        mix.check(a, "registered")
        _load(a, slot_of, _skewed(nk), 1)
        budget = class_bytes(PIN) + 64 * (len(ids) - 1) + 950000
        a.set_key_budget(budget)
        assert a.key_budget() == budget
        res, after, bins = _rebalance_and_check(a, ids, LADDER, budget)
        assert len(bins) >= 4 and len(set(after[i] for i in range(nk - 1))) == 4   # every rung is in use
        assert after[0] == after[1] == 8 and after[150] == 0 and after[199] == PIN
        assert res["pinned_bytes"] == class_bytes(PIN) and res["demoted"] == 0 and res["promoted"] >= 100
        mix.check(a, "rebalanced")
        # again: the mix added a few uses, nothing else moved
        res, _, _ = _rebalance_and_check(a, ids, LADDER, budget)
        assert res["promoted"] + res["demoted"] <= len(mix.gold_ids) + 3
        # a floor on the uses sends the little used back to rung 0; a smaller budget demotes from the top
        res, after, _ = _rebalance_and_check(a, ids, LADDER, budget, min_uses=100)
        assert res["demoted"] >= 60 and after[50] == 0 and after[0] == 8
        mix.check(a, "min_uses 100")
        res, after, _ = _rebalance_and_check(a, ids, LADDER, budget - 600000)
        assert res["demoted"] >= 1 and a.key_memory()[0] <= budget - 600000
        mix.check(a, "smaller budget")
        # a two-rung ladder: the keys at the other rungs are pinned where they are
        res, after, _ = _rebalance_and_check(a, ids, [0, S(6)], budget)
        assert res["pinned_bytes"] > class_bytes(PIN)
        mix.check(a, "two rungs")


def test_ageing_demotes_and_storage_is_reused(lib, points):
    """Five hot keys at the top rung; aged to zero while five others take the
    load, they change places, and again, within the budget and -- after the
    first swap -- within the key blocks already held."""
    from minbft_amd.authenticator import Authenticator
    pts = points[:40]
    ladder = [0, S(3), 8]
    sets = [np.arange(0, 5), np.arange(5, 10)]
    with Authenticator(0) as a:
        slot_of = _register(a, pts)
        ids = list(range(len(pts)))
        a.set_key_accounting(True)
        budget = 64 * len(pts) + 5 * (class_bytes(8) - 64) + 100
        a.set_key_budget(budget)
        held = []
        batches = []
        for swap in range(4):
            hot, cold = sets[swap % 2], sets[1 - swap % 2]
            counts = np.zeros(len(pts), dtype=np.int64)
            counts[hot] = 2000
            a.age_key_usage(16)   # a few thousand uses >> 16: the former hot set reads zero
            assert not a.key_usage(n=int(slot_of.max()) + 1)[0].any()
            batches.append(_load(a, slot_of, counts, 10 + swap))
            res, after, _ = _rebalance_and_check(a, ids, ladder, budget)
            assert all(after[int(k)] == 8 for k in hot) and all(after[int(k)] == 0 for k in cold)
            assert (res["promoted"], res["demoted"]) == (5, 5 if swap else 0)
            assert a.key_memory()[0] <= budget
            held.append(a.key_memory()[2])
            for e, r, s, sl in batches:   # every batch so far still verifies
                assert (a.verify_prehashed(e, r, s, sl) == ACCEPT).all()
        assert held[1] == held[2] == held[3]


def test_over_budget_and_errors(lib, points):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    pts = points[:30]
    lad = np.array(LADDER, dtype=np.uint32)
    with Authenticator(0) as a:
        slot_of = _register(a, pts)
        ids = list(range(len(pts)))
        a.set_key_class(ROLE_CLIENT, 29, PIN)
        res = _lib.MbftRebalanceResult()

        def raw(ladder):
            ld = np.array(ladder, dtype=np.uint32)
            return a.lib.mbft_rebalance_keys(a.ctx, ld.ctypes.data, len(ld), 0, res)
        # accounting off, then no budget: MBFT_ERR_STATE
        a.set_key_budget(1 << 20)
        assert raw(LADDER) == _lib.ERR_STATE
        a.set_key_accounting(True)
        a.set_key_budget(0)
        assert raw(LADDER) == _lib.ERR_STATE
        a.set_key_budget(1 << 20)
        # ladders the rule refuses: MBFT_ERR_ARG
        for bad in ([S(5), 0], [0, S(5), 0x104], [0, S(9), 4], [0, 0x102, S(4)], [0, 3], [],
                    [0, S(2), S(3), S(4), S(5), S(7), S(9), 8, 12]):
            assert raw(bad) == _lib.ERR_ARG, bad
        assert a.lib.mbft_rebalance_keys(a.ctx, lad.ctypes.data, 4, 0, None) == _lib.ERR_ARG
        assert a.lib.mbft_age_key_usage(a.ctx, 64) == _lib.ERR_ARG
        assert a.lib.mbft_age_key_usage(a.ctx, 0) == _lib.OK
        assert _classes(a, ids) == {**{i: 0 for i in ids}, 29: PIN}
        # the cost model through the C-ABI
        assert [a.key_class_cost(c) for c in (0, S(3), 0x103, 8, 16, 3, 0x300)] == [2908, 1540, 1540, 320, 160, 0, 0]
        # a budget below keys x 64: everything to rung 0, the excess exact, MBFT_OK
        _load(a, slot_of, np.full(len(pts), 20), 3)
        a.set_slot_classes(slot_of[:10], S(6))
        budget = 64 * 29 - 1
        a.set_key_budget(budget)
        r2, after, _ = _rebalance_and_check(a, ids, LADDER, budget)
        assert r2["over_budget"] == class_bytes(PIN) + 64 * 29 - budget and r2["demoted"] == 10
        assert all(after[i] == 0 for i in range(29)) and after[29] == PIN


def test_cold_keys(lib, points):
    from minbft_amd.authenticator import Authenticator
    pts = points[:60]
    with Authenticator(0) as a:
        slot_of = _register(a, pts)
        # before any count exists every valid slot is cold
        got, total = a.cold_keys(0, 100)
        assert total == 60 and np.array_equal(got, np.sort(slot_of))
        a.set_key_accounting(True)
        counts = np.arange(60) % 7          # keys 0, 7, 14 ...: no use; the others 1 .. 6
        _load(a, slot_of, counts, 5)
        for max_uses in (0, 2, 6):
            want = np.sort(slot_of[counts <= max_uses])
            for cap in (len(want) + 3, len(want), 4, 0):
                got, total = a.cold_keys(max_uses, cap)
                assert total == len(want)
                assert np.array_equal(got, want[:cap]), (max_uses, cap)   # ascending, the cap lowest
        # released slots are never listed
        a.remove_public_key(ROLE_CLIENT, 0)
        a.remove_public_key(ROLE_CLIENT, 14)
        got, total = a.cold_keys(0, 100)
        assert np.array_equal(got, np.sort(slot_of[[7, 21, 28, 35, 42, 49, 56]])) and total == 7
        assert a.key_memory()[0] == 58 * 64 and not a.key_budget()   # it changes nothing, and needs no budget


def test_two_engines(lib, points):
    """A sharded batch first, so that both engines hold counts: the plan is the
    model's on the summed counts, both engines verify the mix as before, and an
    ageing leaves every slot's sum within the stated interval."""
    from minbft_amd.authenticator import Authenticator
    from test_gpu_multi import _extra_devices
    pts = points[:80]
    with Authenticator(0) as a:
        slot_of = _register(a, pts)
        ids = list(range(len(pts)))
        a.set_key_accounting(True)
        a.add_device(_extra_devices(1)[0])
        a.set_shard_min(512)
        counts = np.zeros(len(pts), dtype=np.int64)
        counts[:4], counts[4:20], counts[20:50] = [1501, 800, 799, 300], 40, 3
        e, r, s, sl = _load(a, slot_of, counts, 7)   # 5,000 items: two shards
        uses, _ = a.key_usage(slot_of)
        assert np.array_equal(uses, counts.astype(np.uint64))
        budget = 64 * len(pts) + 2 * class_bytes(8) + 40000
        a.set_key_budget(budget)
        res, after, bins = _rebalance_and_check(a, ids, LADDER, budget)
        assert after[0] == 8 and after[79] == 0 and len(bins) >= 4
        e2 = e.copy()
        e2[::3, 31] ^= 1
        want = np.where(np.arange(len(e)) % 3 == 0, REJECT, ACCEPT)
        assert np.array_equal(a.verify_prehashed(e2, r, s, sl), want)     # sharded: both engines, the new classes
        total, _ = a.key_usage(slot_of)
        assert np.array_equal(total, 2 * counts.astype(np.uint64))
        a.age_key_usage(1)
        aged, _ = a.key_usage(slot_of)
        half = total >> np.uint64(1)
        assert (aged <= half).all() and (aged + np.uint64(1) >= half).all()   # two parts: within one of the whole's shift
