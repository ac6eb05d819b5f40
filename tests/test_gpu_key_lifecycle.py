"""The life of a key after registration, through the C-ABI, against the
golden expectations and the oracle: re-classing of registered keys (every
status unchanged after every step), removal with reuse of slot numbers and
storage, per-key use counts taken on the GPU, and promotion by count.

Classes are the public codes: a comb window 4..29, 0 (table-free),
``_lib.key_class_teeth(t)``.  Batch sizes 300 and 4,097: a small-batch form,
and the large form with its two queues.
"""
import hashlib
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays

pytestmark = pytest.mark.gpu

ACCEPT, REJECT, UNKNOWN_KEY, BAD_KEY = 0, 1, 4, 5
ROLE_CLIENT = 3
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
SIZES = (300, 4097)


def T(t):
    return 0x100 | t


def class_bytes(cls):
    if cls == 0:
        return 64
    if cls >= 0x100:
        return 64 << (cls & 0xFF)
    s = -(-256 // cls)
    return 64 * (((s - 1) << (cls - 1)) + (1 << (256 - (s - 1) * cls)))


def _check(st, exp, labels, what=""):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i % len(labels)], i, int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, len(bad), bad[:10])
    assert set(np.unique(st).tolist()) <= {ACCEPT, REJECT}, what


def _register_ids(a, xy):
    """Every distinct key of xy under (ROLE_CLIENT, k); the slot per item and
    the ids."""
    keys, inv = np.unique(xy, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    a.add_role(ROLE_CLIENT)
    for k, q in enumerate(keys):
        a.set_public_key(ROLE_CLIENT, k, bytes(q))
    slot_of = np.array([a.key_slot(ROLE_CLIENT, k) for k in range(len(keys))], dtype=np.uint32)
    return slot_of[inv], slot_of, len(keys)


def _run_sizes(a, e, r, s, slots, exp, labels, what):
    for n in SIZES:
        idx = np.arange(n) % len(labels)
        st = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
        _check(st, exp[idx], [labels[i] for i in idx], "%s n=%d" % (what, n))


# ----------------------------------------------------------------- re-classing
def test_reclass_walk_golden(lib):
    """The 551 prehashed vectors' keys, registered table-free, walked through
    0 -> t=2 -> t=8 -> W=4 -> W=16 -> t=4 -> 0 (the bulk form, the last key by
    the single form): after every step every status is what it was and
    mbft_get_key_class / mbft_key_memory report the step."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays()
    assert len(labels) == 551
    with Authenticator(0) as a:
        a.set_key_window(0)
        slots, slot_of, nk = _register_ids(a, xy)
        assert a.key_memory()[0] == 64 * nk
        _run_sizes(a, e, r, s, slots, exp, labels, "registered")
        blocks = a.key_memory()[2]
        for cls in (T(2), T(8), 4, 16, T(4), 0):
            a.set_slot_classes(slot_of[:-1], cls)
            assert a.key_class(ROLE_CLIENT, nk - 1)[0] != cls  # (the bulk call named the others only)
            a.set_key_class(ROLE_CLIENT, nk - 1, cls)
            for k in range(nk):
                assert a.key_class(ROLE_CLIENT, k) == (cls, class_bytes(cls)), (cls, k)
            live, listed, held = a.key_memory()
            assert live == nk * class_bytes(cls)
            assert held >= blocks and held >= live + listed
            blocks = held
            _run_sizes(a, e, r, s, slots, exp, labels, "class %#x" % cls)
        # back at window 0 every piece of the first round was there to take: no new block
        a.set_slot_classes(slot_of, T(2))
        assert a.key_memory()[2] == blocks
        a.set_slot_classes(slot_of, T(2))  # already there: nothing to do
        assert a.key_memory()[2] == blocks
        _run_sizes(a, e, r, s, slots, exp, labels, "again t=2")


@pytest.mark.parametrize("name", ["ladder_edges.json", "teeth_edges.json"])
def test_edges_under_reclassed_keys(lib, name):
    """The crafted edge vectors under keys that ARRIVED in window 0 and t = 4
    by re-class (registered at W = 8)."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays(name)
    with Authenticator(0) as a:
        a.set_key_window(8)
        slots, slot_of, nk = _register_ids(a, xy)
        for cls in (0, T(4)):
            a.set_slot_classes(slot_of, cls)
            assert a.key_class(ROLE_CLIENT, 0) == (cls, class_bytes(cls))
            _run_sizes(a, e, r, s, slots, exp, labels, "%s class %#x" % (name, cls))


def test_three_classes_one_reclassed(lib):
    """Keys of three classes in every wave; one key is re-classed between two
    runs of the same batch."""
    from minbft_amd.authenticator import Authenticator
    from test_gpu_compact_keys import _register_classes
    parts = [prehashed_arrays(), prehashed_arrays("ladder_edges.json"), prehashed_arrays("teeth_edges.json")]
    xy, e, r, s, exp = (np.concatenate([p[k] for p in parts]) for k in range(5))
    labels = sum((p[5] for p in parts), [])
    with Authenticator(0) as a:
        slots, cls = _register_classes(a, xy, [("t", 4), ("w", 8), ("w", 0)])
        groups = [np.nonzero(cls == ci)[0] for ci in range(3)]
        for n in SIZES:
            idx = np.array([groups[i % 3][(i // 3) % len(groups[i % 3])] for i in range(n)])
            for w in range(0, n - 63, 64):
                assert set(cls[idx[w:w + 64]].tolist()) == {0, 1, 2}
            lab = [labels[i] for i in idx]
            _check(a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx]), exp[idx], lab, "before n=%d" % n)
            one = slots[groups[n % 3][0]]  # a t = 4 key at 4,097, a window-0 key at 300
            a.set_slot_classes(np.array([one]), 12)
            _check(a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx]), exp[idx], lab, "after n=%d" % n)


def test_failure_keeps_the_class(lib):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays()
    with Authenticator(0) as a:
        a.set_key_teeth(3)
        slots, slot_of, nk = _register_ids(a, xy)
        mem = a.key_memory()
        for bad in (1, 3, 30, 0xFF, T(0), T(1), T(9), 0x200, 0xFFFFFFFF):
            assert a.lib.mbft_set_key_class(a.ctx, ROLE_CLIENT, 0, bad) == _lib.ERR_ARG
            assert a.lib.mbft_set_slot_classes(a.ctx, slot_of.ctypes.data, nk, bad) == _lib.ERR_ARG
        assert a.lib.mbft_set_key_class(a.ctx, ROLE_CLIENT, nk + 5, 8) == _lib.ERR_KEY
        far = np.array([int(slot_of.max()) + 1], dtype=np.uint32)
        assert a.lib.mbft_set_slot_classes(a.ctx, far.ctypes.data, 1, 8) == _lib.ERR_ARG
        assert a.key_memory() == mem
        assert all(a.key_class(ROLE_CLIENT, k) == (T(3), 512) for k in range(nk))
        _run_sizes(a, e, r, s, slots, exp, labels, "after refusals")


# --------------------------------------------------------------------- removal
def _key(tag):
    from oracle import p256 as o
    d = int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big") % (o.N - 1) + 1
    return d, o.pubkey(d)


def _request(d, client, seq, tamper=False):
    """A signed REQUEST of `client` (and the VerifyMessageAuthenTag call it
    stands for); tamper: the operation changed after signing."""
    from oracle import p256 as o
    m = o.Msg(type=o.MSG_REQUEST, stream=seq, client_id=client, seq=seq, op=b"op %d" % seq)
    r, s = o.ecdsa_sign(d, o.quirk_digest(o.msg_authen_bytes(m)))
    m.sig = o.der_encode_sig(r, s)
    if tamper:
        m.op = m.op + b"!"
    return m


def _call(m):
    from oracle import p256 as o
    return (ROLE_CLIENT, m.client_id, o.msg_authen_bytes(m), m.sig)


def _every_entry_point(a, msgs, want, resident_too=True):
    """The calls of msgs (REQUESTs) through verify_batch, the flat and the
    compact flat form (device-decoded), check_messages_flat past the small
    route, and lone calls with the resident verifier off and on."""
    from oracle import p256 as o
    from test_gpu_small_check import _packed
    calls = [_call(m) for m in msgs]
    assert [int(x) for x in a.verify_batch(calls)] == want, "verify_batch"
    assert [int(x) for x in a.verify_batch_flat(calls, pinned=True)] == want, "flat"
    assert [int(x) for x in a.verify_batch_flat32(calls, pinned=True)] == want, "flat32"
    reps = 520 // len(msgs) + 1
    tiled = msgs * reps
    assert len(tiled) > 512
    recs, arena = _packed(a, tiled)
    with a.check_messages_flat(recs, arena, 4) as b:
        got = [b.resolve(j) for j in range(len(tiled))]
    assert got == [0 if w == 0 else (o.ST_REQUEST_SIG << 8) | w for w in want] * reps, "check_messages_flat"
    for res in ((0, 16) if resident_too else (0,)):
        a.set_resident(res)
        assert [a.verify_status(*c) for c in calls] == want, "lone calls, resident %d" % res
    a.set_resident(0)


def test_removal_and_rotation(lib, monkeypatch):
    import torch
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    from test_gpu_tablefree import _oracle_auth
    _fast_oracle(monkeypatch)
    (d1, q1), (d2, q2), (d3, q3) = _key("life a"), _key("life b"), _key("life c")
    # ids 10 and 11 share key 1, id 12 has key 2; id 99 is never registered
    msgs = [_request(d1, 10, 1), _request(d1, 11, 2), _request(d2, 12, 3), _request(d1, 10, 4, tamper=True),
            _request(d2, 99, 5), _request(d1, 12, 6)]
    keys = {ROLE_CLIENT: {10: q1, 11: q1, 12: q2}}

    def want():
        ref = _oracle_auth(keys)
        return [ref.verify(*_call(m)) for m in msgs]

    with Authenticator(0) as a:
        a.set_small_check(0)  # (every check takes the device message layer)
        a.add_role(ROLE_CLIENT)
        a.set_key_window(8)
        for id_, q in keys[ROLE_CLIENT].items():
            a.set_public_key(ROLE_CLIENT, id_, o.pkix_encode(q))
        s1, s2 = a.key_slot(ROLE_CLIENT, 10), a.key_slot(ROLE_CLIENT, 12)
        assert a.key_slot(ROLE_CLIENT, 11) == s1 != s2
        w0 = want()
        assert w0 == [ACCEPT, ACCEPT, ACCEPT, REJECT, UNKNOWN_KEY, REJECT]
        _every_entry_point(a, msgs, w0)
        # id 10 leaves: unknown like an id never registered; id 11 goes on verifying on the same point
        a.remove_public_key(ROLE_CLIENT, 10)
        assert a.lib.mbft_remove_public_key(a.ctx, ROLE_CLIENT, 10) == _lib.ERR_KEY
        assert a.lib.mbft_key_slot(a.ctx, ROLE_CLIENT, 10) == _lib.ERR_KEY
        del keys[ROLE_CLIENT][10]
        w1 = want()
        assert w1 == [UNKNOWN_KEY, ACCEPT, ACCEPT, UNKNOWN_KEY, UNKNOWN_KEY, REJECT]
        _every_entry_point(a, msgs, w1)
        assert a.key_slot(ROLE_CLIENT, 11) == s1 and a.key_memory()[1] == 0
        # ... until it too is removed: the slot is released, its raw number reads BAD_KEY on the device
        a.remove_public_key(ROLE_CLIENT, 11)
        del keys[ROLE_CLIENT][11]
        w2 = want()
        assert w2 == [UNKNOWN_KEY, UNKNOWN_KEY, ACCEPT, UNKNOWN_KEY, UNKNOWN_KEY, REJECT]
        _every_entry_point(a, msgs, w2)
        assert a.key_memory()[:2] == (class_bytes(8), class_bytes(8))
        dev = torch.device("cuda", 0)
        m = msgs[0]
        rr, ss, _ = o.der_parse_sig(m.sig)
        items = [np.frombuffer(o.quirk_digest(o.msg_authen_bytes(m)), dtype=np.uint8),
                 np.frombuffer(rr.to_bytes(32, "big"), dtype=np.uint8),
                 np.frombuffer(ss.to_bytes(32, "big"), dtype=np.uint8)]
        de, dr, ds = (torch.from_numpy(np.stack([v, v]).copy()).to(dev) for v in items)
        dsl = torch.from_numpy(np.array([s1, s2], dtype=np.uint32).view(np.int32)).to(dev)
        dst = torch.full((2,), 0xAA, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        a.verify_prehashed_device(de.data_ptr(), dr.data_ptr(), ds.data_ptr(), dsl.data_ptr(), 2, dst.data_ptr(), 0)
        torch.cuda.synchronize()
        assert dst.cpu().numpy().tolist() == [BAD_KEY, REJECT]
        # rotation: the same (role, id) comes back with another key, in the released slot
        a.set_public_key(ROLE_CLIENT, 10, o.pkix_encode(q3))
        assert a.key_slot(ROLE_CLIENT, 10) == s1 and a.key_memory()[1] == 0
        keys[ROLE_CLIENT][10] = q3
        new = _request(d3, 10, 7)
        msgs2 = msgs + [new]
        ref = _oracle_auth(keys)
        w3 = [ref.verify(*_call(x)) for x in msgs2]
        assert w3 == [REJECT, UNKNOWN_KEY, ACCEPT, REJECT, UNKNOWN_KEY, REJECT, ACCEPT]
        _every_entry_point(a, msgs2, w3)
        # rotation by overwriting: the pair is mapped to another key without a remove in between;
        # its earlier slot is released (nothing else maps to it) and its table goes on the list
        live, listed, _ = a.key_memory()
        a.set_public_key(ROLE_CLIENT, 10, o.pkix_encode(q1))
        s4 = a.key_slot(ROLE_CLIENT, 10)
        assert s4 != s1 and a.key_memory()[:2] == (live, listed + class_bytes(8))
        keys[ROLE_CLIENT][10] = q1
        ref = _oracle_auth(keys)
        w4 = [ref.verify(*_call(x)) for x in msgs2]
        assert w4 == [ACCEPT, UNKNOWN_KEY, ACCEPT, REJECT, UNKNOWN_KEY, REJECT, REJECT]
        _every_entry_point(a, msgs2, w4, resident_too=False)
        a.set_public_key(ROLE_CLIENT, 10, o.pkix_encode(q1))  # the same key again: nothing moves
        assert a.key_slot(ROLE_CLIENT, 10) == s4 and a.key_memory()[:2] == (live, listed + class_bytes(8))
        # a pair that shares its slot with another leaves it in place
        a.set_public_key(ROLE_CLIENT, 11, o.pkix_encode(q1))
        a.set_public_key(ROLE_CLIENT, 11, o.pkix_encode(q2))
        assert a.key_slot(ROLE_CLIENT, 10) == s4 and a.key_slot(ROLE_CLIENT, 11) == s2
        assert a.verify_status(*_call(msgs2[0])) == ACCEPT


def _chain(count, start=2):
    """count distinct valid points: start G, (start + 1) G, ..."""
    from oracle import p256 as o
    pts, p = [], o.scalar_mult(start, o.G)
    for _ in range(count):
        pts.append(p)
        p = o.point_add(p, o.G)
    return pts


def _crafted(pts, first, which, rng):
    """A valid signature under key pts[k] = (first + k) G for every k of
    `which`, made without the key's discrete log (the construction of
    test_gpu_compact_keys.test_many_keys): R = t G with t = u1 + u2 d."""
    from oracle import p256 as o
    cyc = [o.scalar_mult(k, o.G) for k in range(1, 40)]
    e, r, s = (np.zeros((len(which), 32), dtype=np.uint8) for _ in range(3))
    for i, k in enumerate(which):
        d, u2 = first + int(k), rng.randrange(1, N)
        t = 1 + i % 39
        u1 = (t - u2 * d) % N
        rr = cyc[t - 1][0] % N
        ss = rr * pow(u2, -1, N) % N
        e[i] = np.frombuffer((u1 * ss % N).to_bytes(32, "big"), dtype=np.uint8)
        r[i] = np.frombuffer(rr.to_bytes(32, "big"), dtype=np.uint8)
        s[i] = np.frombuffer(ss.to_bytes(32, "big"), dtype=np.uint8)
    return e, r, s


def _xy(q):
    return q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


@pytest.mark.parametrize("cls", [T(4), 0, 4])
def test_churn_keeps_memory_and_slots(lib, cls):
    """300 rounds of register-one and remove-one: after the first round the
    key blocks held and the highest slot number stay what they are."""
    from minbft_amd.authenticator import Authenticator
    pts = _chain(302)
    e, r, s = _crafted(pts, 2, range(302), random.Random(cls))
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        if cls >= 0x100:
            a.set_key_teeth(cls & 0xFF)
        else:
            a.set_key_window(cls)
        a.set_public_key(ROLE_CLIENT, 0, _xy(pts[0]))  # a resident of the store, beside the churn
        held = top = None
        for k in range(1, 301):
            a.set_public_key(ROLE_CLIENT, k, _xy(pts[k]))
            sl = a.key_slot(ROLE_CLIENT, k)
            if k % 50 == 1:  # the newcomer verifies in its (reused) slot and storage
                st = a.verify_prehashed(e[[0, k, k]], r[[0, k, k]], s[[0, k - 1, k]],
                                        np.array([a.key_slot(ROLE_CLIENT, 0), sl, sl]))
                assert st.tolist() == [ACCEPT, REJECT, ACCEPT], k
            a.remove_public_key(ROLE_CLIENT, k)
            live, listed, blocks = a.key_memory()
            assert (live, listed) == (class_bytes(cls), class_bytes(cls))
            if k == 1:
                held, top = blocks, sl
            assert (blocks, sl) == (held, top), k


# ------------------------------------------------------------------ use counts
def _mix(rng, n, nkeys):
    """n items over nkeys keys ((k + 2) G): key, tampered or not, and for some
    an id / slot that is not registered."""
    key = rng.integers(0, nkeys, n)
    tam = rng.random(n) < 0.2
    unk = rng.random(n) < 0.1
    return key, tam, unk


def test_accounting_end_to_end(lib):
    import torch
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    from test_gpu_small_check import _packed
    nkeys, n = 6, 5000
    pts = _chain(nkeys)
    rng = np.random.default_rng(41)
    key, tam, unk = _mix(rng, n, nkeys)
    e, r, s = _crafted(pts, 2, key, random.Random(5))
    e[tam, 31] ^= 1
    dkeys = [_key("acct %d" % k) for k in range(3)]
    signed = [_request(dkeys[k % 3][0], 100 + k % 3 if k % 7 else 99, k, tamper=(k % 5 == 0)) for k in range(40)]
    with Authenticator(0) as a:
        a.set_small_check(0)
        a.add_role(ROLE_CLIENT)
        a.set_key_window(0)
        for k in range(nkeys):
            a.set_public_key(ROLE_CLIENT, k, _xy(pts[k]))
        a.set_key_teeth(4)
        for k in range(3):
            a.set_public_key(ROLE_CLIENT, 100 + k, o.pkix_encode(dkeys[k][1]))
        slot_of = np.array([a.key_slot(ROLE_CLIENT, k) for k in range(nkeys)], dtype=np.uint32)
        nslots = nkeys + 3
        slots = slot_of[key].copy()
        slots[unk] = nslots + 7
        want_st = np.where(unk, BAD_KEY, np.where(tam, REJECT, ACCEPT))
        tally_u = np.bincount(slots[~unk], minlength=nslots).astype(np.uint64)
        tally_r = np.bincount(slots[~unk & tam], minlength=nslots).astype(np.uint64)

        def usage():
            return a.key_usage(n=nslots)

        # off: nothing is counted
        assert (a.verify_prehashed(e, r, s, slots) == want_st).all()
        u, rj = usage()
        assert not u.any() and not rj.any()
        a.set_key_accounting(True)
        # the host form (one engine) and the device form on a stream of the caller's
        assert (a.verify_prehashed(e, r, s, slots) == want_st).all()
        u, rj = usage()
        assert np.array_equal(u, tally_u) and np.array_equal(rj, tally_r)
        dev = torch.device("cuda", 0)
        d = [torch.from_numpy(v).to(dev) for v in (e, r, s)]
        d.append(torch.from_numpy(slots.view(np.int32)).to(dev))
        d.append(torch.full((n,), 0xAA, dtype=torch.uint8, device=dev))
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        a.verify_prehashed_device(*(t.data_ptr() for t in d[:4]), n, d[4].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert (d[4].cpu().numpy() == want_st).all()
        u, rj = usage()
        assert np.array_equal(u, 2 * tally_u) and np.array_equal(rj, 2 * tally_r)
        a.reset_key_usage()
        u, rj = usage()
        assert not u.any() and not rj.any()
        # calls: verify_batch and the flat form count the calls that reach the GPU under a known id
        calls = [_call(m) for m in signed] * 125
        assert len(calls) == n
        sl_of_id = {100 + k: a.key_slot(ROLE_CLIENT, 100 + k) for k in range(3)}
        cu, cr = np.zeros(nslots, dtype=np.uint64), np.zeros(nslots, dtype=np.uint64)
        st_want = []
        for m in signed:
            if m.client_id == 99:
                st_want.append(UNKNOWN_KEY)
                continue
            bad = m.op.endswith(b"!")
            st_want.append(REJECT if bad else ACCEPT)
            cu[sl_of_id[m.client_id]] += 1
            cr[sl_of_id[m.client_id]] += int(bad)
        assert [int(x) for x in a.verify_batch(calls)] == st_want * 125
        u, rj = usage()
        assert np.array_equal(u, 125 * cu) and np.array_equal(rj, 125 * cr)
        assert [int(x) for x in a.verify_batch_flat(calls, pinned=True)] == st_want * 125
        u, rj = usage()
        assert np.array_equal(u, 250 * cu) and np.array_equal(rj, 250 * cr)
        # the message layer verifies identical calls once: the counts are verifies performed
        a.reset_key_usage()
        recs, arena = _packed(a, signed * 15)
        with a.check_messages_flat(recs, arena, 4) as b:
            got = [b.resolve(j) for j in range(len(signed) * 15)]
        assert got == [0 if w == 0 else (o.ST_REQUEST_SIG << 8) | w for w in st_want] * 15
        u, rj = usage()
        assert np.array_equal(u, cu) and np.array_equal(rj, cr)
        # counts survive a re-class ...
        a.set_slot_classes(np.array(list(sl_of_id.values()), dtype=np.uint32), 8)
        u2, rj2 = usage()
        assert np.array_equal(u2, cu) and np.array_equal(rj2, cr)
        # ... a resident call is counted (W = 8 keys: the resident verifier serves them) ...
        a.set_resident(16)
        first = next(m for m in signed if m.client_id == 100 and not m.op.endswith(b"!"))
        assert a.verify_status(*_call(first)) == ACCEPT
        assert a.resident_stats()["calls"] >= 1
        a.set_resident(0)
        u3, _ = usage()
        cu[sl_of_id[100]] += 1
        assert np.array_equal(u3, cu)
        # ... and are zero once the slot is released and reused
        a.remove_public_key(ROLE_CLIENT, 100)
        a.set_public_key(ROLE_CLIENT, 200, _xy(_chain(1, 1000)[0]))
        assert a.key_slot(ROLE_CLIENT, 200) == sl_of_id[100]
        u4, rj4 = usage()
        cu[sl_of_id[100]] = cr[sl_of_id[100]] = 0
        assert np.array_equal(u4, cu) and np.array_equal(rj4, cr)


def test_accounting_two_engines(lib):
    """A sharded batch: each engine counts its shard, the read sums them."""
    from minbft_amd.authenticator import Authenticator
    from test_gpu_multi import _extra_devices
    nkeys, n = 5, 5000
    pts = _chain(nkeys)
    rng = np.random.default_rng(43)
    key, tam, unk = _mix(rng, n, nkeys)
    e, r, s = _crafted(pts, 2, key, random.Random(6))
    e[tam, 31] ^= 1
    with Authenticator(0) as a:
        a.set_key_teeth(3)
        a.set_key_accounting(True)
        slot_of, valid = a.register_points(np.array([list(_xy(q)) for q in pts], dtype=np.uint8))
        a.add_device(_extra_devices(1)[0])
        a.set_shard_min(512)
        slots = slot_of[key].copy()
        slots[unk] = nkeys + 3
        st = a.verify_prehashed(e, r, s, slots)
        assert (st == np.where(unk, BAD_KEY, np.where(tam, REJECT, ACCEPT))).all()
        u, rj = a.key_usage(n=nkeys)
        assert np.array_equal(u, np.bincount(slots[~unk], minlength=nkeys).astype(np.uint64))
        assert np.array_equal(rj, np.bincount(slots[~unk & tam], minlength=nkeys).astype(np.uint64))
        # a re-class reaches both engines: the sharded batch verifies as before
        a.set_slot_classes(slot_of, 8)
        assert (a.verify_prehashed(e, r, s, slots) == st).all()
        # and so does a release: the raw slot numbers are given up
        a.release_slots(slot_of[:2])
        gone = np.isin(slots, slot_of[:2])
        st2 = a.verify_prehashed(e, r, s, slots)
        assert (st2 == np.where(gone, BAD_KEY, st)).all()


# ------------------------------------------------------------------- promotion
def test_promotion_by_count(lib):
    """64 table-free keys; key 7 signs 3,000 of 4,200 items, key 9 signs 600,
    the rest a few each.  mbft_promote_hot_keys(ctx, 8, 2, 500) moves exactly
    those two to W = 8; the batch's statuses are what they were."""
    from minbft_amd.authenticator import Authenticator
    nkeys, n = 64, 4200
    pts = _chain(nkeys)
    rest = [k for k in range(nkeys) if k not in (7, 9)]
    key = np.array([7] * 3000 + [9] * 600 + [rest[i % len(rest)] for i in range(600)])
    np.random.default_rng(3).shuffle(key)
    e, r, s = _crafted(pts, 2, key, random.Random(8))
    tam = np.arange(n) % 9 == 0
    e[tam, 31] ^= 1
    want = np.where(tam, REJECT, ACCEPT)
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        a.set_key_window(0)
        for k in range(nkeys):
            a.set_public_key(ROLE_CLIENT, k, _xy(pts[k]))
        slots = np.array([a.key_slot(ROLE_CLIENT, k) for k in range(nkeys)], dtype=np.uint32)[key]
        a.set_key_accounting(True)
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
        assert a.promote_hot_keys(8, 2, 3001) == 0   # nobody has that many
        assert a.promote_hot_keys(8, 2, 3000) == 1   # only key 7 does
        assert a.key_class(ROLE_CLIENT, 7)[0] == 8 and a.key_class(ROLE_CLIENT, 9)[0] == 0
        a.set_key_class(ROLE_CLIENT, 7, 0)           # (back, by hand; the counts are kept)
        assert a.promote_hot_keys(8, 2, 500) == 2
        for k in range(nkeys):
            assert a.key_class(ROLE_CLIENT, k) == ((8, class_bytes(8)) if k in (7, 9) else (0, 64)), k
        assert a.key_memory()[0] == 2 * class_bytes(8) + 62 * 64
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
        assert a.promote_hot_keys(8, 2, 500) == 0    # already there
        # every key promoted: none is of a queued class any more
        assert a.promote_hot_keys(8, nkeys, 0) == 62
        assert all(a.key_class(ROLE_CLIENT, k) == (8, class_bytes(8)) for k in range(nkeys))
        assert a.key_memory()[0] == nkeys * class_bytes(8)
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
