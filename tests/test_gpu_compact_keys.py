"""Compact keys (mbft_set_key_teeth, t = 2..8 teeth): a key with a small table
of 2^t entries, verified by a comb with doublings
(minbft_amd/csrc/teeth_dev.h) -- through the C-ABI, against the golden
expectations and the oracle.

* the prehashed golden set, tests/golden/ladder_edges.json and
  tests/golden/teeth_edges.json (vectors crafted from chosen (u1, u2): single
  teeth, single columns, all-ones and zero columns, the ragged top tooth,
  Q = +-G joins) with every key compact, for every t as one batch and, tiled
  past 4,096 items, through k_verify, the second compacted queue and
  k_verify_ladder; each small-batch form at t = 3 and t = 8;
* window 8, window 0, teeth 4 and teeth 6 side by side with all four in every
  wave; the queue's shapes (empty, one item per wave, out-of-range r / s, an
  off-curve slot, a slot out of range);
* four batches in flight on one stream;
* every entry point against the oracle with compact client keys: lone calls
  (resident verifier off and on), verify_batch, the device-decoded flat form,
  the message layer's device and small routes;
* two engines; the key store (key_teeth(), windows(), refused teeth, clear
  and re-register, 20,000 keys in one call, 300 one by one).
"""
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays

pytestmark = pytest.mark.gpu

REJECT, BAD_KEY = 1, 5
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


@pytest.fixture(scope="module")
def golden():
    """prehashed.json (551 vectors) + ladder_edges.json + teeth_edges.json, as one set."""
    parts = [prehashed_arrays(), prehashed_arrays("ladder_edges.json"), prehashed_arrays("teeth_edges.json")]
    assert len(parts[0][5]) == 551 and len(parts[1][5]) >= 200 and 200 <= len(parts[2][5]) <= 400
    xy, e, r, s, exp = (np.concatenate([p[k] for p in parts]) for k in range(5))
    return xy, e, r, s, exp, sum((p[5] for p in parts), [])


def _check(st, exp, labels, what=""):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i % len(labels)], i, int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, len(bad), bad[:10])
    assert set(np.unique(st).tolist()) <= {0, REJECT}, what


def _tile(arrs, reps):
    return [np.concatenate([a] * reps) for a in arrs]


@pytest.mark.parametrize("shape", ["one_batch", "large"])
@pytest.mark.parametrize("t", list(range(2, 9)))
def test_golden_every_teeth(lib, golden, t, shape):
    """Every key compact with t teeth: the golden set as one batch (the
    small-batch kernels serve it in place), and tiled just past 4,096 items
    (k_verify queues every item, k_verify_ladder serves the queue)."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    reps = 1 if shape == "one_batch" else 4096 // len(labels) + 1
    with Authenticator(0) as a:
        a.set_key_teeth(t)
        assert a.key_teeth() == t and a.windows()[1] == 0
        slots, valid = a.register_points(xy)
        assert valid.all()
        te, tr, ts, tsl, texp = _tile([e, r, s, slots, exp], reps)
        assert (len(texp) > 4096) == (shape == "large")
        st = a.verify_prehashed(te, tr, ts, tsl)
    _check(st, texp, labels, "t=%d" % t)


@pytest.mark.parametrize("t", [3, 8])
@pytest.mark.parametrize("form", ["default", "split", "pairs", "pairs_lane_inv", "quads", "quads_planes"])
def test_golden_small_forms(lib, golden, form, t):
    """Batches of <= 200 under each small-batch setting, at t = 3 (ragged top
    tooth) and t = 8."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    with Authenticator(0) as a:
        if form != "default":
            a.set_small_batch_form(256 if form == "split" else 0)
            a.set_small_batch_inverse({"pairs_lane_inv": 0, "quads": 2, "quads_planes": 3}.get(form, 1))
        a.set_key_teeth(t)
        slots, valid = a.register_points(xy)
        assert valid.all()
        st = np.concatenate([a.verify_prehashed(e[k:k + 200], r[k:k + 200], s[k:k + 200], slots[k:k + 200])
                             for k in range(0, len(labels), 200)])
    _check(st, exp, labels, "%s t=%d" % (form, t))


def _register_classes(a, xy, classes):
    """Deals the distinct keys of xy to the classes (("w", W) or ("t", T)) --
    the key with the most vectors first, each to the class that has the
    fewest vectors so far, since a point has one class per context -- and
    registers them.  Returns the slots and the class index per item."""
    keys, inv, cnt = np.unique(xy, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    load, class_of_key = [0] * len(classes), np.zeros(len(keys), dtype=np.int64)
    for k in np.argsort(-cnt, kind="stable"):
        ci = load.index(min(load))
        class_of_key[k] = ci
        load[ci] += int(cnt[k])
    slots = np.zeros(len(xy), dtype=np.uint32)
    cls = class_of_key[inv]
    for ci, (kind, val) in enumerate(classes):
        (a.set_key_window if kind == "w" else a.set_key_teeth)(val)
        sl, v = a.register_points(xy[cls == ci])
        assert v.all()
        slots[cls == ci] = sl
    return slots, cls


def test_mixed_classes(lib, golden):
    """Window 8, window 0, teeth 4 and teeth 6 in one context, the items
    ordered so that every four consecutive ones -- hence every wave -- hold
    all four classes: below and above 4,096 items."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    order = np.random.default_rng(11).permutation(len(labels))
    xy, e, r, s, exp = (v[order] for v in (xy, e, r, s, exp))
    labels = [labels[i] for i in order]
    with Authenticator(0) as a:
        # (the two fixture keys, which have the most vectors, land in the compact classes)
        slots, cls = _register_classes(a, xy, [("t", 4), ("t", 6), ("w", 8), ("w", 0)])
        assert a.key_teeth() == 0 and a.windows()[1] == 0
        groups = [np.nonzero(cls == ci)[0] for ci in range(4)]
        assert all(len(g) >= 100 for g in groups)
        for n in (len(labels), 4352):
            idx = np.array([groups[i % 4][(i // 4) % len(groups[i % 4])] for i in range(n)])
            for w in range(0, n - 63, 64):
                assert set(cls[idx[w:w + 64]].tolist()) == {0, 1, 2, 3}
            st = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
            _check(st, exp[idx], [labels[i] for i in idx], "n=%d" % n)


def _edge_key_vectors():
    """The edge vectors under the fixture's own key (not a golden key, not +-G)."""
    xy, e, r, s, exp, labels = prehashed_arrays("teeth_edges.json")
    sel = [i for i, l in enumerate(labels) if l.startswith("u2=")]
    assert len(sel) >= 100 and (xy[sel] == xy[sel[0]]).all()
    return xy[sel[0]], e[sel], r[sel], s[sel], exp[sel], [labels[i] for i in sel]


def test_queue_shapes(lib):
    """Above 4,096 items: no compact item while the context holds such a key;
    exactly one compact item per wave; compact items with r = 0, s = N,
    s = 2^256 - 1; an off-curve compact slot; a slot out of range."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays()
    kxy, ke, kr, ks, kexp, klabels = _edge_key_vectors()
    n = 66 * 64
    idx = np.arange(n) % len(labels)
    with Authenticator(0) as a:
        a.set_key_teeth(5)
        bad_xy = kxy.copy()
        bad_xy[63] ^= 1  # off the curve
        tf, tv = a.register_points(np.stack([kxy, bad_xy]))
        assert tv.tolist() == [1, 0]
        a.set_key_window(8)
        slots, valid = a.register_points(xy)
        assert valid.all()
        nslots = int(max(slots.max(), tf.max())) + 1
        be, br, bs, bsl, bexp = e[idx], r[idx], s[idx], slots[idx], exp[idx]
        # 1. the context holds a compact key, the batch has no such item
        _check(a.verify_prehashed(be, br, bs, bsl), bexp, labels, "none")
        # 2. exactly one compact item per wave, at a different lane each
        pos = np.array([64 * w + (7 * w + 3) % 64 for w in range(66)])
        pick = np.arange(66) % len(klabels)
        e1, r1, s1, sl1, exp1 = be.copy(), br.copy(), bs.copy(), bsl.copy(), bexp.copy()
        e1[pos], r1[pos], s1[pos], sl1[pos], exp1[pos] = ke[pick], kr[pick], ks[pick], tf[0], kexp[pick]
        assert exp1[pos].sum() >= 20
        _check(a.verify_prehashed(e1, r1, s1, sl1), exp1, labels, "one per wave")
        # 3. out-of-range r / s on compact items, the off-curve slot, a slot out of range
        e2, r2, s2, sl2 = e1.copy(), r1.copy(), s1.copy(), sl1.copy()
        want = np.where(exp1 == 1, 0, REJECT)
        acc = [int(p) for p, k in zip(pos, pick) if kexp[k] == 1]
        p0, p1, p2, p3, p4 = acc[:5]
        r2[p0] = 0
        s2[p1] = np.frombuffer(N.to_bytes(32, "big"), dtype=np.uint8)
        s2[p2] = 0xFF
        sl2[p3] = tf[1]
        sl2[p4] = nslots + 5
        want[[p0, p1, p2]] = REJECT
        want[[p3, p4]] = BAD_KEY
        st = a.verify_prehashed(e2, r2, s2, sl2)
        bad = np.nonzero(st != want)[0]
        assert not len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]]


def test_batches_in_flight(lib, golden):
    """Four back-to-back batches of ~5,000 items on one stream, no
    synchronize between the calls: window-8 and compact keys mixed."""
    import torch
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    dev = torch.device("cuda", 0)
    with Authenticator(0) as a:
        a.set_key_window(8)
        s8, _ = a.register_points(xy[: n // 3])
        a.set_key_teeth(4)
        s4, _ = a.register_points(xy[n // 3:])
        slots = np.concatenate([s8, s4])
        stream = torch.cuda.Stream(device=dev)
        batches = []
        for b in range(4):
            idx = (np.arange(4900 + 37 * b) * (b + 1) + 11 * b) % n  # a different order per batch
            d = [torch.from_numpy(np.ascontiguousarray(v[idx])).to(dev) for v in (e, r, s)]
            d.append(torch.from_numpy(slots[idx].astype(np.uint32).view(np.int32)).to(dev))
            d.append(torch.full((len(idx),), 0xAA, dtype=torch.uint8, device=dev))
            batches.append((idx, d))
        torch.cuda.synchronize()
        for idx, d in batches:  # (no synchronize inside this loop)
            a.verify_prehashed_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      len(idx), d[4].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        for b, (idx, d) in enumerate(batches):
            _check(d[4].cpu().numpy(), exp[idx], [labels[i] for i in idx], "batch %d" % b)


# ----------------------------------------------------------------- entry points
@pytest.fixture(scope="module")
def big_stream():
    from test_gpu_tablefree import _streams
    return _streams(1, 150, 0x7E01)  # 600 messages + the faults: the device message layer


@pytest.fixture(scope="module")
def small_stream():
    from test_gpu_tablefree import _streams
    return _streams(4, 6, 0x7E02)  # 60 messages + the faults: the small route


def _auth(keys):
    """Replica and USIG keys at window 8, client keys compact (t = 4)."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    a = Authenticator(0)
    for role in (o.ROLE_REPLICA, o.ROLE_USIG, o.ROLE_CLIENT):
        if role == o.ROLE_CLIENT:
            a.set_key_teeth(4)
        else:
            a.set_key_window(8)
        a.add_role(role)
        for id_, q in keys[role].items():
            a.set_public_key(role, id_, o.pkix_encode(q))
    a.enable_usig(True)
    return a


@pytest.mark.parametrize("resident", [0, 32])
def test_lone_calls(lib, monkeypatch, small_stream, resident):
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    from test_gpu_tablefree import _calls, _oracle_auth
    _fast_oracle(monkeypatch)
    n, msgs, keys = small_stream
    # requests first: the lone calls are mostly the compact client's
    calls = _calls(sorted(msgs, key=lambda m: m.type), random.Random(3), 24)
    rq = next(m for m in msgs if m.type == 1)  # a REQUEST: tampered message, tampered signature
    ab = o.msg_authen_bytes(rq)
    calls.append((o.ROLE_CLIENT, rq.client_id, ab[:9] + bytes([ab[9] ^ 1]) + ab[10:], rq.sig))
    calls.append((o.ROLE_CLIENT, rq.client_id, ab, rq.sig[:-1] + bytes([rq.sig[-1] ^ 1])))
    calls.append((o.ROLE_CLIENT, rq.client_id, ab, rq.sig))
    ref = _oracle_auth(keys)
    want = [ref.verify(*c) for c in calls]
    assert want[-3:] == [REJECT, REJECT, 0]
    a = _auth(keys)
    try:
        a.set_resident(resident)
        got = [a.verify_status(*c) for c in calls]
    finally:
        a.close()
    assert got == want


def test_batch_entry_points(lib, monkeypatch, big_stream):
    """verify_batch and the device-decoded compact flat form (pinned)."""
    from test_gpu_configs import _fast_oracle
    from test_gpu_tablefree import _calls, _oracle_auth
    _fast_oracle(monkeypatch)
    n, msgs, keys = big_stream
    calls = _calls(msgs, random.Random(4), 400)
    ref = _oracle_auth(keys)
    want = [ref.verify(*c) for c in calls]
    for form in ("batch", "flat32"):
        a = _auth(keys)
        try:
            got = a.verify_batch(calls) if form == "batch" else a.verify_batch_flat32(calls, pinned=True)
        finally:
            a.close()
        assert [int(g) for g in got] == want, form


@pytest.mark.parametrize("size", ["device_layer", "small_route"])
def test_message_layer(lib, monkeypatch, big_stream, small_stream, size):
    """validate_messages_flat and check_messages_flat + resolve over 600
    messages (the device message layer) and over 64 (the small route)."""
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    from test_gpu_small_check import _packed
    from test_gpu_tablefree import _oracle_auth
    _fast_oracle(monkeypatch)
    n, msgs, keys = big_stream if size == "device_layer" else small_stream
    assert (len(msgs) > 512) == (size == "device_layer")
    assert {m.type for m in msgs} >= {o.MSG_REQUEST, o.MSG_PREPARE, o.MSG_COMMIT}
    want = np.array(o.validate_messages(_oracle_auth(keys), msgs, n, 0))
    assert (want != 0).sum() >= 3
    a = _auth(keys)
    try:
        got = a.validate_messages_via_flat(msgs, n, 0)
    finally:
        a.close()
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    want_ns = np.array(o.validate_messages(_oracle_auth(keys), msgs, n, 3))  # (no stream stop)
    a = _auth(keys)
    try:
        recs, arena = _packed(a, msgs)
        with a.check_messages_flat(recs, arena, n) as b:
            got = np.array([b.resolve(j) for j in range(len(msgs))])
    finally:
        a.close()
    assert (got == want_ns).all(), np.nonzero(got != want_ns)[0][:10]


def test_two_engines(lib, golden):
    from minbft_amd.authenticator import Authenticator
    from test_gpu_multi import _extra_devices
    xy, e, r, s, exp, labels = golden
    reps = 4096 // len(labels) + 1
    with Authenticator(0) as a:
        a.set_key_teeth(4)
        s1, _ = a.register_points(xy[:300])          # replayed on the engine added below
        a.set_key_teeth(7)
        s2, _ = a.register_points(xy[300:500])       # (a second run of another class to replay)
        a.add_device(_extra_devices(1)[0])
        assert a.key_teeth() == 7
        s3, _ = a.register_points(xy[500:])          # registered on both at once
        slots = np.concatenate([s1, s2, s3])
        te, tr, ts, tsl, texp = _tile([e, r, s, slots, exp], reps)
        one = a.verify_prehashed(te, tr, ts, tsl)    # (below the default shard size: one engine)
        a.set_shard_min(512)
        two = a.verify_prehashed(te, tr, ts, tsl)
    _check(two, texp, labels)
    assert (one == two).all()


# -------------------------------------------------------------------- key store
def test_teeth_and_refusals(lib):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    with Authenticator(0) as a:
        g0, q0 = a.windows()
        assert a.key_teeth() == 0
        for t in (0, 1, 9, -1):
            assert a.lib.mbft_set_key_teeth(a.ctx, t) == _lib.ERR_ARG
        assert a.key_teeth() == 0 and a.windows() == (g0, q0)
        a.set_key_teeth(_lib.TEETH_MIN)
        assert a.key_teeth() == 2 and a.windows() == (g0, 0)
        a.set_key_teeth(_lib.TEETH_MAX)
        assert a.key_teeth() == 8 and a.windows() == (g0, 0)
        for w in (1, 2, 3, 30, -1):  # the window's own range is what it was
            assert a.lib.mbft_set_key_window(a.ctx, w) == _lib.ERR_ARG
        assert a.key_teeth() == 8
        a.set_key_window(_lib.WINDOW_NONE)
        assert a.key_teeth() == 0 and a.windows() == (g0, 0)
        a.set_key_teeth(4)
        assert a.key_teeth() == 4 and a.windows() == (g0, 0)
        a.set_key_window(4)
        assert a.key_teeth() == 0 and a.windows() == (g0, 4)


def test_clear_and_reregister(lib, golden):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    with Authenticator(0) as a:
        for kind, v in (("t", 4), ("w", 8), ("t", 4)):
            (a.set_key_teeth if kind == "t" else a.set_key_window)(v)
            slots, valid = a.register_points(xy)
            assert valid.all()
            _check(a.verify_prehashed(e, r, s, slots), exp, labels, "%s %d" % (kind, v))
            a.clear_keys()


def test_many_keys(lib):
    """20,000 distinct points registered at t = 4 in one call and 300 one by
    one; a signature under each verifies, a tampered one does not.  Key i is
    (i + 2) G and the signature is crafted without its discrete log in hand:
    R = u1 G + u2 Q = (u1 + u2 (i + 2)) G for chosen u1, u2 (the construction
    of test_gpu_tablefree.test_many_keys, u2 spread over the whole range so
    that every column of the comb is used)."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    count, lone = 20000, 300
    pts, p = [], o.point_add(o.G, o.G)
    for _ in range(count + lone):
        pts.append(p)
        p = o.point_add(p, o.G)
    xy = np.array([list(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")) for q in pts], dtype=np.uint8)
    cyc = [o.scalar_mult(k, o.G) for k in range(1, 40)]
    rng = random.Random(0x4ee7)
    e, r, s = (np.zeros((count + lone, 32), dtype=np.uint8) for _ in range(3))
    for i in range(count + lone):
        d, u2 = i + 2, rng.randrange(1, N)
        t = 1 + i % 39                       # R = t G with t = u1 + u2 d (mod N)
        u1 = (t - u2 * d) % N
        rr = cyc[t - 1][0] % N
        ss = rr * pow(u2, -1, N) % N
        e[i] = np.frombuffer((u1 * ss % N).to_bytes(32, "big"), dtype=np.uint8)
        r[i] = np.frombuffer(rr.to_bytes(32, "big"), dtype=np.uint8)
        s[i] = np.frombuffer(ss.to_bytes(32, "big"), dtype=np.uint8)
    for i in (0, 1, count - 1, count, count + lone - 1):  # the construction itself, against the oracle
        assert o.go_ecdsa_verify(pts[i], bytes(e[i]), int.from_bytes(bytes(r[i]), "big"),
                                 int.from_bytes(bytes(s[i]), "big"))
    bad_e = e.copy()
    bad_e[:, 31] ^= 1
    with Authenticator(0) as a:
        a.set_key_teeth(4)
        slots, valid = a.register_points(xy[:count])
        assert valid.all() and len(set(slots.tolist())) == count
        ones = []
        for i in range(count, count + lone):
            sl, v = a.register_points(xy[i:i + 1])
            assert v.all()
            ones.append(int(sl[0]))
        slots = np.concatenate([slots, np.array(ones, dtype=slots.dtype)])
        assert len(set(slots.tolist())) == count + lone
        st = a.verify_prehashed(e, r, s, slots)
        assert (st == 0).all(), np.nonzero(st)[0][:10]
        st = a.verify_prehashed(bad_e[-2000:], r[-2000:], s[-2000:], slots[-2000:])
        assert (st == REJECT).all()
