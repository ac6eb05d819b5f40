"""Table-free keys (key window 0, MBFT_WINDOW_NONE): a key whose whole device
state is its point, verified by the double-and-add ladder
(minbft_amd/csrc/ladder_dev.h) instead of a comb -- through the C-ABI, against
the golden expectations and the oracle.

* the prehashed golden set and tests/golden/ladder_edges.json (vectors
  crafted from chosen (u1, u2): the recoding's degenerate scalar N - 2, the
  corners, Q = +-G joins) with every key at window 0, on each small-batch form
  and, tiled past 4,096 items, through k_verify, the second compacted queue
  and k_verify_ladder;
* windows 8 and 0 side by side; the queue's shapes (empty, full, one item per
  wave, out-of-range r / s, an off-curve slot, a slot out of range);
* four batches in flight on one stream (the queue is per pipeline buffer);
* every entry point against the oracle with table-free client keys: lone
  calls (resident verifier off and on), verify_batch, the device-decoded flat
  form, the message layer's device and small routes;
* two engines; the key store (windows(), refused windows, clear and
  re-register, 20,000 keys in one call, 300 one by one).
"""
import hashlib
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays

pytestmark = pytest.mark.gpu

REJECT, BAD_KEY = 1, 5
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


@pytest.fixture(scope="module")
def golden():
    """prehashed.json (551 vectors) + ladder_edges.json, as one set."""
    a, b = prehashed_arrays(), prehashed_arrays("ladder_edges.json")
    assert len(a[5]) == 551 and len(b[5]) >= 200
    xy, e, r, s, exp = (np.concatenate([a[k], b[k]]) for k in range(5))
    return xy, e, r, s, exp, a[5] + b[5]


def _check(st, exp, labels, what=""):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i % len(labels)], i, int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, len(bad), bad[:10])
    assert set(np.unique(st).tolist()) <= {0, REJECT}, what


def _tile(arrs, reps):
    return [np.concatenate([a] * reps) for a in arrs]


@pytest.mark.parametrize("form", ["one_batch", "default", "split", "pairs", "pairs_lane_inv", "quads",
                                  "quads_planes"])
def test_golden_small_forms(lib, golden, form):
    """Every key table-free, below 4,096 items: as one batch, and in batches of
    <= 200 under each small-batch setting of test_prehashed_golden_small_batches."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    with Authenticator(0) as a:
        if form not in ("one_batch", "default"):
            a.set_small_batch_form(256 if form == "split" else 0)
            a.set_small_batch_inverse({"pairs_lane_inv": 0, "quads": 2, "quads_planes": 3}.get(form, 1))
        a.set_key_window(0)
        assert a.windows()[1] == 0
        slots, valid = a.register_points(xy)
        assert valid.all()
        step = len(labels) if form == "one_batch" else 200
        st = np.concatenate([a.verify_prehashed(e[k:k + step], r[k:k + step], s[k:k + step], slots[k:k + step])
                             for k in range(0, len(labels), step)])
    _check(st, exp, labels, form)


def test_golden_large_path(lib, golden):
    """Tiled just past 4,096 items: k_verify queues every item, k_verify_ladder
    serves the queue; every copy equals the golden expectation."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    reps = 4096 // len(labels) + 1
    with Authenticator(0) as a:
        a.set_key_window(0)
        slots, valid = a.register_points(xy)
        assert valid.all()
        te, tr, ts, tsl, texp = _tile([e, r, s, slots, exp], reps)
        assert len(texp) > 4096
        st = a.verify_prehashed(te, tr, ts, tsl)
    _check(st, texp, labels)


def test_mixed_windows(lib, golden):
    """Half the keys at window 8, half table-free, in one context: below and
    above 4,096 items."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    order = np.random.default_rng(5).permutation(n)  # (both files' keys in both halves)
    xy, e, r, s, exp = (v[order] for v in (xy, e, r, s, exp))
    labels = [labels[i] for i in order]
    with Authenticator(0) as a:
        a.set_key_window(8)
        s8, v8 = a.register_points(xy[: n // 2])
        a.set_key_window(0)
        s0, v0 = a.register_points(xy[n // 2:])
        assert v8.all() and v0.all() and a.windows()[1] == 0
        slots = np.concatenate([s8, s0])
        _check(a.verify_prehashed(e, r, s, slots), exp, labels, "small")
        te, tr, ts, tsl, texp = _tile([e, r, s, slots, exp], 4096 // n + 1)
        _check(a.verify_prehashed(te, tr, ts, tsl), texp, labels, "large")


def _edge_key_vectors():
    """The edge vectors under the fixture's own key (not a golden key, not +-G)."""
    xy, e, r, s, exp, labels = prehashed_arrays("ladder_edges.json")
    sel = [i for i, l in enumerate(labels) if l.startswith("u2=")]
    assert len(sel) >= 100 and (xy[sel] == xy[sel[0]]).all()
    return xy[sel[0]], e[sel], r[sel], s[sel], exp[sel], [labels[i] for i in sel]


def test_queue_shapes(lib):
    """Above 4,096 items: no table-free item while the context holds such a
    key; exactly one table-free item per wave; table-free items with r = 0,
    s = N, s = 2^256 - 1; an off-curve table-free slot; a slot out of range."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays()
    kxy, ke, kr, ks, kexp, klabels = _edge_key_vectors()
    n = 66 * 64
    idx = np.arange(n) % len(labels)
    with Authenticator(0) as a:
        a.set_key_window(0)
        bad_xy = kxy.copy()
        bad_xy[63] ^= 1  # off the curve
        tf, tv = a.register_points(np.stack([kxy, bad_xy]))
        assert tv.tolist() == [1, 0]
        a.set_key_window(8)
        slots, valid = a.register_points(xy)
        assert valid.all()
        nslots = int(max(slots.max(), tf.max())) + 1
        be, br, bs, bsl, bexp = e[idx], r[idx], s[idx], slots[idx], exp[idx]
        # 1. the context holds a table-free key, the batch has no such item
        _check(a.verify_prehashed(be, br, bs, bsl), bexp, labels, "none")
        # 2. exactly one table-free item per wave, at a different lane each
        pos = np.array([64 * w + (7 * w + 3) % 64 for w in range(66)])
        pick = np.arange(66) % len(klabels)
        e1, r1, s1, sl1, exp1 = be.copy(), br.copy(), bs.copy(), bsl.copy(), bexp.copy()
        e1[pos], r1[pos], s1[pos], sl1[pos], exp1[pos] = ke[pick], kr[pick], ks[pick], tf[0], kexp[pick]
        assert exp1[pos].sum() >= 20
        _check(a.verify_prehashed(e1, r1, s1, sl1), exp1, labels, "one per wave")
        # 3. out-of-range r / s on table-free items, the off-curve slot, a slot out of range
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
    synchronize between the calls: each batch's table-free queue is its own
    (the queue lives in the pipeline buffer, of which verify_device rotates
    three)."""
    import torch
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    dev = torch.device("cuda", 0)
    with Authenticator(0) as a:
        a.set_key_window(8)
        s8, _ = a.register_points(xy[: n // 3])
        a.set_key_window(0)
        s0, _ = a.register_points(xy[n // 3:])
        slots = np.concatenate([s8, s0])
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
def _streams(f, nreq, seed):
    from oracle import p256 as o
    from test_gpu_configs import _c3_streams
    n, msgs, keys = _c3_streams(f, nreq, random.Random(seed), True)
    rd = int.from_bytes(hashlib.sha256(b"tablefree replica").digest(), "big") % (o.N - 1) + 1
    keys[o.ROLE_REPLICA] = {0: o.pubkey(rd)}
    return n, msgs, keys


@pytest.fixture(scope="module")
def big_stream():
    return _streams(1, 150, 0x7F01)  # 600 messages + the faults: the device message layer


@pytest.fixture(scope="module")
def small_stream():
    return _streams(4, 6, 0x7F02)  # 60 messages + the faults: the small route


def _auth(keys):
    """Replica and USIG keys at window 8, client keys table-free."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    a = Authenticator(0)
    for role, w in ((o.ROLE_REPLICA, 8), (o.ROLE_USIG, 8), (o.ROLE_CLIENT, 0)):
        a.set_key_window(w)
        a.add_role(role)
        for id_, q in keys[role].items():
            a.set_public_key(role, id_, o.pkix_encode(q))
    a.enable_usig(True)
    return a


def _oracle_auth(keys):
    from oracle import p256 as o
    ks = o.KeyStore()
    ks.keys = {role: dict(m) for role, m in keys.items()}
    return o.Authenticator(ks)


def _calls(msgs, rng, limit):
    """VerifyMessageAuthenTag calls of a stream's messages (REQUEST: the
    client's signature; PREPARE / COMMIT: the USIG's UI), some tampered, some
    under an unknown client."""
    from oracle import p256 as o
    calls = []
    for m in msgs:
        if len(calls) >= limit:
            break
        if m.type == o.MSG_REQUEST:
            c = (o.ROLE_CLIENT, m.client_id, o.msg_authen_bytes(m), m.sig)
        elif m.type in (o.MSG_PREPARE, o.MSG_COMMIT):
            c = (o.ROLE_USIG, m.replica_id, o.msg_authen_bytes(m), o.ui_marshal(m.ui_counter, m.ui_cert))
        else:
            continue
        k = rng.randrange(6)
        if k == 0:
            b = bytearray(c[2])
            b[rng.randrange(len(b))] ^= 1
            c = (c[0], c[1], bytes(b), c[3])
        elif k == 1 and c[0] == o.ROLE_CLIENT:
            c = (c[0], 99, c[2], c[3])
        calls.append(c)
    assert sum(c[0] == o.ROLE_CLIENT for c in calls) >= 4
    return calls


@pytest.mark.parametrize("resident", [0, 32])
def test_lone_calls(lib, monkeypatch, small_stream, resident):
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    _fast_oracle(monkeypatch)
    n, msgs, keys = small_stream
    # requests first: the lone calls are mostly the table-free client's
    calls = _calls(sorted(msgs, key=lambda m: m.type), random.Random(3), 24)
    rq = next(m for m in msgs if m.type == 1)  # a REQUEST: tampered message, tampered signature
    ab = o.msg_authen_bytes(rq)
    calls.append((o.ROLE_CLIENT, rq.client_id, ab[:9] + bytes([ab[9] ^ 1]) + ab[10:], rq.sig))  # (e: the first 32 bytes)
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
    _fast_oracle(monkeypatch)
    n, msgs, keys = big_stream
    calls = _calls(msgs, random.Random(4), 400)
    for form in ("batch", "flat32"):
        ref = _oracle_auth(keys)
        want = [ref.verify(*c) for c in calls]
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
        a.set_key_window(0)
        s1, _ = a.register_points(xy[:300])          # replayed on the engine added below
        a.add_device(_extra_devices(1)[0])
        s2, _ = a.register_points(xy[300:])          # registered on both at once
        slots = np.concatenate([s1, s2])
        te, tr, ts, tsl, texp = _tile([e, r, s, slots, exp], reps)
        one = a.verify_prehashed(te, tr, ts, tsl)    # (below the default shard size: one engine)
        a.set_shard_min(512)
        two = a.verify_prehashed(te, tr, ts, tsl)
    _check(two, texp, labels)
    assert (one == two).all()


# -------------------------------------------------------------------- key store
def test_windows_and_refusals(lib):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    with Authenticator(0) as a:
        g0 = a.windows()[0]
        a.set_key_window(_lib.WINDOW_NONE)
        assert a.windows() == (g0, 0)
        for w in (1, 2, 3, 30, -1):
            assert a.lib.mbft_set_key_window(a.ctx, w) == _lib.ERR_ARG
        assert a.lib.mbft_set_generator_window(a.ctx, 0) == _lib.ERR_ARG
        assert a.lib.mbft_set_generator_window(a.ctx, 3) == _lib.ERR_ARG
        assert a.windows() == (g0, 0)
        a.set_key_window(4)
        assert a.windows() == (g0, 4)


def test_clear_and_reregister(lib, golden):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    with Authenticator(0) as a:
        for w in (0, 8, 0):
            a.set_key_window(w)
            slots, valid = a.register_points(xy)
            assert valid.all()
            _check(a.verify_prehashed(e, r, s, slots), exp, labels, "window %d" % w)
            a.clear_keys()


def test_many_keys(lib):
    """20,000 distinct points registered at window 0 in one call and 300 one by
    one; a signature under each verifies, a tampered one does not.  Key i is
    (i + 2) G and the signature is crafted without its discrete log in hand:
    R = u1 G + u2 Q = (u1 + u2 (i + 2)) G for chosen u1, u2."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    count, lone = 20000, 300
    pts, p = [], o.point_add(o.G, o.G)
    for _ in range(count + lone):
        pts.append(p)
        p = o.point_add(p, o.G)
    xy = np.array([list(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")) for q in pts], dtype=np.uint8)
    # one (u1, u2) pair per key from a short cycle of multiples of G
    cyc = [o.scalar_mult(k, o.G) for k in range(1, 40)]
    e, r, s = (np.zeros((count + lone, 32), dtype=np.uint8) for _ in range(3))
    for i in range(count + lone):
        d, u2 = i + 2, 1 + i % 3
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
        a.set_key_window(0)
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
