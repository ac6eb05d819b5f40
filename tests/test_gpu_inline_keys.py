"""The inline-key class (mbft_verify_prehashed_keys, _keys_device,
mbft_scheme_verify_flat32): signatures verified under keys
that arrive with the call -- validated on the GPU by k_verify_keys, used by the
table-free keys' ladder, nothing registered -- through the C-ABI, against the
golden expectations and the oracle.

* the three golden sets with each vector's own key inline, host and device form;
* both s^-1 sources (the lane's own up to 4,096 items, the batch's planes
  above) and every guard: sizes around the wave, the block and the threshold,
  with a poisoned status tail;
* key validation per lane (off the curve, (0, 0), coordinates >= p, a point
  that satisfies the equation only mod p) and its precedence over the range
  check, one wave holding valid, bad-key and out-of-range lanes;
* byte-for-byte equivalence with registration at key window 0;
* no state: a context with no key at all; slots, key memory, use counts and
  the verified-call memo untouched around an inline batch;
* generator windows 4, 8 and 16; four batches in flight on one stream;
* the scheme form (the host's DER decode and quirk digest in front).
"""
import hashlib

import numpy as np
import pytest

from golden_util import load, prehashed_arrays

pytestmark = pytest.mark.gpu

ACCEPT, REJECT, MALFORMED_DER, BAD_KEY = 0, 1, 2, 5
POISON = 0xEE


def _b32(x):
    return np.frombuffer(int(x).to_bytes(32, "big"), dtype=np.uint8)


def _xy64(x, y):
    return np.concatenate([_b32(x), _b32(y)])


def _int(a):
    return int.from_bytes(bytes(a), "big")


@pytest.fixture(scope="module")
def golden():
    """prehashed.json (551) + ladder_edges.json (262) + scalar_edges.json (54)."""
    sets = [prehashed_arrays(), prehashed_arrays("ladder_edges.json"), prehashed_arrays("scalar_edges.json")]
    assert [len(v[5]) for v in sets] == [551, 262, 54]
    xy, e, r, s, exp = (np.concatenate([v[k] for v in sets]) for k in range(5))
    return xy, e, r, s, exp, sum((v[5] for v in sets), [])


@pytest.fixture(scope="module")
def auth(lib):
    """A context that never holds a key."""
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    yield a
    a.close()


def _host(a, e, r, s, xy):
    """The host form into a status buffer 256 bytes longer, pre-filled."""
    import ctypes
    n = len(e)
    e, r, s, xy = (np.ascontiguousarray(v, dtype=np.uint8) for v in (e, r, s, xy))
    out = np.full(n + 256, POISON, dtype=np.uint8)
    rc = a.lib.mbft_verify_prehashed_keys(a.ctx, *(ctypes.c_void_p(v.ctypes.data) for v in (e, r, s, xy)), n,
                                          ctypes.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    assert (out[n:] == POISON).all() and (out[:n] != POISON).all()
    return out[:n].copy()


def _to_device(e, r, s, xy):
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.array(v, dtype=np.uint8)).to(dev) for v in (e, r, s, xy)]
    d.append(torch.full((len(e) + 256,), POISON, dtype=torch.uint8, device=dev))
    return d


def _device_status(d, n):
    out = d[4].cpu().numpy()
    assert (out[n:] == POISON).all() and (out[:n] != POISON).all()
    return out[:n].copy()


def _device(a, e, r, s, xy):
    """The device form on a stream of the caller's, the same poisoned tail."""
    import torch
    n = len(e)
    d = _to_device(e, r, s, xy)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.verify_prehashed_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n,
                                   d[4].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return _device_status(d, n)


def _both(a, e, r, s, xy):
    h, d = _host(a, e, r, s, xy), _device(a, e, r, s, xy)
    assert (h == d).all(), np.nonzero(h != d)[0][:10]
    return h


def _same(st, want, what=""):
    bad = np.nonzero(np.asarray(st) != np.asarray(want))[0]
    assert not len(bad), (what, len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]])


# ------------------------------------------------------------------ 1. golden
def test_golden_sets_inline(auth, golden):
    """Every vector of the three sets under its own key, given inline: the
    fixture's expectation, the oracle's verdict, host and device form."""
    from oracle import p256 as o
    xy, e, r, s, exp, labels = golden
    want = np.where(exp == 1, ACCEPT, REJECT)
    for i in range(len(labels)):
        q = (_int(xy[i, :32]), _int(xy[i, 32:]))
        assert o.on_curve(*q), labels[i]
        assert o.go_ecdsa_verify(q, bytes(e[i]), _int(r[i]), _int(s[i])) == bool(exp[i]), labels[i]
    assert 100 < int(exp.sum()) < len(exp) - 100
    _same(_host(auth, e, r, s, xy), want, "host")
    _same(_device(auth, e, r, s, xy), want, "device")
    # the host binding of the same call
    _same(auth.verify_prehashed_keys(e, r, s, xy), want, "binding")


# ------------------------------------------------- 2. s^-1 sources and guards
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4096, 4097, 5510])
def test_sizes_and_guards(auth, golden, n):
    """The 867 vectors tiled or cut to n: 4,097 and 5,510 read s^-1 from the
    batch's planes, the others invert in the lane.  Nothing past n is written,
    everything before it is."""
    xy, e, r, s, exp, _ = golden
    idx = np.arange(n) % len(exp)
    want = np.where(exp[idx] == 1, ACCEPT, REJECT)
    _same(_both(auth, e[idx], r[idx], s[idx], xy[idx]), want, n)


def test_empty_and_null(auth):
    import ctypes
    one = np.zeros(64, dtype=np.uint8)
    p = ctypes.c_void_p(one.ctypes.data)
    lib, ctx = auth.lib, auth.ctx
    assert lib.mbft_verify_prehashed_keys(ctx, None, None, None, None, 0, None) == 0
    assert lib.mbft_verify_prehashed_keys_device(ctx, None, None, None, None, 0, None, None) == 0
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert lib.mbft_verify_prehashed_keys(ctx, *args[:4], 1, args[4]) == -1
        assert lib.mbft_verify_prehashed_keys_device(ctx, *args[:4], 1, args[4], None) == -1
    assert lib.mbft_verify_prehashed_keys(None, p, p, p, p, 1, p) == -1


# ---------------------------------------------------------- 3. key validation
def _equation_only_mod_p():
    """(p + k, y) for the smallest k >= 0 with k^3 - 3 k + b a square mod p: (k, y)
    is on the curve, (p + k, y) satisfies the equation mod p and is no key."""
    from oracle import p256 as o
    k = 0
    while True:
        a = (k * k * k - 3 * k + o.B) % o.P
        y = pow(a, (o.P + 1) // 4, o.P)
        if y * y % o.P == a:
            assert o.on_curve(k, y) and o.P + k < 1 << 256
            return o.P + k, y
        k += 1


@pytest.fixture(scope="module")
def crafted():
    """A 64-item group in which valid, bad-key and out-of-range lanes
    alternate, with the oracle's statuses."""
    from oracle import p256 as o
    keys = [(d, o.pubkey(d)) for d in (0x1D0C5EED, 0xA11CE << 64 | 7, o.N - 12345)]
    sigs = []
    for j in range(22):
        d, q = keys[j % 3]
        h = hashlib.sha256(b"inline %d" % j).digest()
        rr, ss = o.ecdsa_sign(d, h)
        sigs.append((q, h, rr, ss))
    qx, qy = keys[0][1]
    xp, yp = _equation_only_mod_p()
    bad_points = [(qx, (qy + 1) % o.P), (0, 0), (o.P, qy), (qx, o.P), (qx, (1 << 256) - 1), (xp, yp)]
    assert not any(o.on_curve(x, y) for x, y in bad_points)
    assert (yp * yp - (xp ** 3 - 3 * xp + o.B)) % o.P == 0  # the range check stands on its own
    out_of_range = [(0, None), (None, 0), (o.N, None), (None, o.N), ((1 << 256) - 1, None), (None, o.N + 1)]
    items, want, kinds = [], [], []
    for lane in range(64):
        q, h, rr, ss = sigs[lane // 3]
        kind = lane % 3
        if kind == 1:  # a bad key; every other one also with r or s out of range: BAD_KEY wins
            q = bad_points[(lane // 3) % len(bad_points)]
            if (lane // 3) % 2:
                rr = 0 if lane % 2 else rr
                ss = ss if lane % 2 else o.N
        elif kind == 2:  # a good key, r or s outside [1, N)
            nr, ns = out_of_range[(lane // 3) % len(out_of_range)]
            rr, ss = (rr if nr is None else nr), (ss if ns is None else ns)
        if lane == 63:  # one more valid lane: a tampered digest
            h = hashlib.sha256(b"other").digest()
        items.append((q, h, rr, ss))
        if not (q[0] < o.P and q[1] < o.P and o.on_curve(*q)):
            want.append(BAD_KEY)
        else:
            want.append(ACCEPT if o.go_ecdsa_verify(q, h, rr, ss) else REJECT)
        kinds.append(kind)
    want = np.array(want, dtype=np.uint8)
    kinds = np.array(kinds)
    assert (want[kinds == 1] == BAD_KEY).all() and (want[kinds == 2] == REJECT).all()
    assert (want[kinds == 0][:-1] == ACCEPT).all() and want[63] == REJECT
    xy = np.stack([_xy64(*it[0]) for it in items])
    e = np.stack([np.frombuffer(it[1], dtype=np.uint8) for it in items])
    r = np.stack([_b32(it[2]) for it in items])
    s = np.stack([_b32(it[3]) for it in items])
    return xy, e, r, s, want, bad_points, sigs


def test_key_validation_per_lane(auth, crafted):
    from oracle import p256 as o
    xy, e, r, s, want, bad_points, sigs = crafted
    q, h, rr, ss = sigs[0]
    he = np.frombuffer(h, dtype=np.uint8)
    # each bad point on its own under a valid signature, then with r = 0
    for x, y in bad_points:
        for r1 in (rr, 0):
            st = _both(auth, he[None], _b32(r1)[None], _b32(ss)[None], _xy64(x, y)[None])
            assert st.tolist() == [BAD_KEY], (hex(x), hex(y), r1)
    # a good key with r = 0, s = 0, r = N, s = N
    for r1, s1 in ((0, ss), (rr, 0), (o.N, ss), (rr, o.N)):
        st = _both(auth, he[None], _b32(r1)[None], _b32(s1)[None], _xy64(*q)[None])
        assert st.tolist() == [REJECT], (r1, s1)
    assert _both(auth, he[None], _b32(rr)[None], _b32(ss)[None], _xy64(*q)[None]).tolist() == [ACCEPT]
    # one wave holding all three kinds; 65 of them for the planes path
    _same(_both(auth, e, r, s, xy), want, "64")
    t = [np.concatenate([v] * 65) for v in (e, r, s, xy, want)]
    assert len(t[4]) == 4160
    _same(_both(auth, t[0], t[1], t[2], t[3]), t[4], "4160")


# ------------------------------------------------ 4. the same as registration
def test_equals_registration(auth, golden, crafted):
    """The same points registered table-free on a second context, the invalid
    ones included: mbft_verify_prehashed answers byte for byte what the inline
    form answers."""
    from minbft_amd.authenticator import Authenticator
    gxy, ge, gr, gs, _, _ = golden
    cxy, ce, cr, cs, cwant, _, _ = crafted
    t = [np.concatenate([v] * 65) for v in (ce, cr, cs, cxy)]
    with Authenticator(0) as b:
        b.set_key_window(0)
        for e, r, s, xy, what in ((ce, cr, cs, cxy, "crafted"), (t[0], t[1], t[2], t[3], "crafted x 65"),
                                  (ge, gr, gs, gxy, "golden")):
            slots, valid = b.register_points(xy)
            inline = _both(auth, e, r, s, xy)
            assert ((inline == BAD_KEY) == (valid == 0)).all(), what
            _same(b.verify_prehashed(e, r, s, slots), inline, what)
    assert (cwant == BAD_KEY).sum() >= 20


# ------------------------------------------------------------------ 5. no state
def test_context_without_keys(lib, golden):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, _ = golden
    want = np.where(exp == 1, ACCEPT, REJECT)
    with Authenticator(0) as a:
        _same(_host(a, e[:300], r[:300], s[:300], xy[:300]), want[:300], "host")
        _same(_device(a, e[:300], r[:300], s[:300], xy[:300]), want[:300], "device")
        assert a.key_memory()[0] == 0


def test_leaves_the_key_store_alone(lib, golden):
    """Registered keys of three classes, accounting on, a memo set: an inline
    batch of 5,510 items changes none of it."""
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    xy, e, r, s, exp, _ = golden
    distinct = []
    for i in range(len(exp)):
        if not any((xy[i] == xy[j]).all() for j in distinct):
            distinct.append(i)
        if len(distinct) == 3:
            break
    own = np.array([i for i in range(len(exp)) if any((xy[i] == xy[j]).all() for j in distinct)])
    idx = np.arange(5510) % len(exp)
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        for cid, (j, select) in enumerate(zip(distinct, (lambda: a.set_key_window(8), lambda: a.set_key_window(0),
                                                         lambda: a.set_key_signed_teeth(5)))):
            select()
            a.set_public_key(ROLE_CLIENT, cid, bytes(xy[j]))
        a.set_key_accounting(True)
        a.set_verified_memo(1 << 20)
        slot_of = {bytes(xy[j]): a.key_slot(ROLE_CLIENT, cid) for cid, j in enumerate(distinct)}
        assert len(set(slot_of.values())) == 3
        slots = np.array([slot_of[bytes(xy[i])] for i in own], dtype=np.uint32)
        before = a.verify_prehashed(e[own], r[own], s[own], slots)
        _same(before, np.where(exp[own] == 1, ACCEPT, REJECT), "registered, before")

        def state():
            return (a.key_memory(), [v.tolist() for v in a.key_usage(n=8)], a.verified_memo_stats(),
                    [a.key_slot(ROLE_CLIENT, cid) for cid in range(3)], a.windows(), a.verified_memo())

        st0 = state()
        assert sum(st0[1][0]) > 0 and st0[5] > 0  # the counts are live, a memo is set
        want = np.where(exp[idx] == 1, ACCEPT, REJECT)
        _same(_both(a, e[idx], r[idx], s[idx], xy[idx]), want, "inline")
        assert state() == st0
        _same(a.verify_prehashed(e[own], r[own], s[own], slots), before, "registered, after")


# ---------------------------------------------------------- 6. generator windows
@pytest.mark.parametrize("wg", [4, 8, 16])
def test_generator_windows(lib, wg):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, _ = prehashed_arrays("ladder_edges.json")
    with Authenticator(0) as a:
        a.set_generator_window(wg)
        assert a.windows()[0] == wg
        _same(_both(a, e, r, s, xy), np.where(exp == 1, ACCEPT, REJECT), wg)


# ------------------------------------------------------------ 7. batches in flight
def test_batches_in_flight(auth, golden):
    """Four back-to-back device calls of 5,510 items on one caller stream, no
    synchronize between them: each takes its own buffer of the rotation."""
    import torch
    xy, e, r, s, exp, _ = golden
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    batches = []
    for b in range(4):
        idx = (np.arange(5510) + 211 * b + 5) % len(exp)  # a different rotation of the tiling per batch
        batches.append((idx, _to_device(e[idx], r[idx], s[idx], xy[idx])))
    torch.cuda.synchronize()
    for idx, d in batches:  # (no synchronize inside this loop)
        auth.verify_prehashed_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                          len(idx), d[4].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for b, (idx, d) in enumerate(batches):
        _same(_device_status(d, len(idx)), np.where(exp[idx] == 1, ACCEPT, REJECT), "batch %d" % b)


# ------------------------------------------------------------- 8. the scheme form
@pytest.fixture(scope="module")
def scheme_calls():
    """Calls (msg, tag, xy64, key id or None) with the oracle's statuses."""
    from oracle import p256 as o
    keys = [(d, o.pubkey(d)) for d in (0x5C4E3E, o.N - 99, 0xB0B << 100 | 3)]
    bad_xy = bytes(_xy64(keys[0][1][0], (keys[0][1][1] + 1) % o.P))
    memo = {}

    def expect(msg, tag, xy):
        try:
            rr, ss, _ = o.der_parse_sig(tag)
        except o.Asn1Error:
            return MALFORMED_DER
        x, y = _int(xy[:32]), _int(xy[32:])
        if not (x < o.P and y < o.P and o.on_curve(x, y)):
            return BAD_KEY
        k = (x, y, o.quirk_digest(msg)[:32], rr, ss)
        if k not in memo:
            memo[k] = ACCEPT if o.go_ecdsa_verify((x, y), o.quirk_digest(msg), rr, ss) else REJECT
        return memo[k]

    calls, what = [], []

    def add(kind, msg, tag, xy, kid):
        calls.append((bytes(msg), bytes(tag), bytes(xy), kid))
        what.append(kind)

    malformed = [bytes.fromhex(v["sig"]) for v in load("der.json") if v["ok"] == 0]
    wellformed = [bytes.fromhex(v["sig"]) for v in load("der.json") if v["ok"] == 1]
    assert len(malformed) >= 100
    msgs = [o.authen_request(7, b"op"), o.authen_request(1 << 40, bytes(range(200))), o.authen_req_view_change(3), b"",
            o.authen_reply(5, 9, b"result"), b"x" * 31, b"y" * 32, b"z" * 33, o.authen_prepare(1, 2, 3, b"op"),
            o.authen_commit(0, 1, 2, 3, b"op", 4), b"REQUEST", o.authen_req_view_change(1 << 63)]
    assert len(msgs[2]) == 23
    for j, msg in enumerate(msgs):
        kid = j % 3
        d, q = keys[kid]
        xy = bytes(_xy64(*q))
        rr, ss = o.ecdsa_sign(d, o.quirk_digest(msg))
        tag = o.der_encode_sig(rr, ss)
        add("valid", msg, tag, xy, kid)
        add("high-s", msg, o.der_encode_sig(rr, o.N - ss), xy, kid)
        add("trailing", msg, tag + b"\x00\x01trailing", xy, kid)
        add("bad key", msg, tag, bad_xy, None)
        add("zero point", msg, tag, bytes(64), None)
        add("other key", msg, tag, bytes(_xy64(*keys[(kid + 1) % 3][1])), (kid + 1) % 3)
        if len(msg) > 32:
            t = bytearray(msg)
            t[32 + j % (len(msg) - 32)] ^= 0x40
            add("tamper >= 32", t, tag, xy, kid)
        if len(msg) > 0:
            t = bytearray(msg)
            t[(5 * j) % min(len(msg), 32)] ^= 1
            add("tamper < 32", t, tag, xy, kid)
    for j, tag in enumerate(malformed):
        d, q = keys[j % 3]
        bad = j % 4 == 3
        add("malformed", msgs[j % len(msgs)], tag, bad_xy if bad else bytes(_xy64(*q)), None if bad else j % 3)
    add("malformed", msgs[0], b"", bytes(_xy64(*keys[0][1])), 0)
    for j, tag in enumerate(wellformed):  # decodes, but somebody else's numbers (r or s may be out of range)
        add("foreign", msgs[j % len(msgs)], tag, bytes(_xy64(*keys[j % 3][1])), j % 3)
    want = [expect(m, t, q) for (m, t, q, _) in calls]
    by_kind = {}
    for k, w in zip(what, want):
        by_kind.setdefault(k, set()).add(w)
    assert by_kind == {"valid": {ACCEPT}, "high-s": {ACCEPT}, "trailing": {ACCEPT}, "bad key": {BAD_KEY},
                       "zero point": {BAD_KEY}, "other key": {REJECT}, "tamper >= 32": {ACCEPT},
                       "tamper < 32": {REJECT}, "malformed": {MALFORMED_DER}, "foreign": {REJECT}}, by_kind
    return calls, np.array(want, dtype=np.uint8), [bytes(_xy64(*q)) for _, q in keys]


def test_scheme_form(auth, scheme_calls):
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    calls, want, key_xy = scheme_calls
    assert auth.scheme_verify([]).tolist() == []
    assert auth.scheme_verify([calls[0][:3]]).tolist() == [ACCEPT]  # one call
    order = np.random.default_rng(8).permutation(len(calls))[:300]
    assert len(order) == 300 and len(calls) >= 300
    for sel, what in ((order, "300"), (np.arange(len(calls)), "all")):
        got = auth.scheme_verify([calls[i][:3] for i in sel])
        _same(got, want[sel], what)
    # under a client id registered with the same key, the role path says the same
    with Authenticator(0) as b:
        b.add_role(ROLE_CLIENT)
        for kid, xy in enumerate(key_xy):
            b.set_public_key(ROLE_CLIENT, kid, xy)
        reg = [i for i, c in enumerate(calls) if c[3] is not None]
        got = b.verify_batch([(ROLE_CLIENT, calls[i][3], calls[i][0], calls[i][1]) for i in reg])
        _same(got, want[reg], "role path")
    assert len(reg) >= 200


def test_scheme_form_null_arguments(auth):
    import ctypes
    lib, ctx = auth.lib, auth.ctx
    off = np.zeros(2, dtype=np.uint32)
    buf = np.zeros(64, dtype=np.uint8)
    po, pb = ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(buf.ctypes.data)
    assert lib.mbft_scheme_verify_flat32(ctx, None, None, None, None, None, 0, None) == 0
    assert lib.mbft_scheme_verify_flat32(ctx, pb, None, pb, po, pb, 1, pb) == -1
    assert lib.mbft_scheme_verify_flat32(ctx, pb, po, pb, None, pb, 1, pb) == -1
    assert lib.mbft_scheme_verify_flat32(ctx, pb, po, pb, po, None, 1, pb) == -1
    assert lib.mbft_scheme_verify_flat32(ctx, pb, po, pb, po, pb, 1, None) == -1
    # an empty message and an empty tag need no bytes: a truncated sequence
    st = np.full(1, POISON, dtype=np.uint8)
    assert lib.mbft_scheme_verify_flat32(ctx, None, po, None, po, pb, 1, ctypes.c_void_p(st.ctypes.data)) == 0
    assert st.tolist() == [MALFORMED_DER]
