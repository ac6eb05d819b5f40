"""The P-384 class through the C-ABI (mbft_verify_prehashed_p384_keys,
_keys_device, mbft_scheme_verify_p384_flat32) against the
expected statuses of tests/golden/p384_edges.json:

* every fixture vector in both prehashed forms, and the scheme form;
* sizes 1, 63, 64, 65, 255, 256, 257 and 1,000 with a poisoned status tail;
* one wave holding valid, bad-key and out-of-range lanes;
* four device-form batches in flight on one stream;
* a context with no key; key store, use counts and memo unchanged around a
  batch; NULL arguments.
"""
import ctypes

import numpy as np
import pytest

import p384_ops_util as u

pytestmark = pytest.mark.gpu

ACCEPT, REJECT, MALFORMED_DER, BAD_KEY = 0, 1, 2, 5
POISON = 0xEE


def _hex_rows(vecs, key):
    return np.array([list(bytes.fromhex(v[key])) for v in vecs], dtype=np.uint8)


@pytest.fixture(scope="module")
def golden():
    """(e, r, s, xy, want, labels) of the prehashed vectors; the scheme calls."""
    allv = u.fixtures()
    pre = [v for v in allv if v["kind"] == "prehashed"]
    sch = [v for v in allv if v["kind"] == "scheme"]
    e, r, s = (_hex_rows(pre, k) for k in "ers")
    xy = np.concatenate([_hex_rows(pre, "x"), _hex_rows(pre, "y")], axis=1)
    want = np.array([v["status"] for v in pre], dtype=np.uint8)
    assert e.shape == (len(pre), 48) and xy.shape == (len(pre), 96) and len(pre) >= 200
    assert {int(w) for w in want} == {ACCEPT, REJECT, BAD_KEY}
    return e, r, s, xy, want, [v["label"] for v in pre], sch


@pytest.fixture(scope="module")
def auth(lib):
    """A context that never holds a key."""
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    yield a
    a.close()


def _host(a, e, r, s, xy):
    n = len(e)
    e, r, s, xy = (np.ascontiguousarray(v, dtype=np.uint8) for v in (e, r, s, xy))
    out = np.full(n + 256, POISON, dtype=np.uint8)
    rc = a.lib.mbft_verify_prehashed_p384_keys(a.ctx, *(ctypes.c_void_p(v.ctypes.data) for v in (e, r, s, xy)), n,
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
    import torch
    n = len(e)
    d = _to_device(e, r, s, xy)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    a.verify_prehashed_p384_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n,
                                        d[4].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return _device_status(d, n)


def _both(a, e, r, s, xy):
    h, d = _host(a, e, r, s, xy), _device(a, e, r, s, xy)
    assert (h == d).all(), np.nonzero(h != d)[0][:10]
    return h


def _same(st, want, labels=None, what=""):
    bad = np.nonzero(np.asarray(st) != np.asarray(want))[0]
    assert not len(bad), (what, len(bad), [(int(i), labels[i] if labels else "", int(st[i]), int(want[i])) for i in bad[:10]])


def test_fixture_vectors_prehashed(auth, golden):
    e, r, s, xy, want, labels, _ = golden
    _same(_host(auth, e, r, s, xy), want, labels, "host")
    _same(_device(auth, e, r, s, xy), want, labels, "device")
    _same(auth.verify_prehashed_p384_keys(e, r, s, xy), want, labels, "binding")
    # each vector alone as well: lane 0 of a lone wave
    for i in (0, 1, len(want) // 2, len(want) - 1):
        _same(_both(auth, e[i:i + 1], r[i:i + 1], s[i:i + 1], xy[i:i + 1]), want[i:i + 1], labels[i:i + 1], "alone")


def test_fixture_vectors_scheme(auth, golden):
    sch = golden[6]
    calls = [(bytes.fromhex(v["msg"]), bytes.fromhex(v["tag"]), bytes.fromhex(v["xy"])) for v in sch]
    want = np.array([v["status"] for v in sch], dtype=np.uint8)
    labels = [v["label"] for v in sch]
    assert {int(w) for w in want} == {ACCEPT, REJECT, MALFORMED_DER, BAD_KEY}
    assert {len(c[0]) for c in calls} >= {0, 1, 15, 16, 17, 23, 100}
    assert auth.scheme_verify_p384([]).tolist() == []
    _same(auth.scheme_verify_p384(calls), want, labels, "all")
    _same(auth.scheme_verify_p384(calls[:1]), want[:1], labels, "one call")
    order = np.random.default_rng(9).permutation(len(calls))
    _same(auth.scheme_verify_p384([calls[i] for i in order]), want[order], [labels[i] for i in order], "shuffled")
    # only malformed calls: nothing travels
    mal = [i for i, w in enumerate(want) if w == MALFORMED_DER]
    _same(auth.scheme_verify_p384([calls[i] for i in mal]), want[mal], None, "malformed only")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_and_guards(auth, golden, n):
    e, r, s, xy, want, labels, _ = golden
    idx = (np.arange(n) * 7 + n) % len(want)
    _same(_both(auth, e[idx], r[idx], s[idx], xy[idx]), want[idx], [labels[i] for i in idx], n)


def test_one_wave_of_mixed_lanes(auth, golden):
    """64 lanes in which accepted, rejected-in-range, out-of-range and bad-key
    items alternate: a lane that dies early leaves its neighbours' answers alone."""
    e, r, s, xy, want, labels, _ = golden
    kinds = {"ok": [i for i, w in enumerate(want) if w == ACCEPT],
             "range": [i for i, l in enumerate(labels) if l.startswith(("r = ", "s = "))],
             "bad": [i for i, w in enumerate(want) if w == BAD_KEY],
             "reject": [i for i, (w, l) in enumerate(zip(want, labels)) if w == REJECT and l.startswith("wrong")]}
    assert all(len(v) >= 8 for v in kinds.values())
    order = ["ok", "bad", "range", "ok", "reject", "bad", "ok", "range"]
    idx = np.array([kinds[order[lane % 8]][(lane // 8) % len(kinds[order[lane % 8]])] for lane in range(64)])
    assert len({int(w) for w in want[idx]}) == 3
    _same(_both(auth, e[idx], r[idx], s[idx], xy[idx]), want[idx], [labels[i] for i in idx], "wave")


def test_batches_in_flight(auth, golden):
    """Four back-to-back device calls on one caller stream, no synchronize
    between them: each takes its own buffer of the rotation."""
    import torch
    e, r, s, xy, want, labels, _ = golden
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    batches = []
    for b in range(4):
        idx = (np.arange(700) + 53 * b + 5) % len(want)
        batches.append((idx, _to_device(e[idx], r[idx], s[idx], xy[idx])))
    torch.cuda.synchronize()
    for idx, d in batches:  # (no synchronize inside this loop)
        auth.verify_prehashed_p384_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                               len(idx), d[4].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for b, (idx, d) in enumerate(batches):
        _same(_device_status(d, len(idx)), want[idx], None, "batch %d" % b)


def test_context_without_keys(lib, golden):
    from minbft_amd.authenticator import Authenticator
    e, r, s, xy, want, labels, sch = golden
    with Authenticator(0) as a:
        _same(_host(a, e[:100], r[:100], s[:100], xy[:100]), want[:100], labels, "host")
        _same(_device(a, e[:100], r[:100], s[:100], xy[:100]), want[:100], labels, "device")
        v = sch[0]
        assert a.scheme_verify_p384([(bytes.fromhex(v["msg"]), bytes.fromhex(v["tag"]), bytes.fromhex(v["xy"]))]).tolist() \
            == [v["status"]]
        assert a.key_memory()[0] == 0


def test_leaves_the_key_store_alone(lib, golden):
    """Registered P-256 keys of three classes, accounting on, a memo set: a
    P-384 batch changes none of it, and P-384 keys still cannot be registered."""
    from golden_util import prehashed_arrays
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    import p384_ref as o
    e, r, s, xy, want, labels, _ = golden
    pxy, pe, pr, ps, pexp, _ = prehashed_arrays()
    distinct = []
    for i in range(len(pexp)):
        if not any((pxy[i] == pxy[j]).all() for j in distinct):
            distinct.append(i)
        if len(distinct) == 3:
            break
    own = np.array([i for i in range(len(pexp)) if any((pxy[i] == pxy[j]).all() for j in distinct)])
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        for cid, (j, select) in enumerate(zip(distinct, (lambda: a.set_key_window(8), lambda: a.set_key_window(0),
                                                         lambda: a.set_key_signed_teeth(5)))):
            select()
            a.set_public_key(ROLE_CLIENT, cid, bytes(pxy[j]))
        a.set_key_accounting(True)
        a.set_verified_memo(1 << 20)
        slot_of = {bytes(pxy[j]): a.key_slot(ROLE_CLIENT, cid) for cid, j in enumerate(distinct)}
        slots = np.array([slot_of[bytes(pxy[i])] for i in own], dtype=np.uint32)
        before = a.verify_prehashed(pe[own], pr[own], ps[own], slots)
        _same(before, np.where(pexp[own] == 1, ACCEPT, REJECT), None, "registered, before")

        def state():
            return (a.key_memory(), [v.tolist() for v in a.key_usage(n=8)], a.verified_memo_stats(),
                    [a.key_slot(ROLE_CLIENT, cid) for cid in range(3)], a.windows(), a.verified_memo())

        st0 = state()
        assert sum(st0[1][0]) > 0 and st0[5] > 0
        _same(_both(a, e, r, s, xy), want, labels, "p384")
        assert state() == st0
        # mbft_set_public_key_pkix keeps refusing a P-384 key
        with pytest.raises(Exception):
            a.set_public_key(ROLE_CLIENT, 9, o.pkix_encode(o.pubkey(77)))
        assert a.pkix_parse_p384(o.pkix_encode(o.pubkey(77))) == o.pkix_encode(o.pubkey(77))[24:]
        assert state() == st0
        _same(a.verify_prehashed(pe[own], pr[own], ps[own], slots), before, None, "registered, after")


def test_empty_and_null(auth):
    one = np.zeros(96, dtype=np.uint8)
    p = ctypes.c_void_p(one.ctypes.data)
    lib, ctx = auth.lib, auth.ctx
    assert lib.mbft_verify_prehashed_p384_keys(ctx, None, None, None, None, 0, None) == 0
    assert lib.mbft_verify_prehashed_p384_keys_device(ctx, None, None, None, None, 0, None, None) == 0
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert lib.mbft_verify_prehashed_p384_keys(ctx, *args[:4], 1, args[4]) == -1
        assert lib.mbft_verify_prehashed_p384_keys_device(ctx, *args[:4], 1, args[4], None) == -1
    assert lib.mbft_verify_prehashed_p384_keys(None, p, p, p, p, 1, p) == -1
    off = np.zeros(2, dtype=np.uint32)
    po = ctypes.c_void_p(off.ctypes.data)
    fn = lib.mbft_scheme_verify_p384_flat32
    assert fn(ctx, None, None, None, None, None, 0, None) == 0
    assert fn(ctx, p, None, p, po, p, 1, p) == -1
    assert fn(ctx, p, po, p, None, p, 1, p) == -1
    assert fn(ctx, p, po, p, po, None, 1, p) == -1
    assert fn(ctx, p, po, p, po, p, 1, None) == -1
    assert fn(None, p, po, p, po, p, 1, p) == -1
    st = np.full(1, POISON, dtype=np.uint8)
    assert fn(ctx, None, po, None, po, p, 1, ctypes.c_void_p(st.ctypes.data)) == 0
    assert st.tolist() == [MALFORMED_DER]
