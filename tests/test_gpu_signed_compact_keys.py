"""Signed compact keys (mbft_set_key_signed_teeth, t = 2..9 teeth): a key with
a table of 2^(t-1) entries, verified by the compact class's comb over a
signed all-nonzero recoding (minbft_amd/csrc/teeth_dev.h) -- through the
C-ABI, against the golden expectations and the oracle.

* the prehashed golden set, tests/golden/ladder_edges.json and
  tests/golden/steeth_edges.json (the scalars whose last column meets the
  doubling case, odd and even; 1, 2, N - 1, N - 2; all-same-sign columns; the
  ragged top; u1 G == +-u2 Q and Q == +-G joins) with every key signed
  compact, for every t at the smallest size of each verify form: <= 256 items
  (split), the whole set as one batch (quads by default, pairs by setting),
  and tiled to 8,192 items (k_verify, the second queue, k_verify_ladder);
* signed 5, unsigned 4, window 0 and window 8 side by side in every wave;
* batches in flight on two caller streams;
* every entry point against the oracle with signed compact client keys;
* two engines; selecting, switching and refusing; clear and re-register.
"""
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays

pytestmark = pytest.mark.gpu

REJECT = 1
STEETH = list(range(2, 10))


@pytest.fixture(scope="module")
def golden():
    """prehashed.json (551 vectors) + ladder_edges.json + steeth_edges.json, as one set."""
    parts = [prehashed_arrays(), prehashed_arrays("ladder_edges.json"), prehashed_arrays("steeth_edges.json")]
    assert len(parts[0][5]) == 551 and len(parts[1][5]) >= 200 and 200 <= len(parts[2][5]) <= 400
    assert sum(l.startswith("u2=degenerate") for l in parts[2][5]) >= 48
    xy, e, r, s, exp = (np.concatenate([p[k] for p in parts]) for k in range(5))
    return xy, e, r, s, exp, sum((p[5] for p in parts), [])


def _check(st, exp, labels, what=""):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i % len(labels)], i, int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, len(bad), bad[:10])
    assert set(np.unique(st).tolist()) <= {0, REJECT}, what


@pytest.mark.parametrize("form", ["split", "quads", "pairs", "tiled"])
@pytest.mark.parametrize("t", STEETH)
def test_golden_every_teeth_and_form(lib, golden, t, form):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    assert 256 < n <= 4096
    with Authenticator(0) as a:
        if form == "pairs":
            a.set_small_batch_form(0)
            a.set_small_batch_inverse(1)
        a.set_key_signed_teeth(t)
        assert a.key_signed_teeth() == t and a.key_teeth() == 0 and a.windows()[1] == 0
        slots, valid = a.register_points(xy)
        assert valid.all()
        if form == "split":
            st = np.concatenate([a.verify_prehashed(e[k:k + 256], r[k:k + 256], s[k:k + 256], slots[k:k + 256])
                                 for k in range(0, n, 256)])
            want = exp
        elif form == "tiled":
            idx = np.arange(8192) % n
            st = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
            want = exp[idx]
        else:
            st = a.verify_prehashed(e, r, s, slots)
            want = exp
    _check(st, want, labels, "%s t=%d" % (form, t))


def _register_classes(a, xy, classes):
    """Deals the distinct keys of xy to the classes (the key with the most
    vectors first, each to the class with the fewest vectors so far) and
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
        {"w": a.set_key_window, "t": a.set_key_teeth, "s": a.set_key_signed_teeth}[kind](val)
        sl, v = a.register_points(xy[cls == ci])
        assert v.all()
        slots[cls == ci] = sl
    return slots, cls


def test_mixed_classes(lib, golden):
    """Signed 5, unsigned 4, window 0 and window 8 in one context, the items
    ordered so that every four consecutive ones -- hence every wave -- hold
    all four classes: below and above 4,096 items."""
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    order = np.random.default_rng(12).permutation(len(labels))
    xy, e, r, s, exp = (v[order] for v in (xy, e, r, s, exp))
    labels = [labels[i] for i in order]
    with Authenticator(0) as a:
        slots, cls = _register_classes(a, xy, [("s", 5), ("t", 4), ("w", 0), ("w", 8)])
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 0 and a.windows()[1] == 8
        groups = [np.nonzero(cls == ci)[0] for ci in range(4)]
        assert all(len(g) >= 100 for g in groups)
        for n in (len(labels), 4352):
            idx = np.array([groups[i % 4][(i // 4) % len(groups[i % 4])] for i in range(n)])
            for w in range(0, n - 63, 64):
                assert set(cls[idx[w:w + 64]].tolist()) == {0, 1, 2, 3}
            st = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
            _check(st, exp[idx], [labels[i] for i in idx], "n=%d" % n)


def test_batches_in_flight_on_two_streams(lib, golden):
    """Four batches of ~5,000 items, alternating between two caller streams,
    no synchronize between the calls: window-8 and signed compact keys mixed."""
    import torch
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    dev = torch.device("cuda", 0)
    with Authenticator(0) as a:
        a.set_key_window(8)
        s8, _ = a.register_points(xy[: n // 3])
        a.set_key_signed_teeth(6)
        s6, _ = a.register_points(xy[n // 3:])
        slots = np.concatenate([s8, s6])
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        batches = []
        for b in range(4):
            idx = (np.arange(4900 + 37 * b) * (b + 1) + 11 * b) % n  # a different order per batch
            d = [torch.from_numpy(np.ascontiguousarray(v[idx])).to(dev) for v in (e, r, s)]
            d.append(torch.from_numpy(slots[idx].astype(np.uint32).view(np.int32)).to(dev))
            d.append(torch.full((len(idx),), 0xAA, dtype=torch.uint8, device=dev))
            batches.append((idx, d))
        torch.cuda.synchronize()
        for b, (idx, d) in enumerate(batches):  # (no synchronize inside this loop)
            a.verify_prehashed_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                      len(idx), d[4].data_ptr(), streams[b % 2].cuda_stream)
        for st in streams:
            st.synchronize()
        for b, (idx, d) in enumerate(batches):
            _check(d[4].cpu().numpy(), exp[idx], [labels[i] for i in idx], "batch %d" % b)


# ----------------------------------------------------------------- entry points
@pytest.fixture(scope="module")
def big_stream():
    from test_gpu_tablefree import _streams
    return _streams(1, 150, 0x57E01)  # 600 messages + the faults: the device message layer


@pytest.fixture(scope="module")
def small_stream():
    from test_gpu_tablefree import _streams
    return _streams(4, 6, 0x57E02)  # 60 messages + the faults: the small route


def _auth(keys):
    """Replica and USIG keys at window 8, client keys signed compact (t = 5)."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    a = Authenticator(0)
    for role in (o.ROLE_REPLICA, o.ROLE_USIG, o.ROLE_CLIENT):
        if role == o.ROLE_CLIENT:
            a.set_key_signed_teeth(5)
        else:
            a.set_key_window(8)
        a.add_role(role)
        for id_, q in keys[role].items():
            a.set_public_key(role, id_, o.pkix_encode(q))
    a.enable_usig(True)
    return a


def test_lone_calls(lib, monkeypatch, small_stream):
    """mbft_verify_message_authen_tag, one call at a time."""
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    from test_gpu_tablefree import _calls, _oracle_auth
    _fast_oracle(monkeypatch)
    n, msgs, keys = small_stream
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
        cls, nbytes = a.key_class(o.ROLE_CLIENT, rq.client_id)
        assert (cls, nbytes) == (0x205, 1024)
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


def test_message_layer_device(lib, monkeypatch, big_stream):
    """validate_messages_flat over 600 messages: the device message layer."""
    from oracle import p256 as o
    from test_gpu_configs import _fast_oracle
    from test_gpu_tablefree import _oracle_auth
    _fast_oracle(monkeypatch)
    n, msgs, keys = big_stream
    assert len(msgs) > 512
    want = np.array(o.validate_messages(_oracle_auth(keys), msgs, n, 0))
    assert (want != 0).sum() >= 3
    a = _auth(keys)
    try:
        got = a.validate_messages_via_flat(msgs, n, 0)
    finally:
        a.close()
    assert (got == want).all(), np.nonzero(got != want)[0][:10]


def test_two_engines(lib, golden):
    from minbft_amd.authenticator import Authenticator
    from test_gpu_multi import _extra_devices
    xy, e, r, s, exp, labels = golden
    n = len(labels)
    with Authenticator(0) as a:
        a.set_key_signed_teeth(4)
        s1, _ = a.register_points(xy[:300])          # replayed on the engine added below
        a.set_key_signed_teeth(9)
        s2, _ = a.register_points(xy[300:500])       # (a second run of another class to replay)
        a.add_device(_extra_devices(1)[0])
        assert a.key_signed_teeth() == 9
        s3, _ = a.register_points(xy[500:])          # registered on both at once
        slots = np.concatenate([s1, s2, s3])
        idx = np.arange(4200) % n
        one = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])    # (below the default shard size: one engine)
        a.set_shard_min(512)
        two = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
    _check(two, exp[idx], labels)
    assert (one == two).all()


# -------------------------------------------------------------------- key store
def test_signed_teeth_and_refusals(lib):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    assert (_lib.STEETH_MIN, _lib.STEETH_MAX, _lib.KEY_CLASS_SIGNED_TEETH(5)) == (2, 9, 0x205)
    with Authenticator(0) as a:
        g0, q0 = a.windows()
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 0
        for t in (0, 1, 10, -1):
            assert a.lib.mbft_set_key_signed_teeth(a.ctx, t) == _lib.ERR_ARG
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 0 and a.windows() == (g0, q0)
        a.set_key_signed_teeth(_lib.STEETH_MIN)
        assert a.key_signed_teeth() == 2 and a.key_teeth() == 0 and a.windows() == (g0, 0)
        a.set_key_signed_teeth(_lib.STEETH_MAX)
        assert a.key_signed_teeth() == 9 and a.key_teeth() == 0 and a.windows() == (g0, 0)
        for w in (1, 2, 3, 30, -1):  # the window's own range is what it was
            assert a.lib.mbft_set_key_window(a.ctx, w) == _lib.ERR_ARG
        assert a.lib.mbft_set_key_teeth(a.ctx, 9) == _lib.ERR_ARG  # ... and the unsigned class's
        assert a.key_signed_teeth() == 9
        a.set_key_teeth(4)
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 4 and a.windows() == (g0, 0)
        a.set_key_signed_teeth(4)
        assert a.key_signed_teeth() == 4 and a.key_teeth() == 0 and a.windows() == (g0, 0)
        a.set_key_window(_lib.WINDOW_NONE)
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 0 and a.windows() == (g0, 0)
        a.set_key_signed_teeth(7)
        a.set_key_window(4)
        assert a.key_signed_teeth() == 0 and a.key_teeth() == 0 and a.windows() == (g0, 4)


def test_clear_and_reregister(lib, golden):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = golden
    with Authenticator(0) as a:
        for kind, v in (("s", 5), ("w", 8), ("s", 5), ("t", 4), ("s", 2)):
            {"w": a.set_key_window, "t": a.set_key_teeth, "s": a.set_key_signed_teeth}[kind](v)
            slots, valid = a.register_points(xy)
            assert valid.all()
            _check(a.verify_prehashed(e, r, s, slots), exp, labels, "%s %d" % (kind, v))
            a.clear_keys()
