"""The resident single-call verifier (mbft_set_resident; resident.cpp,
verify_server.hip k_verify_server) against the oracle and the golden vectors:
VerifyMessageAuthenTag (sample/authentication/authenticator.go:121-134)
one call at a time and from many threads at once, through a kernel that
stays on the GPU between calls -- the same statuses as every other path,
across idle exits and relaunches, key and window changes, batches running
beside it, and turning it off."""
import hashlib
import threading
import time

import numpy as np
import pytest

from golden_util import load

pytestmark = pytest.mark.gpu


def _make_auth(fx, usig=True):
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    for role, m in fx["keystore"].items():
        a.add_role(int(role))
        for id_, pk in m.items():
            a.set_public_key(int(role), int(id_), bytes.fromhex(pk))
    a.enable_usig(usig)
    return a


@pytest.mark.parametrize("name", ["authen.json", "usig_epoch.json"])
def test_resident_golden_sequences(lib, name):
    """Every golden call sequence (ECDSA quirk, DER edge cases, unknown
    roles / ids, USIG epoch capture and mismatch) one call at a time."""
    fx = load(name)
    for seq in fx["sequences"]:
        a = _make_auth(fx)
        try:
            a.set_resident(4)
            got = [a.verify_status(c["role"], c["id"], bytes.fromhex(c["msg"]), bytes.fromhex(c["tag"]))
                   for c in seq]
            st = a.resident_stats()
        finally:
            a.close()
        want = [c["expect"] for c in seq]
        bad = [(c["note"], g, w) for c, g, w in zip(seq, got, want) if g != w]
        assert not bad, bad[:10]
        assert st["calls"] == len(seq) and st["launches"] >= 1 and st["fallbacks"] == 0, st


@pytest.mark.parametrize("form,host_u,hjm", [("two", "1", "4"), ("one", "1", "4"), ("two", "0", "4"),
                                             ("two", "1", "0"), ("one", "1", "0")])
def test_resident_prehashed_golden_as_calls(lib, monkeypatch, form, host_u, hjm):
    """The 551 prehashed golden vectors (valid, tampered, wrong key, high s,
    range edges, e = 0 / N, e >= N, R.x >= N, final infinity, u1 G = u2 Q,
    Q = +-G, comb collisions) as client calls: msg = e (a 32-byte message is
    its own quirk digest, crypto.go:121), tag = DER(r, s); the degenerate
    ones take the exact path inside the resident kernel; the rest leave
    their partial sums to the host join (two workgroups per item, one per
    scalar, or one workgroup; u1, u2 from the host, or computed by the
    waves); or, with MBFT_RESIDENT_HOST_JOIN_MAX=0, joined and x-checked on
    the GPU (the form windows of more than a few calls take)."""
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    from oracle import p256 as o
    monkeypatch.setenv("MBFT_RESIDENT_FORM", form)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_U", host_u)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_JOIN_MAX", hjm)
    vecs = load("prehashed.json")
    a = Authenticator(0)
    try:
        a.set_key_window(8)
        a.add_role(ROLE_CLIENT)
        ids, calls, want = {}, [], []
        for v in vecs:
            key = v["qx"] + v["qy"]
            if key not in ids:
                try:
                    a.set_public_key(ROLE_CLIENT, len(ids), bytes.fromhex(key))
                except ValueError:
                    continue  # an off-curve key: not a call-level case
                ids[key] = len(ids)
            r, s = int(v["r"], 16), int(v["s"], 16)
            calls.append((ROLE_CLIENT, ids[key], bytes.fromhex(v["e"]), o.der_encode_sig(r, s)))
            want.append(0 if v["expect"] else 1)
        a.set_resident(8)
        got = [a.verify_status(*c) for c in calls]
        assert a.resident_stats()["calls"] == len(calls)
        a.set_resident(0)
        ref = list(a.verify_batch(calls))
    finally:
        a.close()
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:10]
    assert ref == got
    assert len(calls) > 500 and 0 in got and 1 in got


def _thread_calls(o, T, reps, tag):
    """Per thread: its own client key and USIG key; valid and tampered ECDSA
    calls and a USIG stream (captures, a mismatch, a tampered UI), with the
    oracle's sequential results."""
    from minbft_amd.authenticator import ROLE_CLIENT, ROLE_USIG
    ks = o.KeyStore(keys={ROLE_CLIENT: {}, ROLE_USIG: {}})
    seqs = []
    for t in range(T):
        dc = int.from_bytes(hashlib.sha256(b"%s client %d" % (tag, t)).digest(), "big") % (o.N - 1) + 1
        du = int.from_bytes(hashlib.sha256(b"%s usig %d" % (tag, t)).digest(), "big") % (o.N - 1) + 1
        ks.keys[ROLE_CLIENT][t] = o.pubkey(dc)
        ks.keys[ROLE_USIG][t] = o.pubkey(du)
        epoch = 5000 + t
        calls = []
        for k in range(reps):
            msg = b"resident %d request %d" % (t, k) + bytes(40)
            r, s = o.ecdsa_sign(dc, o.quirk_digest(msg))
            good = o.der_encode_sig(r, s)
            calls.append((ROLE_CLIENT, t, msg, good))
            calls.append((ROLE_CLIENT, t, b"Y" + msg[1:], good))       # tampered inside e
            calls.append((ROLE_CLIENT, t, msg[:40] + b"!" + msg[41:], good))  # past byte 32: accepted
        for ctr in (1, 2, 3):
            m = b"resident usig %d msg %d" % (t, ctr)
            calls.append((ROLE_USIG, t, m, o.usig_create_ui(du, m, epoch, ctr)))
        m = b"resident usig %d other epoch" % t
        calls.append((ROLE_USIG, t, m, o.usig_create_ui(du, m, epoch + 1, 4)))
        m = b"resident usig %d tampered" % t
        ui = bytearray(o.usig_create_ui(du, m, epoch, 5))
        ui[-1] ^= 1
        calls.append((ROLE_USIG, t, m, bytes(ui)))
        ref = o.Authenticator(ks)
        seqs.append([(c, ref.verify(*c)) for c in calls])
    return ks, seqs


def _register(a, ks):
    from minbft_amd.authenticator import ROLE_CLIENT, ROLE_USIG
    a.add_role(ROLE_CLIENT)
    a.add_role(ROLE_USIG)
    a.enable_usig(True)
    for role in (ROLE_CLIENT, ROLE_USIG):
        for t, q in ks.keys[role].items():
            a.set_public_key(role, t, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))


@pytest.mark.parametrize("slots,coalesce", [(16, False), (4, True)])
def test_resident_concurrent_threads_vs_oracle(lib, slots, coalesce):
    """16 threads at once, each its own sequence; with 4 slots the calls
    that find every slot taken go through the coalescer instead.  Every
    status equals the oracle's sequential result for its thread."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    T, reps = 16, 4
    ks, seqs = _thread_calls(o, T, reps, b"conc%d" % slots)
    a = Authenticator(0)
    try:
        _register(a, ks)
        a.set_concurrency(4)
        if coalesce:
            a.set_coalescing(True)
        a.set_resident(slots)
        got = [[] for _ in range(T)]
        barrier = threading.Barrier(T)

        def run(t):
            barrier.wait()
            for c, _ in seqs[t]:
                got[t].append(a.verify_status(*c))

        th = [threading.Thread(target=run, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        st = a.resident_stats()
    finally:
        a.close()
    for t in range(T):
        assert got[t] == [w for _, w in seqs[t]], t
    assert any(w == 9 for _, w in seqs[0])  # EPOCH_MISMATCH exercised
    n = sum(len(s) for s in seqs)
    assert st["calls"] + st["fallbacks"] == n, st
    assert st["calls"] > 0


def test_resident_idle_exit_and_relaunch(lib, monkeypatch):
    """A short idle limit and lifetime: the kernel leaves between calls and
    the next call relaunches it; statuses stay right across generations."""
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    monkeypatch.setenv("MBFT_RESIDENT_IDLE_US", "300")
    monkeypatch.setenv("MBFT_RESIDENT_LIFE_MS", "4")
    ks, seqs = _thread_calls(o, 1, 6, b"idle")
    a = Authenticator(0)
    try:
        _register(a, ks)
        a.set_resident(2)
        got = []
        for k, (c, _) in enumerate(seqs[0]):
            got.append(a.verify_status(*c))
            if k % 3 == 0:
                time.sleep(0.003)  # past the idle limit: the generation leaves
        # a burst longer than the lifetime: relaunched while calls arrive
        t0 = time.perf_counter()
        burst = 0
        while time.perf_counter() - t0 < 0.02:
            c, w = seqs[0][0]
            assert a.verify_status(*c) == w
            burst += 1
        st = a.resident_stats()
    finally:
        a.close()
    assert got == [w for _, w in seqs[0]]
    assert st["launches"] >= 4, st
    assert st["calls"] == len(got) + burst


def test_resident_key_and_window_changes(lib):
    """Keys registered and the generator table rebuilt while the resident
    kernel is live (each waits for the calls in flight; every item carries
    its own table pointers)."""
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    from oracle import p256 as o
    a = Authenticator(0)
    try:
        a.add_role(ROLE_CLIENT)
        keys = {}
        a.set_resident(4)
        for step, gw in enumerate((16, 12, 16)):
            d = int.from_bytes(hashlib.sha256(b"late key %d" % step).digest(), "big") % (o.N - 1) + 1
            q = o.pubkey(d)
            a.set_public_key(ROLE_CLIENT, step, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
            keys[step] = d
            if step == 1:
                a.set_generator_window(gw)
            for i, dk in keys.items():
                msg = b"window %d key %d" % (gw, i) + bytes(30)
                r, s = o.ecdsa_sign(dk, o.quirk_digest(msg))
                tag = o.der_encode_sig(r, s)
                assert a.verify_status(ROLE_CLIENT, i, msg, tag) == 0, (step, i)
                assert a.verify_status(ROLE_CLIENT, i, b"Z" + msg[1:], tag) == 1, (step, i)
                assert a.verify_status(ROLE_CLIENT, 99, msg, tag) == o.UNKNOWN_KEY
        assert a.resident_stats()["calls"] >= 9
    finally:
        a.close()


def test_resident_beside_batches(lib):
    """Single calls through the resident kernel while 256K-call flat batches
    (the Go binding's compact form, GPU decode) run on the lanes: both stay
    exact, no batch is held behind the kernel (round 5's bound was +10 ms),
    and the Go binding's default resident kernel (32 slots, a pool of
    MBFT_RESIDENT_SERVERS = 16 workgroups) costs the batches little: the
    best of 4 batches with it live within 1.25x the best of 4 without, off /
    live alternated twice (1.17 inside the whole GPU suite's process, where
    127 tests ran before it; 1.07-1.10 in a fresh process, which is what the
    bench's resident_interference line measures for C2 and the authenticator
    level).  Measured on this shape (tools/beside_probe.py,
    profiles/round6_beside_*.jsonl): 1.07-1.10 -- and 1.07 with ONE server
    workgroup and no calls at all, against 1.02-1.03 for the same calls
    through the launch path: the persistent dispatch itself costs the batch,
    not the pool's size, its PCIe polling (no change with 32x fewer polls)
    or other work's launch latency (unchanged, tools/launch_probe.py).  One
    workgroup pair per slot cost C2 16-25 % at 32 slots."""
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT, flat_calls, host_array
    from oracle import p256 as o
    d = int.from_bytes(hashlib.sha256(b"beside").digest(), "big") % (o.N - 1) + 1
    q = o.pubkey(d)
    msgs = [b"beside %d" % i + bytes(40) for i in range(64)]
    tags = []
    for m in msgs:
        r, s = o.ecdsa_sign(d, o.quirk_digest(m))
        tags.append(o.der_encode_sig(r, s))
    B = 1 << 18
    batch = [(ROLE_CLIENT, 0, msgs[i % 64] if i % 7 else b"#" + msgs[i % 64][1:], tags[i % 64])
             for i in range(B)]
    want_batch = np.array([0 if i % 7 else 1 for i in range(B)], dtype=np.uint8)
    flat = flat_calls(batch, True, compact=True)
    a = Authenticator(0)
    alone, live, errs, stats = [], [], [], []
    try:
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
        a.set_concurrency(2)

        out = host_array(B)  # one status buffer: no page-locked free (a device sync) between batches

        def timed(k):
            ts = []
            for _ in range(k):
                t0 = time.perf_counter()
                a.verify_flat32_arrays(*flat, out=out, pinned=True)
                ts.append(time.perf_counter() - t0)
                assert np.array_equal(np.asarray(out), want_batch)
            return ts

        timed(2)  # warm the lanes
        for _ in range(2):
            alone += timed(4)
            a.set_resident(32)
            stop = threading.Event()

            def singles():
                k = 0
                while not stop.is_set():
                    i = k % 64
                    st = a.verify_status(ROLE_CLIENT, 0, msgs[i], tags[i])
                    if st != 0:
                        errs.append((k, st))
                    k += 1
                    time.sleep(0.0002)

            th = threading.Thread(target=singles)
            th.start()
            try:
                time.sleep(0.01)
                live += timed(4)
            finally:
                stop.set()
                th.join()
            stats.append(a.resident_stats())
            a.set_resident(0)
    finally:
        a.close()
    assert not errs, errs[:5]
    assert all(st["calls"] > 0 for st in stats), stats
    assert max(live) < max(alone) + 0.010, (live, alone, stats)  # nothing held behind the kernel
    assert min(live) <= 1.25 * min(alone), (live, alone, stats)


def test_resident_off_and_close_while_live(lib):
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    from oracle import p256 as o
    d = 12345
    q = o.pubkey(d)
    msg = b"off and on" + bytes(30)
    r, s = o.ecdsa_sign(d, o.quirk_digest(msg))
    tag = o.der_encode_sig(r, s)
    a = Authenticator(0)
    try:
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
        a.set_resident(3)
        assert a.verify_status(ROLE_CLIENT, 0, msg, tag) == 0
        a.set_resident(0)
        assert a.verify_status(ROLE_CLIENT, 0, msg, tag) == 0  # the launch path
        assert a.resident_stats()["slots"] == 0
        a.set_resident(64)
        assert a.verify_status(ROLE_CLIENT, 0, msg, tag) == 0
        with pytest.raises(Exception):
            a.set_resident(65)
    finally:
        a.close()  # with the kernel live


@pytest.mark.parametrize("f", [1, 4])
def test_resident_small_check_windows_vs_oracle(lib, monkeypatch, f):
    """The small message-check route with the resident kernel serving its
    calls (check_calls_on -> resident_check: windows whose unique calls fit
    8 slots go to the mailbox, larger ones launch as before): C3 streams with
    faults in windows of 1, 2, 3 and 16 messages, resolved in order, against
    the oracle's sequential validators."""
    import random
    from test_gpu_configs import _c3_streams, _fast_oracle
    from test_gpu_msgdev import _auth_for
    from test_gpu_small_check import _oracle_want, _windows
    _fast_oracle(monkeypatch)
    rng = random.Random(0x7E5 + f)
    n, msgs, keys = _c3_streams(f, 4 if f == 4 else 40, rng, True)
    want = _oracle_want(keys, msgs, n)
    for sizes in ([1], [2], [3, 1], [16]):
        a = _auth_for(keys)
        try:
            a.set_resident(8)
            got = _windows(a, msgs, n, sizes)
            st = a.resident_stats()
        finally:
            a.close()
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (sizes, [(int(i), int(got[i]), int(want[i])) for i in bad[:10]])
        if sizes == [1]:
            assert st["calls"] > 0, st
    assert (want != 0).any() and (want == 0).any()


def test_resident_small_check_golden_and_replies(lib):
    """The golden MinBFT streams (windows of 1) and the client's REPLY loop
    (validate_replies_flat, windows of 1) through the resident kernel."""
    from minbft_amd.authenticator import Authenticator
    from test_gpu_authen import _msgs
    from test_gpu_replies_go import _go_loop
    from test_gpu_small_check import _windows
    from oracle import p256 as o
    fx = load("messages.json")

    def ctx():
        a = Authenticator(0)
        for role, m in fx["keystore"].items():
            a.add_role(int(role))
            for id_, pk in m.items():
                a.set_public_key(int(role), int(id_), bytes.fromhex(pk))
        a.enable_usig(True)
        return a
    for sq in fx["sequences"]:
        msgs = _msgs(sq["msgs"])
        with ctx() as a:
            want = a.validate_messages_via_flat(msgs, sq["n"], 3)
        with ctx() as a:
            a.set_resident(8)
            got = _windows(a, msgs, sq["n"], [1])
        assert [int(g) for g in got] == [int(w) for w in want]
    for sq in fx["replies"]:
        msgs = _msgs(sq["msgs"])
        oks = o.KeyStore()
        oks.keys = {int(role): {int(i): o.pkix_decode(bytes.fromhex(pk)) for i, pk in m.items()}
                    for role, m in fx["keystore"].items()}
        want = o.validate_replies(o.Authenticator(oks), msgs, sq["client_id"], 0)
        with ctx() as a:
            a.set_resident(8)
            got, panic_at = _go_loop(a, msgs, sq["client_id"], 1)
        stop = next((i for i, w in enumerate(want) if w == (9 << 8)), None)
        if stop is None:
            assert panic_at is None and got == want
        else:
            assert got == want[:stop]


def test_resident_native_threads_stress(lib):
    """64 and 16 OS threads (tools/conc_calls.cpp: the C-ABI from native
    threads, as goroutines reach it through cgo) hammering 64 / 16 slots with
    a mix of valid and tampered calls, several rounds: every status must be
    the expected one (a race in the mailbox protocol shows up as a stray
    reject or accept here, not in the slower Python-thread tests: a done word
    that overtook its partial sums' stores showed up as 1-7 stray rejects in
    ~40 K calls)."""
    import ctypes

    from __graft_entry__ import build_conc_calls
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    from oracle import p256 as o
    drv = ctypes.CDLL(build_conc_calls())
    drv.conc_calls_run.restype = ctypes.c_double
    drv.conc_calls_run.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7
    d = int.from_bytes(hashlib.sha256(b"stress").digest(), "big") % (o.N - 1) + 1
    q = o.pubkey(d)
    base = []
    for i in range(32):
        m = b"stress %d" % i + bytes(40)
        r, s = o.ecdsa_sign(d, o.quirk_digest(m))
        base.append((m, o.der_encode_sig(r, s)))
    n = 64 * 512  # ~0.4 M calls in all, ~1 s: enough to see a 1-in-10^4 ordering race
    msgs, tags, want = [], [], []
    for k in range(n):
        m, t = base[k % 32]
        if k % 5 == 3:
            m = b"#" + m[1:]  # tampered inside e: rejected
        msgs.append(m)
        tags.append(t)
        want.append(0 if k % 5 != 3 else 1)
    role = np.full(n, ROLE_CLIENT, dtype=np.uint32)
    ids = np.zeros(n, dtype=np.uint32)
    mbuf = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    tbuf = np.frombuffer(b"".join(tags), dtype=np.uint8).copy()
    moff = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    toff = np.concatenate([[0], np.cumsum([len(t) for t in tags])]).astype(np.uint64)
    a = Authenticator(0)
    try:
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
        a.set_concurrency(4)
        a.set_coalescing(True)
        fn = ctypes.cast(a.lib.mbft_verify_message_authen_tag, ctypes.c_void_p).value
        for threads, slots in ((64, 64), (16, 16), (64, 16)):
            a.set_resident(slots)
            for _ in range(4):
                rc = np.full(n, -99, dtype=np.int32)
                drv.conc_calls_run(fn, a.ctx, threads, n // threads, role.ctypes.data, ids.ctypes.data,
                                   mbuf.ctypes.data, moff.ctypes.data, tbuf.ctypes.data, toff.ctypes.data,
                                   rc.ctypes.data)
                bad = np.nonzero(rc != np.array(want))[0]
                assert not len(bad), (threads, slots, [(int(i), int(rc[i]), want[i]) for i in bad[:8]])
            a.set_resident(0)
    finally:
        a.close()


def test_null_stream_not_held_by_live_resident_kernel(lib, monkeypatch):
    """The resident kernel's stream is non-blocking (lowest priority, its own
    hardware queue), so null-stream work -- a synchronous copy on torch's
    default stream, the library's key-map upload -- does not wait for the
    live generation (the CU-masked stream was blocking, so such a
    copy waited up to the kernel's idle exit).  The generation is kept alive
    (idle exit 300 ms) while both are timed."""
    import torch
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT, flat_calls
    from oracle import p256 as o
    monkeypatch.setenv("MBFT_RESIDENT_IDLE_US", "300000")
    monkeypatch.setenv("MBFT_RESIDENT_LIFE_MS", "600")
    d = 4242
    q = o.pubkey(d)
    msg = b"null stream" + bytes(30)
    r, s = o.ecdsa_sign(d, o.quirk_digest(msg))
    tag = o.der_encode_sig(r, s)
    a = Authenticator(0)
    try:
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
        a.set_resident(4)
        assert a.verify_status(ROLE_CLIENT, 0, msg, tag) == 0  # the generation is live now
        host = torch.arange(1 << 16, dtype=torch.int32)
        t0 = time.perf_counter()
        dev = host.to("cuda:0")  # null stream
        torch.cuda.default_stream(0).synchronize()
        copy_s = time.perf_counter() - t0
        assert torch.equal(dev.cpu(), host)
        # a new key: the next device-decoded batch re-uploads the key map
        d2 = 777
        q2 = o.pubkey(d2)
        a.set_public_key(ROLE_CLIENT, 1, q2[0].to_bytes(32, "big") + q2[1].to_bytes(32, "big"))
        r2, s2 = o.ecdsa_sign(d2, o.quirk_digest(msg))
        flat = flat_calls([(ROLE_CLIENT, 1, msg, o.der_encode_sig(r2, s2))] * 4096, True, compact=True)
        assert a.verify_status(ROLE_CLIENT, 1, msg, o.der_encode_sig(r2, s2)) == 0  # relaunched, live again
        t0 = time.perf_counter()
        out = a.verify_flat32_arrays(*flat, pinned=True)  # first device-decoded batch: grows its staging
        batch_s = time.perf_counter() - t0
        st = a.resident_stats()
    finally:
        a.close()
    assert list(np.asarray(out)) == [0] * 4096
    assert st["own_queue"], st
    assert copy_s < 0.1, copy_s
    assert batch_s < 0.1, batch_s
