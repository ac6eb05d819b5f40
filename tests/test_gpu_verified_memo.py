"""The verified-call memo (mbft_set_verified_memo) through the
C-ABI: two contexts, one with the memo and one without, over the same
messages.  Every validator result is compared between them and with
oracle.validate_messages, and the memo's counters say what was looked up, hit,
inserted.  mbft_set_small_check(ctx, 0): every pass takes the device route.

The memo is sized so that the CPU model (the `bucket` command of
tests/memo_plan_check over the test's own tuples) shows no run of P full
entries possible; that is asserted first, then dropped == 0.
"""
import copy
import hashlib
import random
import struct
import subprocess
import threading

import numpy as np
import pytest

from test_gpu_configs import _fast_oracle
from test_gpu_msgdev import _auth_for, _check_resolve

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
NREP = 4
MEMO = 4 << 20  # two generations of 16,384 entries
CLIENT = 7


def _key(tag):
    from oracle import p256 as o
    d = int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big") % (o.N - 1) + 1
    return d, o.pubkey(d)


class World:
    """A 4-replica system: USIG keys of the replicas, one client key, random
    epochs, and the contexts over them."""

    def __init__(self, tag, rng):
        from oracle import p256 as o
        self.o = o
        self.usig = {i: _key(f"{tag} usig {i}") for i in range(NREP)}
        self.cli = _key(f"{tag} client")
        self.epoch = {i: rng.randrange(1, 1 << 64) for i in range(NREP)}
        self.ctr = {i: 0 for i in range(NREP)}
        self.keys = {o.ROLE_USIG: {i: q for i, (_, q) in self.usig.items()}, o.ROLE_CLIENT: {CLIENT: self.cli[1]}}
        self.seq = 0

    def oracle(self):
        ks = self.o.KeyStore()
        ks.keys = {role: dict(m) for role, m in self.keys.items()}
        return self.o.Authenticator(ks)

    def contexts(self, memo=MEMO):
        a, b = _auth_for(self.keys, window=8), _auth_for(self.keys, window=8)
        for x in (a, b):
            x.set_small_check(0)
        if memo:
            a.set_verified_memo(memo)
        return a, b

    def request(self, rng, op=None):
        o = self.o
        self.seq += 1
        rq = o.Msg(type=o.MSG_REQUEST, stream=1000, client_id=CLIENT, seq=self.seq, op=op or rng.randbytes(64))
        rq.sig = o.der_encode_sig(*o.ecdsa_sign(self.cli[0], o.quirk_digest(o.msg_authen_bytes(rq))))
        return rq

    def prepare(self, rq, counter=None, epoch=None):
        o = self.o
        if counter is None:
            self.ctr[0] += 1
            counter = self.ctr[0]
        pr = o.Msg(type=o.MSG_PREPARE, stream=0, replica_id=0, view=0, client_id=CLIENT, seq=rq.seq, op=rq.op,
                   sig=rq.sig, ui_counter=counter)
        pr.ui_cert = o.usig_create_ui(self.usig[0][0], o.msg_authen_bytes(pr), self.epoch[0] if epoch is None else epoch,
                                      counter)[8:]
        return pr

    def commit(self, pr, rid):
        o = self.o
        self.ctr[rid] += 1
        cm = o.Msg(type=o.MSG_COMMIT, stream=rid, replica_id=rid, prep_replica_id=0, view=0, client_id=CLIENT,
                   seq=pr.seq, op=pr.op, sig=pr.sig, prep_ui_counter=pr.ui_counter, prep_ui_cert=pr.ui_cert,
                   ui_counter=self.ctr[rid])
        cm.ui_cert = o.usig_create_ui(self.usig[rid][0], o.msg_authen_bytes(cm), self.epoch[rid], self.ctr[rid])[8:]
        return cm


def calls_of(o, m):
    """The authenticator calls the validators make for one message, as
    (role, id, authen bytes, counter, tag): core/prepare.go:55, core/commit.go:82."""
    rq = (o.ROLE_CLIENT, m.client_id, o.msg_authen_bytes(m, o.MSG_REQUEST), None, m.sig)
    if m.type == o.MSG_REQUEST:
        return [rq]
    if m.type == o.MSG_PREPARE:
        return [rq, (o.ROLE_USIG, m.replica_id, o.msg_authen_bytes(m, o.MSG_PREPARE), m.ui_counter, m.ui_cert)]
    return [rq, (o.ROLE_USIG, m.prep_replica_id, o.msg_authen_bytes(m, o.MSG_PREPARE), m.prep_ui_counter, m.prep_ui_cert),
            (o.ROLE_USIG, m.replica_id, o.msg_authen_bytes(m), m.ui_counter, m.ui_cert)]


def tuple_words(o, a, call):
    """A call's memo tuple: slot, then e, r, s as they lie in the batch."""
    role, id_, ab, ctr, tag = call
    if ctr is None:
        e, sig = o.quirk_digest(ab)[:32], tag
    else:
        e, sig = o.usig_digest(ab, struct.unpack(">Q", tag[:8])[0], ctr), tag[8:]
    r, s, _ = o.der_parse_sig(sig)
    raw = e + r.to_bytes(32, "big") + s.to_bytes(32, "big")
    return (a.key_slot(role, id_),) + struct.unpack("<24I", raw)


def unique_calls(o, msgs):
    seen = {}
    for m in msgs:
        for c in calls_of(o, m):
            seen.setdefault((c[0], c[1], c[2], c[3], c[4]), c)
    return list(seen.values())


def assert_model_has_room(a, tuples):
    """No run of P full entries can form whatever the insert order: a run
    [b, b + P) is filled from homes in [b - P + 1, b + P), so every span of
    2P - 1 buckets must hold fewer than P of the tuples' homes."""
    import __graft_entry__ as ge
    prog = ge.build_memo_check_host()
    entries = a.verified_memo() // 256
    lines = ["consts"] + [f"bucket {entries} " + " ".join(map(str, t)) for t in tuples]
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True)
    out = p.stdout.split("\n")[:-1]
    P = int(out[0].split()[2])
    homes = np.array([int(x.split()[0]) for x in out[1:]], dtype=np.int64)
    cnt = np.bincount(homes, minlength=entries)
    cs = np.concatenate([[0], np.cumsum(np.concatenate([cnt, cnt[:2 * P - 2]]))])
    assert int((cs[2 * P - 1:] - cs[:-(2 * P - 1)]).max()) < P


def delta(a, before):
    now = a.verified_memo_stats()
    return {k: now[k] - before[k] for k in now}, now


def assert_same_usage(a, b, rejects_at_least):
    """Uses AND rejects per key are the same with the memo on or off."""
    ua, ub = a.key_usage(n=NREP + 1), b.key_usage(n=NREP + 1)
    assert np.array_equal(ua[0], ub[0]) and np.array_equal(ua[1], ub[1]), (ua, ub)
    assert int(ua[1].sum()) >= rejects_at_least and int(ua[0].sum()) > int(ua[1].sum())


def flags(o):
    return o.VF_NO_STREAM_STOP | o.VF_NO_PANIC_STOP


def run_pass(o, a, b, ref, msgs):
    """One pass on both contexts and the oracle; the results, all equal."""
    got_a, got_b = _check_resolve(a, msgs, NREP), _check_resolve(b, msgs, NREP)
    want = np.array(o.validate_messages(ref, msgs, NREP, flags(o)))
    assert (got_b == want).all(), np.nonzero(got_b != want)[0][:10]
    assert (got_a == want).all(), np.nonzero(got_a != want)[0][:10]
    return want


def test_protocol_shape_three_passes(lib, monkeypatch):
    """REQUESTs, then PREPAREs, then COMMITs, as they would arrive: in passes 2
    and 3 the embedded calls earlier passes accepted are hits, lookups - hits is
    the new signatures only (the one-wait form: 8, 8 and 24 messages).  Then
    the whole stream twice: every accepted call a hit, nothing new inserted."""
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E30)
    w = World("memo shape", rng)
    reqs = [w.request(rng) for _ in range(8)]
    preps = [w.prepare(rq) for rq in reqs]
    commits = [w.commit(pr, rid) for pr in preps for rid in (1, 2, 3)]
    assert len(reqs + preps + commits) == 40
    a, b = w.contexts()
    try:
        for x in (a, b):
            x.set_key_accounting(True)
        assert a.verified_memo() == MEMO and b.verified_memo() == 0
        assert_model_has_room(a, [tuple_words(o, a, c) for c in unique_calls(o, reqs + preps + commits)])
        ref = w.oracle()
        st = a.verified_memo_stats()
        assert st == dict.fromkeys(st, 0)
        for msgs, lookups, hits in ((reqs, 8, 0), (preps, 16, 8), (commits, 40, 16)):
            assert (run_pass(o, a, b, ref, msgs) == 0).all()
            d, st = delta(a, st)
            assert (d["lookups"], d["hits"], d["inserts"], d["dropped"]) == (lookups, hits, lookups - hits, 0)
        stream = [m for k in range(8) for m in [reqs[k], preps[k]] + commits[3 * k:3 * k + 3]]
        for _ in range(2):
            assert (run_pass(o, a, b, ref, stream) == 0).all()
            d, st = delta(a, st)
            assert (d["lookups"], d["hits"], d["inserts"], d["dropped"]) == (40, 40, 0, 0)
        assert st["rotations"] == 0 and st["clears"] == 0
        ua, ub = a.key_usage(n=NREP + 1), b.key_usage(n=NREP + 1)  # the use counts do not see the memo
        assert np.array_equal(ua[0], ub[0]) and np.array_equal(ua[1], ub[1]) and int(ua[0].sum()) == 8 + 16 + 40 + 80
        zero = b.verified_memo_stats()
        assert zero == dict.fromkeys(zero, 0)  # off means off
    finally:
        a.close()
        b.close()


def _gpu_signed_requests(o, a, w, rng, count):
    """`count` distinct REQUESTs signed by the batch signer (Python's signer
    takes 7 ms a message)."""
    from minbft_amd.authenticator import Authenticator
    out = []
    for _ in range(count):
        w.seq += 1
        out.append(o.Msg(type=o.MSG_REQUEST, stream=1000, client_id=CLIENT, seq=w.seq, op=rng.randbytes(24)))
    tags, lens = a.generate_tags(o.ROLE_CLIENT, [o.msg_authen_bytes(m) for m in out])
    for m, t in zip(out, Authenticator.tag_bytes(tags, lens)):
        m.sig = t
    return out


def _tamper(m):
    t = copy.copy(m)
    sig = bytearray(t.sig)
    sig[-1] ^= 1
    t.sig = bytes(sig)
    return t


def test_host_read_back_route(lib, monkeypatch):
    """5,000 distinct REQUESTs are more than MBFT_LANE_INV_MAX unique calls: the
    large form over the compacted arrays.  The same 5,000 and 100 new: 100
    misses, planned again.  4,500 new and 500 old: large again.  The memo-less
    context gives the same results throughout; the oracle is asked about
    every tampered message and every eighth of the others."""
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E31)
    w = World("memo large", rng)
    a, b = w.contexts(memo=128 << 20)  # 9,090 tuples in 524,288 entries a generation
    try:
        for x in (a, b):
            x.set_key_accounting(True)
        a.set_private_key(o.ROLE_CLIENT, w.cli[0].to_bytes(32, "big"))
        first = _gpu_signed_requests(o, a, w, rng, 5000)
        new100 = _gpu_signed_requests(o, a, w, rng, 100)
        new4500 = _gpu_signed_requests(o, a, w, rng, 4500)
        bad100, bad4500 = set(range(0, 100, 10)), set(range(0, 4500, 9))
        new100 = [_tamper(m) if i in bad100 else m for i, m in enumerate(new100)]
        new4500 = [_tamper(m) if i in bad4500 else m for i, m in enumerate(new4500)]
        good = [m for i, m in enumerate(new100) if i not in bad100] + [m for i, m in enumerate(new4500) if i not in bad4500]
        assert_model_has_room(a, [tuple_words(o, a, calls_of(o, m)[0]) for m in first + good])
        ref = w.oracle()
        st = a.verified_memo_stats()
        passes = ((first, set(), 5000, 0), (first + new100, {5000 + i for i in bad100}, 5100, 5000),
                  (new4500 + first[:500], bad4500, 5000, 500))
        for msgs, bad, lookups, hits in passes:
            got_a, got_b = _check_resolve(a, msgs, NREP), _check_resolve(b, msgs, NREP)
            assert np.array_equal(got_a, got_b)
            assert np.array_equal(np.nonzero(got_a)[0], np.array(sorted(bad), dtype=np.int64))
            ask = sorted(bad | set(range(0, len(msgs), 8)))
            want = o.validate_messages(ref, [msgs[i] for i in ask], NREP, flags(o))
            assert [int(got_a[i]) for i in ask] == want
            d, st = delta(a, st)
            assert (d["lookups"], d["hits"], d["dropped"]) == (lookups, hits, 0)
            assert d["inserts"] == lookups - hits - len(bad)  # rejects are not remembered
        assert_same_usage(a, b, rejects_at_least=10 + 500)
    finally:
        a.close()
        b.close()


def test_not_a_hit_and_rejects_not_remembered(lib, monkeypatch):
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E32)
    w = World("memo near", rng)
    rq = w.request(rng)
    pr = w.prepare(rq)
    a, b = w.contexts()
    try:
        for x in (a, b):
            x.set_key_accounting(True)
        ref = w.oracle()
        assert (run_pass(o, a, b, ref, [rq, pr]) == 0).all()
        _, st = delta(a, a.verified_memo_stats())
        assert st["inserts"] == 2
        # one bit of the signature, of the message (the sequence number: bytes 7..14 of e), of the counter
        sig_bit = _tamper(rq)
        msg_bit = copy.copy(rq)
        msg_bit.seq ^= 1
        ctr_bit = copy.copy(pr)
        ctr_bit.ui_counter ^= 2
        near = [sig_bit, msg_bit, ctr_bit]
        want = run_pass(o, a, b, ref, near)
        assert (want != 0).all()
        d, st = delta(a, st)
        # (the PREPARE's embedded REQUEST is the remembered one: the only hit)
        assert (d["lookups"], d["hits"], d["inserts"]) == (4, 1, 0)
        # rejected calls are looked up and verified again, every time
        run_pass(o, a, b, ref, near)
        d, st = delta(a, st)
        assert (d["lookups"], d["hits"], d["inserts"]) == (4, 1, 0)
        # the high-s twin (r, N - s) is another tuple: a miss, verified, accepted, remembered
        r, s, _ = o.der_parse_sig(rq.sig)
        twin = copy.copy(rq)
        twin.sig = o.der_encode_sig(r, N_ORDER - s)
        assert (run_pass(o, a, b, ref, [twin]) == 0).all()
        d, st = delta(a, st)
        assert (d["lookups"], d["hits"], d["inserts"]) == (1, 0, 1)
        assert (run_pass(o, a, b, ref, [twin, rq]) == 0).all()
        d, st = delta(a, st)
        assert (d["lookups"], d["hits"], d["inserts"], st["dropped"]) == (2, 2, 0, 0)
        assert_same_usage(a, b, rejects_at_least=6)  # (three rejected calls, sent twice; hits are uses like any)
    finally:
        a.close()
        b.close()


def test_epoch_step_untouched(lib, monkeypatch):
    """The situations of tests/golden/usig_epoch.json (a rejected UI that
    captures nothing, counter != 1 before a capture, the capture, a mismatch
    after it) as PREPAREs -- the golden file's calls are raw authenticator
    calls, which the message layer cannot carry.  A first check that is never
    resolved remembers the signatures and captures no epoch; the second is
    resolved message by message with every accepted signature a hit."""
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E33)
    w = World("memo epoch", rng)
    rqs = [w.request(rng) for _ in range(5)]
    E = w.epoch[0]
    broken = w.prepare(rqs[0], counter=1)
    broken.ui_cert = broken.ui_cert[:-1] + bytes([broken.ui_cert[-1] ^ 1])
    msgs = [broken, w.prepare(rqs[1], counter=2), w.prepare(rqs[2], counter=1), w.prepare(rqs[3], counter=2),
            w.prepare(rqs[4], counter=3, epoch=E ^ 1)]
    a, b = w.contexts()
    try:
        from minbft_amd import _lib
        arr, keep = _lib.make_messages(msgs)
        packed = np.frombuffer(arr, dtype=_lib.message_dtype(), count=len(msgs))
        recs, arena = a.pack_messages(packed, True)
        with a.check_messages_flat(recs, arena, NREP):
            pass  # checked, never resolved
        del keep
        _, st = delta(a, a.verified_memo_stats())
        assert (st["lookups"], st["hits"], st["inserts"]) == (10, 0, 9)
        ref = w.oracle()
        want = run_pass(o, a, b, ref, msgs)
        assert [int(x) & 0xFF for x in want] == [o.REJECT_SIG, o.EPOCH_MISMATCH, o.ACCEPT, o.ACCEPT, o.EPOCH_MISMATCH]
        d, st = delta(a, st)
        assert (d["lookups"], d["hits"], d["inserts"]) == (10, 9, 0)
    finally:
        a.close()
        b.close()


def test_slot_reuse_clears_and_reclass_keeps(lib, monkeypatch):
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E34)
    w = World("memo slots", rng)
    msgs = [w.request(rng) for _ in range(6)]
    a, b = w.contexts()
    try:
        ref = w.oracle()
        assert (run_pass(o, a, b, ref, msgs) == 0).all()
        st = a.verified_memo_stats()
        assert (st["inserts"], st["clears"]) == (6, 0)
        # re-classing keeps the point and the memo
        for x in (a, b):
            x.set_key_class(o.ROLE_CLIENT, CLIENT, 0x100 | 4)
        assert (run_pass(o, a, b, ref, msgs) == 0).all()
        d, st = delta(a, st)
        assert (d["hits"], d["inserts"], st["clears"]) == (6, 0, 0)
        # key A leaves, key B takes its slot number: the old tuples must not be accepted under it
        slot = a.key_slot(o.ROLE_CLIENT, CLIENT)
        other = _key("memo slots other client")
        for x in (a, b):
            x.remove_public_key(o.ROLE_CLIENT, CLIENT)
            x.set_public_key(o.ROLE_CLIENT, CLIENT, o.pkix_encode(other[1]))
        assert a.key_slot(o.ROLE_CLIENT, CLIENT) == slot
        w.keys[o.ROLE_CLIENT][CLIENT] = other[1]
        ref = w.oracle()
        want = run_pass(o, a, b, ref, msgs)
        assert [int(x) & 0xFF for x in want] == [o.REJECT_SIG] * 6
        d, st = delta(a, st)
        assert st["clears"] >= 1 and (d["lookups"], d["hits"], d["inserts"]) == (6, 0, 0)
    finally:
        a.close()
        b.close()


def homes_of(a, tuples):
    """The home bucket of every tuple, from the header's own `bucket`."""
    import __graft_entry__ as ge
    entries = a.verified_memo() // 256
    lines = [f"bucket {entries} " + " ".join(map(str, t)) for t in tuples]
    p = subprocess.run([ge.build_memo_check_host()], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=60, check=True)
    return [int(x.split()[0]) for x in p.stdout.split("\n")[:-1]]


def test_rotation(lib, monkeypatch):
    """The minimum memo: 1,024 entries a generation, a rotation due at 768
    unique calls.  Four fills of 400 distinct accepted REQUESTs rotate twice.
    A generation takes two fills, 800 tuples in 1,024 entries, so the fills are
    CHOSEN with the CPU model: from a pool of signed REQUESTs, those whose home
    buckets are all different within their generation -- every insert then finds
    its home empty whatever the order, and nothing can be dropped.  The latest
    fill hits in full; the first fill is gone, verified again, correctly."""
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E35)
    w = World("memo rotate", rng)
    a, b = w.contexts(memo=2 * 1024 * 128)
    try:
        assert a.verified_memo() == 2 * 1024 * 128
        a.set_private_key(o.ROLE_CLIENT, w.cli[0].to_bytes(32, "big"))
        pool = _gpu_signed_requests(o, a, w, rng, 4800)
        homes = homes_of(a, [tuple_words(o, a, calls_of(o, m)[0]) for m in pool])
        gens, taken = [[], []], [set(), set()]
        for m, h in zip(pool, homes):  # generation 0 first, then generation 1, each 800 different homes
            g = 0 if len(gens[0]) < 800 else 1
            if len(gens[g]) < 800 and h not in taken[g]:
                taken[g].add(h)
                gens[g].append(m)
        assert len(gens[0]) == len(gens[1]) == 800  # (the model: no two tuples of a generation share a home)
        fills = [gens[0][:400], gens[0][400:], gens[1][:400], gens[1][400:]]
        st = a.verified_memo_stats()
        for k, msgs in enumerate(fills):
            assert not _check_resolve(a, msgs, NREP).any()
            d, st = delta(a, st)
            assert (d["lookups"], d["hits"], d["inserts"], d["dropped"]) == (400, 0, 400, 0)
            assert st["rotations"] == (k + 1) // 2
        assert st["rotations"] == 2
        for msgs, hits in ((fills[3], 400), (fills[0], 0)):
            got_a, got_b = _check_resolve(a, msgs, NREP), _check_resolve(b, msgs, NREP)
            assert not got_a.any() and not got_b.any()
            d, st = delta(a, st)
            assert (d["lookups"], d["hits"], d["dropped"]) == (400, hits, 0)
        ref = w.oracle()
        assert o.validate_messages(ref, fills[0][::16], NREP, flags(o)) == [0] * 25
    finally:
        a.close()
        b.close()


def test_two_lanes_at_once(lib, monkeypatch):
    from oracle import p256 as o
    _fast_oracle(monkeypatch)
    rng = random.Random(0x3E36)
    w = World("memo lanes", rng)
    a, b = w.contexts()
    try:
        a.set_private_key(o.ROLE_CLIENT, w.cli[0].to_bytes(32, "big"))
        pool = _gpu_signed_requests(o, a, w, rng, 600)
        pool = [_tamper(m) if i % 7 == 0 else m for i, m in enumerate(pool)]
        want = np.array(o.validate_messages(w.oracle(), pool, NREP, flags(o)))
        a.set_concurrency(2)
        sets = [[list(range(0, 400)), list(range(200, 600)), list(range(0, 600, 2))],
                [list(range(100, 500)), list(range(0, 400)), list(range(1, 600, 2)) + list(range(0, 100, 2))]]
        errs = []

        def worker(t):
            try:
                for idx in sets[t]:
                    got = _check_resolve(a, [pool[i] for i in idx], NREP)
                    if not np.array_equal(got, want[idx]):
                        errs.append((t, np.nonzero(got != want[idx])[0][:5]))
            except Exception as e:  # noqa: BLE001
                errs.append((t, repr(e)))

        th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        st = a.verified_memo_stats()
        assert 0 < st["hits"] <= st["lookups"] == sum(len(i) for s in sets for i in s)
        assert np.array_equal(_check_resolve(b, pool, NREP), want)
    finally:
        a.close()
        b.close()


def test_off_means_off_and_memory_returns(lib):
    import torch
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    with Authenticator(0) as a:
        assert a.lib.mbft_set_verified_memo(a.ctx, 2 * 1024 * 128 - 1) == _lib.ERR_ARG and a.verified_memo() == 0
        a.set_verified_memo(1 << 20)  # (the first use of anything is out of the way)
        a.set_verified_memo(0)
        torch.cuda.synchronize()
        free0, mem0 = torch.cuda.mem_get_info(0)[0], a.key_memory()
        a.set_verified_memo((96 << 20) + 12345)
        assert a.verified_memo() == 64 << 20
        assert torch.cuda.mem_get_info(0)[0] <= free0 - (64 << 20)
        a.clear_verified_memo()
        assert a.verified_memo_stats()["clears"] == 1
        a.set_verified_memo(0)
        assert a.verified_memo() == 0 and a.key_memory() == mem0
        # back where it was: memory the memo kept would show as less (others on the device may free meanwhile)
        assert torch.cuda.mem_get_info(0)[0] >= free0
        st = a.verified_memo_stats()
        assert st == dict.fromkeys(st, 0)
