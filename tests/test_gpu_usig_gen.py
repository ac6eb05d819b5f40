"""The software USIG (mbft_usig_*, k_usig_uis) through the C-ABI against the
oracle: every UI byte for byte oracle.usig_create_ui(d, m, epoch, counter),
the identity, the round trip through the verifier, and the counter contract
(DESIGN.md 4.6).

The oracle signs at ~11 ms a signature, so its side is computed once per
module: 387 UIs (1 + 64 + 65 + 257: the four batch sizes back to back, counters
1..387, so the counter's second byte is exercised) over messages of the lengths
at which SHA-256's padding changes shape."""
import ctypes
import hashlib
import random
import threading

import numpy as np
import pytest

from oracle import p256 as o

pytestmark = pytest.mark.gpu

REPLICA, USIG, CLIENT = 1, 2, 3
ERR_ARG, ERR_KEY, ERR_STATE = -1, -4, -5
NO_STREAM_STOP = 1
EPOCH = 0x0102030405060708
D = 0x6B9D3DAD2E1B8C1C05B19875B6659F4DE23C3B667BF297BA9AA47740787137D8 % o.N
LENGTHS = [0, 55, 56, 63, 64, 119, 120]
SIZES = [1, 64, 65, 257]
TOTAL = sum(SIZES)


def _dbytes(d=D):
    return d.to_bytes(32, "big")


@pytest.fixture(scope="module")
def expected():
    """(msgs, uis): message i is signed under counter i + 1."""
    rng = random.Random(0x0516)
    msgs = [rng.randbytes(LENGTHS[i % len(LENGTHS)] if i % 3 else rng.randrange(0, 200)) for i in range(TOTAL)]
    for i, n in enumerate(LENGTHS):  # every listed length at least once, whatever the mix above
        msgs[2 + i] = rng.randbytes(n)
    return msgs, [o.usig_create_ui(D, m, EPOCH, i + 1) for i, m in enumerate(msgs)]


def _new(lib, d=D, epoch=EPOCH, window=None):
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    if window is not None:
        a.set_signer_window(window)
    if d is not None:
        a.usig_init(_dbytes(d), epoch)
    return a


def _verifier(lib, keys, client=None):
    """A context that knows only public keys: {usig id: d}."""
    from minbft_amd.authenticator import Authenticator
    v = Authenticator(0)
    v.add_role(USIG)
    v.enable_usig(True)
    for id_, d in keys.items():
        v.set_public_key(USIG, id_, o.pkix_encode(o.pubkey(d)))
    if client is not None:
        v.add_role(CLIENT)
        v.set_public_key(CLIENT, client[0], o.pkix_encode(o.pubkey(client[1])))
    return v


def _pack(msgs, pinned=False):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    arr, keep = _lib.make_messages(msgs)
    packed = np.frombuffer(arr, dtype=_lib.message_dtype(), count=len(msgs))
    recs, arena = Authenticator.pack_messages(packed, pinned)
    del keep
    return recs, arena


def _check_slots(uis, lens):
    for i in range(len(lens)):
        assert 16 + 8 <= int(lens[i]) <= 88
        assert not uis[i, int(lens[i]):].any()  # the rest of each slot is zeroed


def _sha(msgs):
    return np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), dtype=np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("form", ["digests", "flat"])
def test_parity_and_counter_sequence(lib, expected, form):
    """n = 1, 64, 65, 257 back to back on one instance: counters 1..387."""
    msgs, want = expected
    a = _new(lib)
    try:
        assert a.usig_next_counter() == 1
        at = 0
        for n in SIZES:
            part = msgs[at:at + n]
            if form == "digests":
                uis, lens, first = a.usig_create_uis_digests(_sha(part))
            else:
                uis, lens, first = a.usig_create_uis(part)
            assert first == at + 1
            _check_slots(uis, lens)
            assert a.ui_bytes(uis, lens) == want[at:at + n], (form, n)
            at += n
            assert a.usig_next_counter() == at + 1
        # n = 0: nothing happens
        uis, lens, first = a.usig_create_uis_digests(np.zeros((0, 32), dtype=np.uint8))
        assert first == TOTAL + 1 and a.usig_next_counter() == TOTAL + 1
    finally:
        a.close()


@pytest.mark.parametrize("w", [4, 5, 6])
def test_signer_windows(lib, expected, w):
    msgs, want = expected
    a = _new(lib, window=w)
    try:
        uis, lens, first = a.usig_create_uis_digests(_sha(msgs[:64]))
        assert first == 1 and a.ui_bytes(uis, lens) == want[:64]
    finally:
        a.close()


def _prepares_commits(n, rng, primary=0, backup=1):
    """n messages, PREPARE and COMMIT mixed, ops of 0, 1 and 256 bytes; a
    COMMIT names a PREPARE of `primary` with some counter."""
    ops = [0, 1, 256]
    out = []
    for i in range(n):
        op = rng.randbytes(ops[i % 3])
        if i % 2 == 0 or i % 7 == 3:
            out.append(o.Msg(type=o.MSG_PREPARE, replica_id=primary, view=rng.randrange(2 ** 64),
                             client_id=rng.randrange(2 ** 32), seq=rng.randrange(2 ** 64), op=op))
        else:
            out.append(o.Msg(type=o.MSG_COMMIT, replica_id=backup, prep_replica_id=rng.randrange(2 ** 32),
                             view=rng.randrange(2 ** 64), client_id=rng.randrange(2 ** 32),
                             seq=rng.randrange(2 ** 64), op=op,
                             prep_ui_counter=rng.randrange(2 ** 64)))
    return out


def test_records_parity(lib):
    rng = random.Random(65)
    msgs = _prepares_commits(65, rng)
    assert {m.type for m in msgs} == {o.MSG_PREPARE, o.MSG_COMMIT}
    assert {(m.type, len(m.op)) for m in msgs} >= {(t, n) for t in (o.MSG_PREPARE, o.MSG_COMMIT)
                                                    for n in (0, 1, 256)}
    recs, arena = _pack(msgs)
    a = _new(lib)
    try:
        uis, lens, first = a.usig_sign_messages_flat(recs, arena)
        assert first == 1 and a.usig_next_counter() == 66
        _check_slots(uis, lens)
        got = a.ui_bytes(uis, lens)
        for i, m in enumerate(msgs):
            assert got[i] == o.usig_create_ui(D, o.msg_authen_bytes(m), EPOCH, i + 1), (i, m.type)
    finally:
        a.close()


def test_identity(lib):
    a = _new(lib)
    try:
        assert a.usig_id() == EPOCH.to_bytes(8, "big") + o.pkix_encode(o.pubkey(D))
        n = ctypes.c_size_t(0)
        buf = ctypes.create_string_buffer(98)
        assert a.lib.mbft_usig_id(a.ctx, buf, 98, ctypes.byref(n)) == ERR_ARG and n.value == 99
    finally:
        a.close()
    for d in (1, o.N - 1):
        a = _new(lib, d=d, epoch=7)
        try:
            assert a.usig_id() == (7).to_bytes(8, "big") + o.pkix_encode(o.pubkey(d))
        finally:
            a.close()


@pytest.mark.parametrize("w", [4, 5, 6])
def test_identity_structured_keys(lib, w):
    """The identity d G (k_sign_pubkey: sign_comb over the table the product
    itself built) for the keys at which the comb's selects change state
    (comb_layout.structured_scalars: a long stay at infinity, carry chains,
    zero runs, the tie digit, the top window alone and its last entry), one
    context per signer window, a fresh epoch per key."""
    from comb_layout import structured_scalars
    from test_gpu_field import golden_module
    mg = golden_module()
    keys = structured_scalars(w, mg.scalar_edge_values(random.Random(0x45444745)))
    a = _new(lib, d=None, window=w)
    try:
        bad = []
        for i, (name, d) in enumerate(keys):
            a.usig_init(_dbytes(d), i)
            if a.usig_id() != i.to_bytes(8, "big") + o.pkix_encode(o.pubkey(d)):
                bad.append(name)
        assert not bad, (len(bad), bad[:10])
    finally:
        a.close()


def test_round_trip_verify_batch(lib, expected):
    """The UIs, in counter order, pass the verifier of a context that knows
    only the public key; the epoch is captured from counter 1."""
    msgs, _ = expected
    a, v = _new(lib), _verifier(lib, {5: D})
    try:
        uis, lens, first = a.usig_create_uis(msgs)
        tags = a.ui_bytes(uis, lens)
        st = v.verify_batch([(USIG, 5, m, t) for m, t in zip(msgs, tags)])
        assert not st.any()
        # a UI does not verify over another message, nor under another counter
        st = v.verify_batch([(USIG, 5, msgs[1], tags[2]),
                             (USIG, 5, msgs[3], (9).to_bytes(8, "big") + tags[3][8:])])
        assert st.tolist() == [1, 1]
    finally:
        a.close()
        v.close()


def test_round_trip_messages(lib):
    """A primary's PREPAREs and a backup's COMMITs, UIs from two USIG
    instances and the embedded REQUESTs signed by mbft_sign_messages_flat,
    validated by a third context: the statuses of oracle.validate_messages.
    Then the primary restarts (new epoch): its new PREPAREs are rejected by the
    verifier that captured the old epoch, as the oracle says."""
    rng = random.Random(3)
    d_p, d_b, d_c = (rng.randrange(1, o.N) for _ in range(3))
    e_p, e_b, e_p2 = 0x1111111111111111, 0x2222222222222222, 0x3333333333333333
    m = 6
    ops = [b"", b"x", rng.randbytes(256), rng.randbytes(40), b"", rng.randbytes(256)]
    reqs = [o.Msg(type=o.MSG_REQUEST, client_id=9, seq=100 + i, op=ops[i]) for i in range(m)]
    prim, back = _new(lib, d_p, e_p), _new(lib, d_b, e_b)
    v = _verifier(lib, {0: d_p, 1: d_b}, client=(9, d_c))
    model = o.Authenticator(o.KeyStore(keys={USIG: {0: o.pubkey(d_p), 1: o.pubkey(d_b)},
                                             CLIENT: {9: o.pubkey(d_c)}}))
    try:
        prim.set_private_key(CLIENT, d_c.to_bytes(32, "big"))
        sigs = prim.tag_bytes(*prim.sign_messages_flat(*_pack(reqs)))

        def prepares(auth):
            ps = [o.Msg(type=o.MSG_PREPARE, stream=0, replica_id=0, view=3, client_id=9, seq=r.seq, op=r.op,
                        sig=s) for r, s in zip(reqs, sigs)]
            uis, lens, first = auth.usig_sign_messages_flat(*_pack(ps))
            for i, (p, ui) in enumerate(zip(ps, auth.ui_bytes(uis, lens))):
                p.ui_counter, p.ui_cert = first + i, ui[8:]
                assert int.from_bytes(ui[:8], "big") == first + i
            return ps

        preps = prepares(prim)
        coms = [o.Msg(type=o.MSG_COMMIT, stream=1, replica_id=1, prep_replica_id=0, view=3, client_id=9,
                      seq=p.seq, op=p.op, sig=p.sig, prep_ui_counter=p.ui_counter, prep_ui_cert=p.ui_cert)
                for p in preps]
        uis, lens, first = back.usig_sign_messages_flat(*_pack(coms))
        for i, (c, ui) in enumerate(zip(coms, back.ui_bytes(uis, lens))):
            c.ui_counter, c.ui_cert = first + i, ui[8:]
        # one PREPARE and one COMMIT altered after signing
        preps[4].op = b"altered"
        coms[2].prep_ui_counter += 1
        batch = preps + coms
        got = v.validate_messages_via_flat(batch, 3, NO_STREAM_STOP)
        want = o.validate_messages(model, batch, 3, NO_STREAM_STOP)
        assert got.tolist() == want
        # (COMMIT 4 embeds the PREPARE as it was signed: valid)
        assert [i for i, w in enumerate(want) if w] == [4, m + 2]
        # the primary restarts: a new instance, a new epoch, counters from 1
        prim.usig_init(d_p.to_bytes(32, "big"), e_p2)
        assert prim.usig_next_counter() == 1
        again = prepares(prim)
        got = v.validate_messages_via_flat(again, 3, NO_STREAM_STOP)
        want = o.validate_messages(model, again, 3, NO_STREAM_STOP)
        assert got.tolist() == want
        assert all(w == (o.ST_PREPARE_UI << 8 | o.EPOCH_MISMATCH) for w in want)
    finally:
        prim.close()
        back.close()
        v.close()


def test_counter_contract_errors(lib):
    msgs = [o.Msg(type=o.MSG_PREPARE, view=1, client_id=2, seq=3, op=b"abc"),
            o.Msg(type=o.MSG_COMMIT, replica_id=1, view=1, client_id=2, seq=3, op=b"abcd", prep_ui_counter=1),
            o.Msg(type=o.MSG_PREPARE, view=1, client_id=2, seq=4, op=b"")]
    recs, arena = _pack(msgs)
    a = _new(lib, d=None)
    try:
        uis = np.full((3, 88), 0x5A, dtype=np.uint8)
        lens = np.full(3, 0x5A, dtype=np.uint8)
        dg = np.zeros((3, 32), dtype=np.uint8)
        off = np.array([0, 1, 2, 3], dtype=np.uint32)
        first = ctypes.c_uint64(77)
        cnt = ctypes.c_uint64(77)

        def records(r, nbytes=None):
            return a.lib.mbft_usig_sign_messages_flat(a.ctx, r.ctypes.data, len(r), arena.ctypes.data,
                                                      arena.nbytes if nbytes is None else nbytes,
                                                      uis.ctypes.data, lens.ctypes.data, ctypes.byref(first))

        def digests():
            return a.lib.mbft_usig_create_uis_digests(a.ctx, dg.ctypes.data, 3, uis.ctypes.data,
                                                      lens.ctypes.data, ctypes.byref(first))

        def flat():
            return a.lib.mbft_usig_create_uis_flat(a.ctx, arena.ctypes.data, off.ctypes.data, 3,
                                                   uis.ctypes.data, lens.ctypes.data, ctypes.byref(first))

        def untouched():
            return (uis == 0x5A).all() and (lens == 0x5A).all() and first.value == 77

        def every_call_is(rc):
            n = ctypes.c_size_t(0)
            buf = ctypes.create_string_buffer(99)
            assert records(recs) == rc and digests() == rc and flat() == rc
            assert a.lib.mbft_usig_next_counter(a.ctx, ctypes.byref(cnt)) == rc
            assert a.lib.mbft_usig_id(a.ctx, buf, 99, ctypes.byref(n)) == rc
            assert untouched()

        every_call_is(ERR_STATE)  # before init
        # a key from mbft_set_private_key is not an instance
        a.set_private_key(USIG, _dbytes())
        every_call_is(ERR_STATE)
        # refused keys
        for bad in (0, o.N, o.N + 1, 2 ** 256 - 1):
            assert a.lib.mbft_usig_init(a.ctx, bad.to_bytes(32, "big"), 5) == ERR_KEY
        every_call_is(ERR_STATE)
        a.usig_init(_dbytes(), 5)
        assert a.usig_next_counter() == 1
        # a REQUEST (or a REPLY, or an unknown type) anywhere: nothing written, the counter untouched
        for bad_type, pos in ((o.MSG_REQUEST, 1), (o.MSG_REPLY, 0), (o.MSG_REQ_VIEW_CHANGE, 2), (9, 2)):
            bad = recs.copy()
            bad[pos]["type"] = bad_type
            assert records(bad) == ERR_ARG
            assert untouched() and a.usig_next_counter() == 1
        out = recs.copy()  # a field that leaves the arena
        out[1]["op_off"] = arena.nbytes - 3
        assert records(out) == ERR_ARG
        out = recs.copy()
        out[0]["op_len"] = 2 ** 32 - 1
        assert records(out) == ERR_ARG
        assert records(recs, nbytes=arena.nbytes - 1) == ERR_ARG
        assert untouched() and a.usig_next_counter() == 1
        assert records(recs) == 0 and first.value == 1 and lens.all()
        assert a.usig_next_counter() == 4
        # the same epoch again is refused and the instance goes on
        assert a.lib.mbft_usig_init(a.ctx, _dbytes(), 5) == ERR_STATE
        assert a.usig_next_counter() == 4
        # the batch generators keep refusing the role
        tags = np.zeros((3, 72), dtype=np.uint8)
        tl = np.zeros(3, dtype=np.uint8)
        assert a.lib.mbft_generate_tags_prehashed(a.ctx, USIG, dg.ctypes.data, 3, tags.ctypes.data,
                                                  tl.ctypes.data) == ERR_STATE
        # mbft_clear_keys drops the instance; the next one needs a fresh epoch
        a.clear_keys()
        uis[:], lens[:], first.value = 0x5A, 0x5A, 77
        every_call_is(ERR_STATE)
        assert a.lib.mbft_usig_init(a.ctx, _dbytes(), 5) == ERR_STATE
        every_call_is(ERR_STATE)
        a.usig_init(_dbytes(), 6)
        assert a.usig_next_counter() == 1
        assert digests() == 0 and first.value == 1
    finally:
        a.close()


def test_threads_share_one_counter(lib):
    """4 threads x 8 calls x 33 items on one context: every call's range is
    contiguous, the union is exactly 1..1056, and every UI verifies."""
    T, C, K = 4, 8, 33
    rng = random.Random(1056)
    a, v = _new(lib), _verifier(lib, {0: D})
    calls = {}
    errors = []

    def worker(t):
        try:
            for c in range(C):
                msgs = [bytes([t, c, k]) + b"-msg" for k in range(K)]
                uis, lens, first = a.usig_create_uis(msgs)
                calls[(t, c)] = (msgs, a.ui_bytes(uis, lens), first)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    try:
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert len(calls) == T * C
        seen = {}
        for (t, c), (msgs, tags, first) in calls.items():
            for k, (m, tag) in enumerate(zip(msgs, tags)):
                ctr = int.from_bytes(tag[:8], "big")
                assert ctr == first + k  # contiguous within the call
                assert ctr not in seen
                seen[ctr] = (m, tag)
        assert sorted(seen) == list(range(1, T * C * K + 1))
        assert a.usig_next_counter() == T * C * K + 1
        order = sorted(seen)
        rng.shuffle(order)
        order.remove(1)
        order.insert(0, 1)  # counter 1 first: the verifier captures the epoch from it
        st = v.verify_batch([(USIG, 0, seen[k][0], seen[k][1]) for k in order])
        assert not st.any()
    finally:
        a.close()
        v.close()


def test_single_call(lib):
    from minbft_amd.authenticator import Authenticator
    msg = o.authen_prepare(4, 9, 17, b"single")
    with Authenticator(0) as a:
        out = ctypes.create_string_buffer(96)
        n = ctypes.c_size_t(0)

        def single(cap=96):
            return a.lib.mbft_generate_message_authen_tag(a.ctx, USIG, msg, len(msg), out, cap, ctypes.byref(n))

        assert single() == ERR_STATE
        a.set_private_key(USIG, _dbytes())
        assert single() == ERR_STATE  # as before: that key never signs UIs
        a.usig_init(_dbytes(), EPOCH)
        assert single(87) == ERR_ARG and n.value == 88  # a UI that might not fit is not created
        assert a.usig_next_counter() == 1
        assert a.GenerateMessageAuthenTag(USIG, msg) == o.usig_create_ui(D, msg, EPOCH, 1)
        assert a.GenerateMessageAuthenTag(USIG, b"") == o.usig_create_ui(D, b"", EPOCH, 2)
        assert a.usig_next_counter() == 3


def test_determinism(lib, expected):
    """Two contexts with the same (d, epoch) produce identical bytes, through
    either input form."""
    msgs, want = expected
    a, b = _new(lib), _new(lib)
    try:
        ua, la, _ = a.usig_create_uis(msgs[:100])
        ub, lb, _ = b.usig_create_uis_digests(_sha(msgs[:100]))
        assert (ua == ub).all() and (la == lb).all()
    finally:
        a.close()
        b.close()


def test_default_epoch_is_random(lib):
    a = _new(lib, d=None)
    try:
        e1 = a.usig_init(_dbytes())
        assert a.usig_id()[:8] == e1.to_bytes(8, "big")
        e2 = a.usig_init(_dbytes())
        assert e1 != e2 and a.usig_id()[:8] == e2.to_bytes(8, "big")
    finally:
        a.close()
