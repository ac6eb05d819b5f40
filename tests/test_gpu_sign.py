"""The batch GenerateMessageAuthenTag (mbft_generate_tags_* /
mbft_sign_messages_flat, k_sign_tags) through the C-ABI against the oracle's
deterministic signer: every tag byte for byte
der_encode_sig(*oracle.ecdsa_sign(d, e)).

The oracle signs at ~11 ms a signature, so its side is computed once per
module: one 321-item batch (256 + 64 + 1: a full block and a tail wave) under
the key of tests/golden/sign_edges.json -- the edge values of e, the four
fixture pairs with a 31-byte r or s, random e -- and 16 items under each of
the other keys (d = 1, N - 1, the reference fixture key, a random one)."""
import base64
import hashlib
import json
import os
import random

import numpy as np
import pytest

from oracle import p256 as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICA, USIG, CLIENT = 1, 2, 3
ERR_ARG, ERR_STATE = -1, -5
NO_PANIC_STOP = 2
EDGE_E = [0, o.N - 1, o.N, o.N + 1, 2 ** 256 - 1]


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _tag(d, e):
    return o.der_encode_sig(*o.ecdsa_sign(d, e))


@pytest.fixture(scope="module")
def expected():
    """{d: (e list, tag list)}; the first key holds the 321-item batch."""
    edges = _golden("sign_edges.json")
    rng = random.Random(321)
    d_main = int(edges[0]["d"], 16)
    sec1 = base64.b64decode(_golden("kat.json")["reference_fixture_key"]["sec1_private_b64"])
    assert sec1[:7] == bytes.fromhex("30770201010420")
    d_ref = int.from_bytes(sec1[7:39], "big")
    out = {}
    es = [v.to_bytes(32, "big") for v in EDGE_E] + [bytes.fromhex(x["e"]) for x in edges]
    es += [rng.randbytes(32) for _ in range(321 - len(es))]
    out[d_main] = (es, [_tag(d_main, e) for e in es])
    assert [t.hex() for t in out[d_main][1][5:9]] == [x["tag"] for x in edges]
    for d in (1, o.N - 1, d_ref, rng.randrange(1, o.N)):
        es = [v.to_bytes(32, "big") for v in EDGE_E] + [rng.randbytes(32) for _ in range(11)]
        out[d] = (es, [_tag(d, e) for e in es])
    return out


@pytest.fixture(scope="module")
def auth(lib):
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    yield a
    a.close()


def _e_arr(es):
    return np.frombuffer(b"".join(es), dtype=np.uint8).reshape(-1, 32)


def test_parity_every_key(auth, expected):
    for d, (es, want) in expected.items():
        auth.set_private_key(REPLICA, d.to_bytes(32, "big"))
        tags, lens = auth.generate_tags_prehashed(REPLICA, _e_arr(es))
        got = auth.tag_bytes(tags, lens)
        assert [int(x) for x in lens] == [len(t) for t in want]
        assert got == want, hex(d)
        for i in range(len(es)):  # the rest of each slot is zeroed
            assert not tags[i, int(lens[i]):].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_parity_small_batches(auth, expected, n):
    d, (es, want) = next(iter(expected.items()))
    auth.set_private_key(CLIENT, d.to_bytes(32, "big"))
    # slices that hold the edge values and the fixture pairs (items 0..8)
    got = auth.tag_bytes(*auth.generate_tags_prehashed(CLIENT, _e_arr(es[:n])))
    assert got == want[:n]
    if n > 1:
        got = auth.tag_bytes(*auth.generate_tags_prehashed(CLIENT, _e_arr(es[321 - n:])))
        assert got == want[321 - n:]


def test_forms_agree(auth, expected):
    import torch
    d, (es, want) = next(iter(expected.items()))
    auth.set_private_key(REPLICA, d.to_bytes(32, "big"))
    n = len(es)
    dev = torch.device("cuda", 0)
    d_e = torch.from_numpy(_e_arr(es).copy()).to(dev)
    d_tags = torch.full((n, 72), 0xAA, dtype=torch.uint8, device=dev)
    d_lens = torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    auth.generate_tags_prehashed_device(REPLICA, d_e.data_ptr(), n, d_tags.data_ptr(), d_lens.data_ptr(), st)
    torch.cuda.synchronize()
    assert auth.tag_bytes(d_tags.cpu().numpy(), d_lens.cpu().numpy()) == want
    # raw messages: e = (m || SHA256(""))[0:32], shorter than 32 bytes included
    rng = random.Random(49)
    msgs = [rng.randbytes(L) for L in (0, 1, 23, 31, 32, 33, 49) for _ in range(3)]
    e_of = [o.quirk_digest(m)[:32] for m in msgs]
    flat = auth.tag_bytes(*auth.generate_tags(REPLICA, msgs))
    pre = auth.tag_bytes(*auth.generate_tags_prehashed(REPLICA, _e_arr(e_of)))
    assert flat == pre
    assert flat == [_tag(d, e) for e in e_of]
    # full-length messages whose first 32 bytes are the batch's e values
    tails = [e + rng.randbytes(rng.randrange(0, 20)) for e in es]
    assert auth.tag_bytes(*auth.generate_tags(REPLICA, tails)) == want


def test_determinism(auth, expected):
    d, (es, want) = next(iter(expected.items()))
    auth.set_private_key(REPLICA, d.to_bytes(32, "big"))
    a1 = auth.generate_tags_prehashed(REPLICA, _e_arr(es))
    a2 = auth.generate_tags_prehashed(REPLICA, _e_arr(es))
    assert (a1[0] == a2[0]).all() and (a1[1] == a2[1]).all()
    # other positions, another batch size: items 100..199 behind 37 others
    rng = random.Random(7)
    shifted = [rng.randbytes(32) for _ in range(37)] + es[100:200]
    got = auth.tag_bytes(*auth.generate_tags_prehashed(REPLICA, _e_arr(shifted)))
    assert got[37:] == want[100:200]


def _records(msgs):
    """mbft_msg_rec array + arena for oracle Msg objects (op only)."""
    from minbft_amd import _lib
    recs = np.zeros(len(msgs), dtype=_lib.msg_rec_dtype())
    arena = bytearray()
    for i, m in enumerate(msgs):
        r = recs[i]
        r["type"], r["replica_id"], r["client_id"] = m.type, m.replica_id, m.client_id
        r["view"], r["seq"] = m.view, m.seq
        r["op_off"], r["op_len"] = len(arena), len(m.op)
        r["sig_off"], r["sig_len"] = 0, len(m.sig)
        arena += m.op
    # signatures behind the ops (the validators read them; the signer does not)
    for i, m in enumerate(msgs):
        recs[i]["sig_off"] = len(arena)
        arena += m.sig
    return recs, np.frombuffer(bytes(arena) + b"\0", dtype=np.uint8)[: len(arena)]


def _mixed(n):
    rng = random.Random(192)
    lens = [0, 1, 55, 56, 64, 256, 1000]
    msgs = []
    for i in range(n):
        t = (o.MSG_REQUEST, o.MSG_REPLY, o.MSG_REQ_VIEW_CHANGE)[i % 3]
        msgs.append(o.Msg(type=t, replica_id=i % 4, client_id=rng.randrange(2 ** 32),
                          view=rng.randrange(2 ** 64), seq=rng.randrange(2 ** 64),
                          op=rng.randbytes(lens[(i // 3) % len(lens)])))
    return msgs


def test_message_layer(auth):
    rng = random.Random(5)
    d_rep, d_cli = rng.randrange(1, o.N), rng.randrange(1, o.N)
    auth.set_private_key(REPLICA, d_rep.to_bytes(32, "big"))
    auth.set_private_key(CLIENT, d_cli.to_bytes(32, "big"))
    msgs = _mixed(192)
    recs, arena = _records(msgs)
    got = auth.tag_bytes(*auth.sign_messages_flat(recs, arena))
    for m, tag in zip(msgs, got):
        d = d_cli if m.type == o.MSG_REQUEST else d_rep
        assert tag == _tag(d, o.quirk_digest(o.msg_authen_bytes(m))[:32]), m.type
    # PREPARE / COMMIT anywhere: MBFT_ERR_ARG, the outputs untouched
    for bad_type, pos in ((o.MSG_PREPARE, 0), (o.MSG_COMMIT, 191), (9, 77)):
        bad = recs.copy()
        bad[pos]["type"] = bad_type
        tags = np.full((192, 72), 0x5A, dtype=np.uint8)
        lens = np.full(192, 0x5A, dtype=np.uint8)
        rc = auth.lib.mbft_sign_messages_flat(auth.ctx, bad.ctypes.data, 192, arena.ctypes.data,
                                              arena.nbytes, tags.ctypes.data, lens.ctypes.data)
        assert rc == ERR_ARG
        assert (tags == 0x5A).all() and (lens == 0x5A).all()


def test_round_trip_4096_replies(auth):
    from oracle import c_oracle
    n = 4096
    rng = random.Random(4096)
    d = rng.randrange(1, o.N)
    q = o.pubkey(d)
    auth.set_private_key(REPLICA, d.to_bytes(32, "big"))
    auth.add_role(REPLICA)
    auth.set_public_key(REPLICA, 2, o.pkix_encode(q))
    msgs = [o.Msg(type=o.MSG_REPLY, replica_id=2, client_id=7, seq=i, op=rng.randbytes(1 + i % 96))
            for i in range(n)]
    recs, arena = _records(msgs)
    tags = auth.tag_bytes(*auth.sign_messages_flat(recs, arena))
    assert all(8 <= len(t) <= 72 for t in tags)
    for m, t in zip(msgs, tags):
        m.sig = t
    recs, arena = _records(msgs)
    assert not auth.validate_replies_flat(recs, arena, 7, NO_PANIC_STOP).any()
    # a sample through the C oracle
    idx = rng.sample(range(n), 256)
    qxy = np.frombuffer(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"), dtype=np.uint8).reshape(1, 64)
    st = c_oracle.verify_ecdsa_role_batch(qxy, np.zeros(256, dtype=np.uint32),
                                          [o.msg_authen_bytes(msgs[i]) for i in idx], [tags[i] for i in idx])
    assert not st.any()
    # one flipped bit in each of 64 tags: rejected or malformed, as the oracle says
    flipped = rng.sample(range(n), 64)
    for i in flipped:
        t = bytearray(msgs[i].sig)
        bit = rng.randrange(8 * len(t))
        t[bit // 8] ^= 1 << (bit % 8)
        msgs[i].sig = bytes(t)
    recs, arena = _records(msgs)
    res = auth.validate_replies_flat(recs, arena, 7, NO_PANIC_STOP)
    model = o.Authenticator(o.KeyStore(keys={REPLICA: {2: q}}))
    want = o.validate_replies(model, [msgs[i] for i in flipped], 7, NO_PANIC_STOP)
    assert [int(res[i]) for i in flipped] == want
    assert all(w != 0 for w in want)
    ok = np.ones(n, dtype=bool)
    ok[flipped] = False
    assert not res[ok].any()


def test_errors(lib):
    from minbft_amd.authenticator import Authenticator
    with Authenticator(0) as a:
        e = np.zeros((2, 32), dtype=np.uint8)
        tags = np.zeros((2, 72), dtype=np.uint8)
        lens = np.zeros(2, dtype=np.uint8)

        def pre(role, n=2):
            return a.lib.mbft_generate_tags_prehashed(a.ctx, role, e.ctypes.data, n, tags.ctypes.data,
                                                      lens.ctypes.data)

        msgs = [o.Msg(type=o.MSG_REPLY, seq=1, op=b"abc"), o.Msg(type=o.MSG_REQUEST, seq=2, op=b"defg")]
        recs, arena = _records(msgs)

        def rec(r, nbytes=None):
            return a.lib.mbft_sign_messages_flat(a.ctx, r.ctypes.data, len(r), arena.ctypes.data,
                                                 arena.nbytes if nbytes is None else nbytes,
                                                 tags.ctypes.data, lens.ctypes.data)

        assert pre(REPLICA) == ERR_STATE and pre(CLIENT) == ERR_STATE  # no private key
        assert rec(recs) == ERR_STATE
        a.set_private_key(REPLICA, (5).to_bytes(32, "big"))
        assert pre(REPLICA) == 0 and lens.all()
        assert pre(CLIENT) == ERR_STATE
        assert rec(recs) == ERR_STATE           # the REQUEST needs the client key
        assert rec(recs[:1]) == 0
        a.set_private_key(USIG, (5).to_bytes(32, "big"))
        assert pre(USIG) == ERR_STATE           # USIG generation stays in the enclave
        assert pre(REPLICA, 0) == 0             # n = 0
        a.set_private_key(CLIENT, (6).to_bytes(32, "big"))
        assert rec(recs) == 0
        out = recs.copy()                       # a field that leaves the arena
        out[1]["op_off"] = arena.nbytes - 3
        assert rec(out) == ERR_ARG
        out = recs.copy()
        out[0]["op_len"] = 2 ** 32 - 1
        assert rec(out) == ERR_ARG
        assert rec(recs, nbytes=arena.nbytes - 1) == ERR_ARG
        assert a.lib.mbft_set_signer_window(a.ctx, 3) == ERR_ARG
        assert a.lib.mbft_set_signer_window(a.ctx, 7) == ERR_ARG
        a.clear_keys()
        assert pre(REPLICA) == ERR_STATE and pre(CLIENT) == ERR_STATE and rec(recs) == ERR_STATE
        a.set_private_key(REPLICA, (5).to_bytes(32, "big"))
        assert pre(REPLICA) == 0


@pytest.mark.parametrize("w", [4, 6])
def test_other_windows(lib, expected, w):
    """The signer's other table windows (5 is the default: every other test)
    give the same tags (64 items)."""
    from minbft_amd.authenticator import Authenticator
    d, (es, want) = next(iter(expected.items()))
    with Authenticator(0) as a:
        a.set_signer_window(w)
        a.set_private_key(CLIENT, d.to_bytes(32, "big"))
        assert a.tag_bytes(*a.generate_tags_prehashed(CLIENT, _e_arr(es[:64]))) == want[:64]
