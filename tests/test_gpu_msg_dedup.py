"""The device message layer's deduplication and call decode
(msg_kernels.hip k_msg_cands, k_dedup_resolve, k_msg_calls) stage by stage,
through the test-only harness tests/csrc/msg_stage_check.hip (stage_run),
against the oracle and the model in tests/msg_stage_util.py.

k_dedup_resolve compares a candidate in full with its table slot's
representative only when both have the same 64-bit content hash, and no
honest input has two different calls with equal hashes: end to end
(tests/test_gpu_msgdev.py) the branch "collision with different content"
never runs.  The hash is no security boundary -- an attacker can craft
collisions -- so with a wrong comparison a forged message would take the
verdict of a valid one.  Here the harness FORCES the collision: after
k_msg_cands it gives chosen candidates one hash and rebuilds the table as an
honest run would have left it.  A variant that differs from the base COMMIT in
one thing must then come out as a call of its own, with e, r, s and the
outcome of ITS message; a repeat at another offset must stay a repeat.

Every arena exists twice (same fields, same offsets, different filler) and
every output, the content hashes included, must be equal for both."""
import copy
import hashlib
import random

import pytest

from msg_stage_util import (DEAD_SLOT, Keys, check_against_model, der_sig, load_harness, pack, stage_run_both)
from oracle import p256 as o

pytestmark = pytest.mark.gpu

CLIENT, CLIENT2 = 7, 8
OP_LENS = [1, 2, 3, 4, 5, 31, 32, 33, 35, 36, 37, 63, 64, 65, 67]


@pytest.fixture(scope="module")
def h(lib):
    return load_harness()


def keys4():
    """Clients 7 and 8 and the USIGs of replicas 0..3, all valid."""
    pairs = [(o.ROLE_CLIENT, CLIENT, 0), (o.ROLE_CLIENT, CLIENT2, 1)] + [(o.ROLE_USIG, i, 2 + i) for i in range(4)]
    return Keys(pairs, [1] * 6, [0, 0, 1, 2, 3, 4], role_ok=0b1110)


def cert(epoch, seed):
    return o.make_cert(epoch, der_sig(seed))


def op_bytes(n, seed=0):
    out = b""
    while len(out) < n:
        out += hashlib.sha256(b"op%d-%d" % (seed, len(out))).digest()
    return out[:n]


def base_commit(view=3, op_len=40):
    """A COMMIT from replica 1 on the primary's (view mod n = 0) PREPARE,
    valid DER in all three tags: three candidates of the three kinds."""
    return o.Msg(o.MSG_COMMIT, stream=1, replica_id=1, prep_replica_id=0, view=view, client_id=CLIENT, seq=5,
                 op=op_bytes(op_len), sig=der_sig(1), ui_counter=9, ui_cert=cert(0x1122334455667788, 2),
                 prep_ui_counter=4, prep_ui_cert=cert(0x1122334455667788, 3))


def vary(m, **kw):
    v = copy.copy(m)
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def forced(h, bases, variants, n_replicas, aligns=None, seed=0):
    """bases: messages; variants: (message, index of its base, the set of its
    candidates q that differ from the base's).  Candidate q of a base and of
    each of its variants are forced into one hash group; the base comes
    first, so it is the group's representative.  Everything is checked
    against the model, and then what the test is about, said directly: a
    differing candidate is a call of its own, decoded from its own message;
    the others are repeats of the base's."""
    msgs = list(bases) + [v for v, _, _ in variants]
    nb = len(bases)
    owner = list(range(nb)) + [b for _, b, _ in variants]
    group = [2 * (1 + 3 * owner[k // 3] + k % 3) for k in range(3 * len(msgs))]
    if aligns is None:
        aligns = [((i + 1) & 3, (i + 2) & 3, None, (i * 3) & 3) for i in range(len(msgs))]
    recs, a, b = pack(msgs, aligns, seed)
    keys = keys4()
    out = stage_run_both(h, recs, a, b, n_replicas, keys, group, one=3 * len(msgs) <= 4096)
    slots, content = check_against_model(out, msgs, n_replicas, keys, group)
    for j, (v, bi, differ) in enumerate(variants):
        i = nb + j
        for q in range(3):
            c = 3 * i + q
            assert slots[c] is not None and slots[3 * bi + q] is not None
            if q in differ:
                assert content[c] != content[3 * bi + q]
                assert int(out["uniq"][c]) == 1 and int(out["ref"][c]) == c, (j, q)
                assert int(out["call_of"][c]) == int(out["idx"][c])
            else:
                assert content[c] == content[3 * bi + q]
                assert int(out["uniq"][c]) == 0 and int(out["ref"][c]) == 3 * bi + q, (j, q)
                assert int(out["call_of"][c]) == int(out["call_of"][3 * bi + q])
    return out, msgs


ALL, REQ, PREP, COMM = {0, 1, 2}, 0, 1, 2


def field_variants(b, n_replicas):
    v = [
        (vary(b, client_id=CLIENT2), ALL),
        (vary(b, replica_id=2), {COMM}),
        # another primary: the view moves with it (isPrimary must still hold)
        (vary(b, prep_replica_id=2, replica_id=1, view=b.view + 2), {PREP, COMM}),
        (vary(b, view=b.view + n_replicas), {PREP, COMM}),
        (vary(b, seq=b.seq ^ 1), ALL),
        (vary(b, seq=b.seq ^ (1 << 63)), ALL),
        (vary(b, ui_counter=b.ui_counter ^ 2), {COMM}),
        (vary(b, ui_counter=b.ui_counter ^ (1 << 63)), {COMM}),
        (vary(b, prep_ui_counter=b.prep_ui_counter ^ 1), {PREP, COMM}),
        (vary(b, prep_ui_counter=b.prep_ui_counter ^ (1 << 63)), {PREP, COMM}),
        (vary(b, op=b.op[:-1]), ALL),
        (vary(b, sig=b.sig[:-1]), {REQ}),
        (vary(b, ui_cert=b.ui_cert[:-1]), {COMM}),
        (vary(b, prep_ui_cert=b.prep_ui_cert[:-1]), {PREP}),
    ]
    if n_replicas == 4:  # 2^32 and 2^63 are multiples of 4: the primary stays
        v += [(vary(b, view=b.view ^ (1 << 32)), {PREP, COMM}), (vary(b, view=b.view ^ (1 << 63)), {PREP, COMM})]
    return v


@pytest.mark.parametrize("n_replicas", [3, 4])
def test_forced_collision_one_field_differs(h, n_replicas):
    b = base_commit(view=n_replicas)  # primary 0
    vs = field_variants(b, n_replicas)
    assert all((v.prep_replica_id == v.view % n_replicas) for v, _ in vs)
    out, msgs = forced(h, [b], [(v, 0, d) for v, d in vs], n_replicas)
    # 3 calls of the base, then one per differing candidate
    assert int(out["bounds"][1]) == 3 + sum(len(d) for _, d in vs)
    # every call decodes (no dead slot: the keys are known, the DER valid)
    # except the three whose tag lost its last byte
    dead = [j for j in range(int(out["bounds"][1])) if int(out["slot"][j]) == DEAD_SLOT]
    assert len(dead) == 3


def flips(field, data):
    """One flipped bit at every byte position."""
    for p in range(len(data)):
        d = bytearray(data)
        d[p] ^= 1 << (p % 8)
        yield {field: bytes(d)}


@pytest.mark.parametrize("base_align", range(4))
def test_forced_collision_one_operation_byte_differs(h, base_align):
    """Every byte position of the operation, at every length around the 8-word
    blocks and the tail word of same_arena, under all pairs of alignments."""
    bases = [vary(base_commit(op_len=n), seq=100 + n) for n in OP_LENS]
    variants, aligns = [], [(base_align, 1, 2, 3)] * len(bases)
    for bi, b in enumerate(bases):
        for va in range(4):
            for kw in flips("op", b.op):
                variants.append((vary(b, **kw), bi, ALL))
                aligns.append((va, None, None, None))
    forced(h, bases, variants, 3, aligns, seed=base_align)


@pytest.mark.parametrize("base_align", range(4))
def test_forced_collision_one_tag_byte_differs(h, base_align):
    """The same for the three tags at their real lengths (70..72 bytes of DER,
    8 more in a cert); a flip may leave malformed DER: the model decodes the
    variant's own tag either way."""
    b = base_commit()
    variants, aligns = [], [(0, base_align, base_align, base_align)]
    for field, q in (("sig", REQ), ("ui_cert", COMM), ("prep_ui_cert", PREP)):
        for va in range(4):
            for kw in flips(field, getattr(b, field)):
                variants.append((vary(b, **kw), 0, {q}))
                aligns.append((None, va, va, va))
    forced(h, [b], variants, 3, aligns, seed=10 + base_align)


def test_forced_collision_equal_content_stays_a_repeat(h):
    b = base_commit()
    variants = [(copy.copy(b), 0, set()) for _ in range(16)]
    aligns = [(0, 0, 0, 0)] + [(j & 3, (j >> 2) & 3, (j + 1) & 3, (j + 2) & 3) for j in range(16)]
    out, _ = forced(h, [b], variants, 3, aligns, seed=20)
    assert int(out["bounds"][1]) == 3


def test_forced_collision_three_in_a_group(h):
    """a, b != a, c == b: b and c are both compared with the representative a
    only, so each is a call of its own (k_dedup_resolve says so)."""
    a = base_commit()
    b = vary(a, seq=a.seq + 1)
    out, _ = forced(h, [a], [(b, 0, ALL), (copy.copy(b), 0, ALL)], 3, seed=21)
    assert int(out["bounds"][1]) == 9


def test_honest_hashes_number_distinct_calls_in_first_occurrence_order(h):
    """A few hundred messages holding every call several times, at all
    alignments: the unique calls are exactly the distinct contents, numbered
    in first-occurrence order; chash is equal for equal content and differs
    between every one-field variant and its base (a failure there is a hash
    that ignores a field)."""
    b = base_commit(view=4)
    distinct = [b] + [v for v, _ in field_variants(b, 4)]
    for n in (1, 4, 33, 64):
        m = vary(base_commit(view=4, op_len=n), seq=200 + n)
        distinct += [m] + [vary(m, **kw) for kw in flips("op", m.op)]
    distinct += [vary(b, **kw) for f in ("sig", "ui_cert", "prep_ui_cert") for kw in flips(f, getattr(b, f))][::7]
    msgs, aligns = [], []
    for rep in range(3):
        for j, m in enumerate(distinct):
            msgs.append(copy.copy(m))
            x = j + 5 * rep
            aligns.append((x & 3, (x >> 1) & 3, None if x % 3 == 0 else (x >> 2) & 3, (x + rep) & 3))
    assert 300 <= len(msgs) <= 1365
    recs, aa, bb = pack(msgs, aligns, seed=30)
    keys = keys4()
    for one in (True, False):
        out = stage_run_both(h, recs, aa, bb, 4, keys, None, one)
        slots, content = check_against_model(out, msgs, 4, keys)
        order = []
        for k, c in enumerate(content):
            if c is not None and c not in order:
                order.append(c)
        assert int(out["bounds"][1]) == len(order)
        for k, c in enumerate(content):
            if c is not None:
                assert int(out["call_of"][k]) == order.index(c)
                assert content[int(out["cand_of"][int(out["call_of"][k])])] == c
        by_content = {}
        for k, c in enumerate(content):
            if c is not None:
                by_content[c] = int(out["chash"][k])
        assert len(set(by_content.values())) == len(by_content), "two different calls, one hash"


def test_calls_decode_every_outcome(h):
    """REQUEST / PREPARE / COMMIT records over operation lengths 0..130 and
    the SHA-256 block boundaries beyond, counters and views at 0, 1, 2^32 and
    2^64 - 1, tags that fit the LDS slot and that do not, every key outcome,
    short certs and malformed DER: e, r, s, the key slot and every field of
    the outcome record against the model, for each unique call."""
    n_replicas = 3
    # USIG 2: known, valid = 0; USIG 3: unknown; client 9: key slot >= nslots
    pairs = [(o.ROLE_CLIENT, CLIENT, 0), (o.ROLE_CLIENT, CLIENT2, 1), (o.ROLE_USIG, 0, 2), (o.ROLE_USIG, 1, 3),
             (o.ROLE_USIG, 2, 4), (o.ROLE_CLIENT, 9, 77)]
    keys = Keys(pairs, [1, 1, 1, 1, 0], [0, 0, 5, 6, 7], role_ok=0b1110)
    big = (1 << 64) - 1
    msgs, aligns = [], []

    def add(m, j):
        msgs.append(m)
        aligns.append((j & 3, (j >> 2) & 3, (j + 1) & 3, (j >> 1) & 3))

    op_lens = list(range(131)) + [183, 184, 247, 248, 256, 1000]
    ctrs = [1, 2, 1 << 32, big]
    rng = random.Random(41)
    for j, n in enumerate(op_lens * 4):
        j4 = j % len(op_lens) + j // len(op_lens)  # each round moves op_off & 3 by one: all four per length
        kind = j % 3
        view = rng.choice([0, 1, 1 << 32, big, 3, 4])
        primary = view % n_replicas  # 0 or 1: both USIGs valid
        backup = 1 - primary
        seq = rng.choice([0, 1, 1 << 32, big])
        op = op_bytes(n, j)
        # trailing bytes after the DER: ignored in an ECDSA tag, DER_TRAILING in a cert; with 40 of
        # them no tag fits the 25-word LDS slot
        trail = rng.choice([b"", b"", b"\x00", bytes(range(40))])
        if kind == 0:
            add(o.Msg(o.MSG_REQUEST, client_id=[CLIENT, CLIENT2][j & 1], seq=seq, op=op, sig=der_sig(j) + trail), j4)
        elif kind == 1:
            add(o.Msg(o.MSG_PREPARE, replica_id=primary, view=view, client_id=CLIENT, seq=seq, op=op, sig=der_sig(j),
                      ui_counter=ctrs[j % 4], ui_cert=cert(j * 0x0101010101, j) + trail), j4)
        else:
            add(o.Msg(o.MSG_COMMIT, replica_id=backup, prep_replica_id=primary, view=view, client_id=CLIENT2,
                      seq=seq, op=op, sig=der_sig(j) + trail, ui_counter=ctrs[(j + 1) % 4],
                      ui_cert=cert(big - j, j + 1), prep_ui_counter=ctrs[j % 4], prep_ui_cert=cert(j, j + 2) + trail),
                j4)
    b = base_commit()
    edge = [
        vary(b, ui_counter=0), vary(b, prep_ui_counter=0),            # zero counters: no call
        vary(b, replica_id=0),                                        # a COMMIT from the primary
        vary(b, view=4),                                              # not the primary's PREPARE
        o.Msg(o.MSG_REPLY, client_id=CLIENT, seq=1, op=b"x", sig=der_sig(0)),
        o.Msg(o.MSG_REQ_VIEW_CHANGE, view=9),
        vary(b, client_id=12345),                                     # unknown client key
        vary(b, client_id=9),                                         # key slot past the key table
        vary(b, replica_id=2),                                        # known USIG, valid = 0
        vary(b, replica_id=3),                                        # unknown USIG
        vary(b, prep_replica_id=2, replica_id=1, view=5),
        vary(b, sig=b""), vary(b, sig=b"\x30"), vary(b, sig=b.sig[:-1]), vary(b, sig=b"\x31" + b.sig[1:]),
        vary(b, sig=b.sig[:3] + b"\x00" + b.sig[4:]),                 # malformed DER, ECDSA role
        vary(b, ui_cert=b.ui_cert[:8] + b"\x30\x00"),                 # malformed DER in a cert
        vary(b, prep_ui_cert=b.prep_ui_cert[:8] + b.prep_ui_cert[9:]),
        vary(b, sig=o.der_encode_sig(1 << 256, 5)),                   # decodes; r >= 2^256 reads as zero
        vary(b, sig=bytes.fromhex("3006020180020105")),               # negative r
    ]
    edge += [vary(b, ui_cert=b.ui_cert[:n]) for n in range(9)]        # certs shorter than 8 bytes, and 8
    edge += [vary(b, prep_ui_cert=b.prep_ui_cert[:n]) for n in (0, 1, 7)]
    for j, m in enumerate(edge):
        add(m, j)
    # tags around the LDS slot's 25 words at every tag_off & 3: valid DER followed by 0, 1 and 40 bytes, and by
    # what makes the tag 96..101 bytes long (staged exactly when (tag_off & 3) + tag_len <= 100)
    seq = 1000
    for a in range(4):
        sig, crt = der_sig(500 + a), cert(77, 600 + a)
        trails = [b"", b"\x01", bytes(range(40))]
        for t in trails + [bytes(n - len(sig)) for n in range(96, 102)]:
            seq += 1
            msgs.append(o.Msg(o.MSG_REQUEST, client_id=CLIENT, seq=seq, op=op_bytes(9, seq), sig=sig + t))
            aligns.append((None, a, None, None))
        for t in trails + [bytes(n - len(crt)) for n in range(96, 102)]:
            seq += 1
            msgs.append(o.Msg(o.MSG_PREPARE, replica_id=0, view=3, client_id=CLIENT, seq=seq, op=op_bytes(9, seq),
                              sig=sig, ui_counter=seq, ui_cert=crt + t))
            aligns.append((None, None, a, None))
    assert 3 * len(msgs) <= 4096
    recs, aa, bb = pack(msgs, aligns, seed=40)
    for n in op_lens[1:]:
        assert {int(r["op_off"]) & 3 for r in recs if int(r["op_len"]) == n} == {0, 1, 2, 3}, n
    for a in range(4):  # staged and not staged at every alignment
        fits = {(int(r["sig_off"]) & 3) + int(r["sig_len"]) <= 100 for r in recs if int(r["sig_off"]) & 3 == a}
        assert fits == {True, False}
    for roles, one in ((0b1110, True), (0b1110, False), (0b1010, True)):  # last: no USIG scheme registered
        keys.role_ok = roles
        out = stage_run_both(h, recs, aa, bb, n_replicas, keys, None, one)
        check_against_model(out, msgs, n_replicas, keys)
        total = int(out["bounds"][1])
        pres = {int(x) for x in out["info"]["pre"][:total]}
        tails = {int(x) for x in out["info"]["usig_tail"][:total]}
        if roles == 0b1110:  # every outcome occurred
            assert pres == {0xFF, o.MALFORMED_DER, o.UNKNOWN_KEY, o.BAD_KEY, o.BAD_CERT}
            assert tails == {0xFF, o.MALFORMED_DER, o.DER_TRAILING}
            assert (out["slot"][:total] != DEAD_SLOT).sum() > 250  # most calls get a digest
        else:
            assert o.UNKNOWN_ROLE in pres
