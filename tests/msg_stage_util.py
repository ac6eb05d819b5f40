"""Shared by tests/test_gpu_arena_dev.py, tests/test_gpu_msg_dedup.py,
tests/test_gpu_msg_number.py and tests/test_gpu_msg_replay.py: the ctypes side of the test-only harness
tests/csrc/msg_stage_check.hip, byte arenas built twice (same fields at the
same offsets, different filler), and a Python model of the device message
layer's stages written from the rules msg_kernels.hip cites."""
import ctypes
import hashlib
import os
import random
import struct

import numpy as np

from oracle import p256 as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK8, MARK32 = 0xAA, 0xAAAAAAAA

REC = np.dtype([("type", "<u4"), ("stream", "<u4"), ("replica_id", "<u4"), ("prep_replica_id", "<u4"),
                ("client_id", "<u4"), ("op_len", "<u4"), ("sig_len", "<u4"), ("ui_cert_len", "<u4"),
                ("prep_ui_cert_len", "<u4"), ("reserved", "<u4"), ("view", "<u8"), ("seq", "<u8"),
                ("ui_counter", "<u8"), ("prep_ui_counter", "<u8"), ("op_off", "<u8"), ("sig_off", "<u8"),
                ("ui_cert_off", "<u8"), ("prep_ui_cert_off", "<u8")])
CAND = np.dtype([("role", "<u4"), ("id", "<u4"), ("kind", "<u4"), ("msg", "<u4"), ("primary", "<u4"),
                 ("tag_len", "<u4"), ("tag_off", "<u8"), ("prep_ctr", "<u8"), ("counter", "<u8")])
INFO = np.dtype([("pre", "u1"), ("usig_tail", "u1"), ("usig", "u1"), ("role", "u1"), ("fpg", "<u4"),
                 ("ui_epoch", "<u8"), ("counter", "<u8")])

K_REQUEST, K_PREPARE, K_COMMIT = 0, 2, 3           # kernels.h AuthenKind
CHK_CALL, CHK_FAIL, CHK_ZERO, CHK_PANIC = 0, 1, 2, 3  # msg_dev.h kChk*
DEAD_SLOT = 0xFFFFFF00 | o.BAD_KEY                  # msg_kernels.hip kDeadSlotDev


def load_harness():
    path = os.path.join(ROOT, "tests", "libmsg_stage_check.so")
    if not os.path.exists(path):
        from __graft_entry__ import build_msg_stage_check
        build_msg_stage_check()
    h = ctypes.CDLL(path)
    vp, i, u32, u64, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_long
    h.msg_stage_number_one_max.restype = lg
    h.arena_run.argtypes = [i, vp, u64, vp, vp, vp, i, vp]
    h.stage_run.argtypes = [vp, lg, vp, u64, u32, u32, vp, vp, u32, u32, vp, vp, u32, vp, i] + [vp] * 15
    h.number_run.argtypes = [lg, vp, vp, vp, u32, i, vp, vp, vp, vp, vp]
    h.upload_run.argtypes = [vp, u64, u64, vp]
    h.replay_run.argtypes = [lg, vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, vp, u64, vp]
    assert h.msg_stage_rec_size() == REC.itemsize
    assert h.msg_stage_cand_size() == CAND.itemsize
    assert h.msg_stage_info_size() == INFO.itemsize
    assert h.msg_stage_tag_words() == 25
    return h


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------------
# Arenas, built twice
class Arena:
    """Fields at chosen offsets; every byte that belongs to no field is
    filler, random in copy A and its complement in copy B.  put() without an
    alignment packs the field right behind its neighbour (no gap)."""

    def __init__(self, seed, lead=5):
        self.rng = random.Random(seed)
        self.buf = bytearray()
        self.fill = []
        self._pad(lead)

    def _pad(self, k):
        for _ in range(k):
            self.fill.append(len(self.buf))
            self.buf.append(self.rng.randrange(256))

    def put(self, data, align=None, mod=64):
        """-> offset; align: the offset's value modulo `mod` (4 for off & 3)."""
        if align is not None:
            self._pad((align - len(self.buf)) % mod)
        off = len(self.buf)
        self.buf += data
        return off

    def finish(self, tail=3):
        self._pad(tail)
        a = np.frombuffer(bytes(self.buf), dtype=np.uint8).copy()
        b = a.copy()
        b[np.array(self.fill, dtype=np.int64)] ^= 0xFF
        return a, b


def pack(msgs, aligns, seed):
    """o.Msg list -> (recs, arena A, arena B).  aligns[i]: (op, sig, ui_cert,
    prep_ui_cert) values of off & 3, or None for no gap before that field."""
    ar = Arena(seed)
    recs = np.zeros(len(msgs), dtype=REC)
    for i, (m, al) in enumerate(zip(msgs, aligns)):
        r = recs[i]
        r["type"], r["stream"], r["replica_id"], r["prep_replica_id"] = m.type, m.stream, m.replica_id, m.prep_replica_id
        r["client_id"], r["view"], r["seq"] = m.client_id, m.view, m.seq
        r["ui_counter"], r["prep_ui_counter"] = m.ui_counter, m.prep_ui_counter
        for (name, data), a in zip((("op", m.op), ("sig", m.sig), ("ui_cert", m.ui_cert),
                                    ("prep_ui_cert", m.prep_ui_cert)), al):
            r[name + "_len"] = len(data)
            r[name + "_off"] = ar.put(data, a, 4)
    a, b = ar.finish()
    return recs, a, b


# --------------------------------------------------------------------------
# Keys: what k_msg_calls looks a call's (role, id) up in
class Keys:
    def __init__(self, pairs, valid, fpg, role_ok):
        """pairs: (role, id, slot); valid / fpg: per key slot."""
        self.pairs, self.valid, self.fpg, self.role_ok = list(pairs), list(valid), list(fpg), role_ok
        self.map = {(r, i): s for r, i, s in self.pairs}


def table_cap(n):
    cap = 1024  # msgdev.cpp: at least 1,024 slots, at least 2 x 3n
    while cap < 2 * 3 * n:
        cap <<= 1
    return cap


def stage_run(h, recs, arena, n_replicas, keys, group=None, one=True):
    n = len(recs)
    km_key = np.array([(r << 32) | i for r, i, _ in keys.pairs], dtype=np.uint64)
    km_slot = np.array([s for _, _, s in keys.pairs], dtype=np.uint32)
    valid = np.array(keys.valid, dtype=np.uint32)
    fpg = np.array(keys.fpg, dtype=np.uint32)
    g = None if group is None else np.ascontiguousarray(group, dtype=np.uint64)
    assert g is None or len(g) == 3 * n
    out = {"bad": np.zeros(1, np.uint32), "chk": np.zeros(n, np.uint32), "cand": np.zeros(3 * n, CAND),
           "chash": np.zeros(3 * n, np.uint64)}
    for k in ("uniq", "ref", "idx", "call_of", "cand_of"):
        out[k] = np.zeros(3 * n, np.uint32)
    out["bounds"] = np.zeros(2, np.uint32)
    for k in ("e", "r", "s"):
        out[k] = np.zeros((3 * n, 32), np.uint8)
    out["slot"] = np.zeros(3 * n, np.uint32)
    out["info"] = np.zeros(3 * n, INFO)
    recs = np.ascontiguousarray(recs)
    arena = np.ascontiguousarray(arena)
    rc = h.stage_run(ptr(recs), n, ptr(arena), len(arena), n_replicas, table_cap(n), ptr(km_key), ptr(km_slot),
                     len(km_key), keys.role_ok, ptr(valid), ptr(fpg), len(valid), None if g is None else ptr(g),
                     1 if one else 0, *[ptr(out[k]) for k in ("bad", "chk", "cand", "chash", "uniq", "ref", "idx",
                                                               "call_of", "cand_of", "bounds", "e", "r", "s", "slot",
                                                               "info")])
    assert rc == 0, rc
    return out


def stage_run_both(h, recs, a, b, n_replicas, keys, group=None, one=True):
    """The run over both copies of the arena: every output identical (what a
    kernel reads outside a field can change nothing), returned once."""
    x = stage_run(h, recs, a, n_replicas, keys, group, one)
    y = stage_run(h, recs, b, n_replicas, keys, group, one)
    for k in x:
        assert np.array_equal(x[k], y[k]), "filler changed " + k
    return x


REPLAY_PAD = 8                    # sentinel elements behind out and cap
OUT_MARK, CAP_MARK = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NO_CAPTURE = (1 << 64) - 1        # cap_pos of a group nothing captures


def replay_run(h, chk, call_of, info, status, epoch_set, epoch_val):
    """mbft_launch::msg_replay once over injected state.  out and cap go in
    as msgdev.cpp fills them -- cap = cap_pos[G] (~0) | cap_epoch[G] |
    first_bad (n) -- with REPLAY_PAD sentinels behind each, and out[:n] and
    cap_epoch hold the sentinel value too (msgdev.cpp leaves them as they
    were).  -> the launcher's return value, out and cap whole."""
    n, nc, G = len(chk), len(info), len(epoch_set)
    assert len(call_of) == 3 * n and len(status) == nc and len(epoch_val) == G
    chk = np.ascontiguousarray(chk, dtype=np.uint32)
    call_of = np.ascontiguousarray(call_of, dtype=np.uint32)
    info = np.ascontiguousarray(info, dtype=INFO)
    status = np.ascontiguousarray(status, dtype=np.uint8)
    epoch_set = np.ascontiguousarray(epoch_set, dtype=np.uint8)
    epoch_val = np.ascontiguousarray(epoch_val, dtype=np.uint64)
    out = np.full(n + REPLAY_PAD, OUT_MARK, dtype=np.int32)
    cap = np.full(2 * G + 1 + REPLAY_PAD, CAP_MARK, dtype=np.uint64)
    cap[:G] = NO_CAPTURE
    cap[2 * G] = n
    rc = np.full(1, -1, dtype=np.int32)
    r = h.replay_run(n, ptr(chk), ptr(call_of), ptr(info), ptr(status), nc, G, ptr(epoch_set), ptr(epoch_val),
                     ptr(out), len(out), ptr(cap), len(cap), ptr(rc))
    assert r == 0, r
    return int(rc[0]), out, cap


# --------------------------------------------------------------------------
# The model
def model_cands(m, n_replicas):
    """k_msg_cands for one message (core/message-handling.go:409-424 and the
    validators it dispatches to): the candidate calls, a prefix of (REQUEST
    signature, PREPARE UI, COMMIT UI), and the packed checks."""
    cands, checks = [], []

    def request():
        cands.append(dict(role=o.ROLE_CLIENT, id=m.client_id, kind=K_REQUEST, primary=0, tag=m.sig, prep_ctr=0,
                          counter=0))
        checks.append((CHK_CALL, o.ST_REQUEST_SIG, 0))

    def prepare(primary, ctr, cert):
        if primary != m.view % n_replicas:
            checks.append((CHK_FAIL, o.ST_NOT_PRIMARY, 0))
            return False
        request()
        if ctr == 0:
            checks.append((CHK_ZERO, o.ST_PREPARE_UI, 0))
            return False
        cands.append(dict(role=o.ROLE_USIG, id=primary, kind=K_PREPARE, primary=0, tag=cert, prep_ctr=0, counter=ctr))
        checks.append((CHK_CALL, o.ST_PREPARE_UI, 1))
        return True

    if m.type == o.MSG_REQUEST:
        request()
    elif m.type == o.MSG_REPLY:
        checks.append((CHK_PANIC, o.ST_UNKNOWN_TYPE, 0))
    elif m.type == o.MSG_PREPARE:
        prepare(m.replica_id, m.ui_counter, m.ui_cert)
    elif m.type == o.MSG_COMMIT:
        if m.replica_id == m.prep_replica_id:
            checks.append((CHK_FAIL, o.ST_COMMIT_FROM_PRIMARY, 0))
        elif prepare(m.prep_replica_id, m.prep_ui_counter, m.prep_ui_cert):
            if m.ui_counter == 0:
                checks.append((CHK_ZERO, o.ST_COMMIT_UI, 0))
            else:
                cands.append(dict(role=o.ROLE_USIG, id=m.replica_id, kind=K_COMMIT, primary=m.prep_replica_id,
                                  tag=m.ui_cert, prep_ctr=m.prep_ui_counter, counter=m.ui_counter))
                checks.append((CHK_CALL, o.ST_COMMIT_UI, 2))
    else:
        checks.append((CHK_FAIL, o.ST_NOT_IMPLEMENTED, 0))
    packed = len(checks)
    for j, (kind, stage, q) in enumerate(checks):
        packed |= (kind | (stage << 2) | (q << 6)) << (8 + 8 * j)
    return cands, packed


def call_content(c, m):
    """messages.cpp call_key: equal key fields, operation and tag <=> the
    identical authenticator call."""
    usig = c["kind"] in (K_PREPARE, K_COMMIT)
    return (c["role"], c["id"], c["kind"], c["counter"], m.client_id if usig else 0,
            c["primary"] if c["kind"] == K_COMMIT else 0, m.view if usig else 0,
            c["prep_ctr"] if c["kind"] == K_COMMIT else 0, m.seq, bytes(m.op), bytes(c["tag"]))


def be32(v):
    """der_dev.h der_int: 32 big-endian bytes, zeros for a negative value or
    one >= 2^256."""
    return v.to_bytes(32, "big") if 0 <= v < (1 << 256) else bytes(32)


def model_call(c, m, keys):
    """k_msg_calls for one unique call -> (e, r, s, slot, info tuple); the
    rules and their order are batch.cpp prepare_item's (crypto.go:79-89 for an
    ECDSA role: DER first, then the key; usig.go:75-80, sgx-usig.go:159-168,
    usig-enclave.go:217-221 for a UI: key, cert length, then the cert's DER
    and its trailing bytes)."""
    role, tag = c["role"], c["tag"]
    zero = bytes(32)
    pre, tail, usig, fpg, ui_epoch, counter = 0xFF, 0xFF, 0, 0, 0, 0
    e = r = s = zero
    slot = DEAD_SLOT

    def info():
        return (pre, tail, usig, role, fpg, ui_epoch, counter)

    if role > 3 or not (keys.role_ok >> role) & 1:
        pre = o.UNKNOWN_ROLE
        return e, r, s, slot, info()
    known = (role, c["id"]) in keys.map
    sl = keys.map.get((role, c["id"]), 0)
    valid = known and sl < len(keys.valid) and keys.valid[sl] != 0
    if role != o.ROLE_USIG:
        try:
            rv, sv, _ = o.der_parse_sig(tag)
        except o.Asn1Error:
            pre = o.MALFORMED_DER
            return e, r, s, slot, info()
        if not known:
            pre = o.UNKNOWN_KEY
        elif not valid:
            pre = o.BAD_KEY
        else:
            slot = sl
            e = o.quirk_digest(o.msg_authen_bytes(m, o.MSG_REQUEST))[:32]
            r, s = be32(rv), be32(sv)
        return e, r, s, slot, info()
    if not known:
        pre = o.UNKNOWN_KEY
    elif not valid:
        pre = o.BAD_KEY
    elif len(tag) < 8:
        pre = o.BAD_CERT
    else:
        usig, fpg, counter = 1, keys.fpg[sl], c["counter"]
        ui_epoch = struct.unpack(">Q", tag[:8])[0]
        try:
            rv, sv, rest = o.der_parse_sig(tag[8:])
        except o.Asn1Error:
            tail = o.MALFORMED_DER
            return e, r, s, slot, info()
        if rest:
            tail = o.DER_TRAILING
        else:
            slot = sl
            ab = o.msg_authen_bytes(m, o.MSG_PREPARE if c["kind"] == K_PREPARE else o.MSG_COMMIT)
            e = o.usig_digest(ab, ui_epoch, counter)
            r, s = be32(rv), be32(sv)
    return e, r, s, slot, info()


def check_against_model(out, msgs, n_replicas, keys, group=None):
    """Every array stage_run returns against the model.  The hash of a
    candidate is the forced one where group says so, else the device's own
    (chash itself is checked for equal content => equal hash).  Returns the
    model's (cands per slot, contents per slot) for the caller's own checks."""
    n = len(msgs)
    assert int(out["bad"][0]) == 0
    slots = [None] * (3 * n)
    for i, m in enumerate(msgs):
        cands, packed = model_cands(m, n_replicas)
        assert int(out["chk"][i]) == packed, (i, hex(int(out["chk"][i])), hex(packed))
        for q, c in enumerate(cands):
            slots[3 * i + q] = c
    content = [None if c is None else call_content(c, msgs[k // 3]) for k, c in enumerate(slots)]
    chash = [int(x) for x in out["chash"]]
    seen = {}
    for k, c in enumerate(slots):
        if c is None:
            assert chash[k] == 0, k
            continue
        want = chash[k]
        if group is not None and int(group[k]) != 0:
            assert chash[k] == int(group[k])
        else:
            assert chash[k] != 0 and chash[k] & 1, k
            assert seen.setdefault(content[k], want) == want, ("equal content, different hash", k)
        cd = out["cand"][k]
        assert (int(cd["role"]), int(cd["id"]), int(cd["kind"]), int(cd["msg"]), int(cd["primary"]),
                int(cd["tag_len"]), int(cd["prep_ctr"]), int(cd["counter"])) == \
            (c["role"], c["id"], c["kind"], k // 3, c["primary"], len(c["tag"]), c["prep_ctr"], c["counter"]), k
    # k_dedup_resolve: a slot's representative is its smallest candidate; a
    # candidate is a repeat only of a representative with equal content
    rep = {}
    for k, c in enumerate(slots):
        if c is not None:
            rep.setdefault(chash[k], k)
    uniq, ref = [0] * (3 * n), list(range(3 * n))
    for k, c in enumerate(slots):
        if c is None:
            continue
        r = rep[chash[k]]
        same = content[k] == content[r]
        uniq[k] = 1 if (r == k or not same) else 0
        ref[k] = r if same else k
    assert [int(x) for x in out["uniq"]] == uniq
    assert [int(x) for x in out["ref"]] == ref
    idx = np.concatenate(([0], np.cumsum(uniq)[:-1])).astype(np.int64)
    assert np.array_equal(out["idx"].astype(np.int64), idx)
    total = int(sum(uniq))
    assert [int(x) for x in out["bounds"]] == [0, total]
    cand_of = [MARK32] * (3 * n)
    for k, c in enumerate(slots):
        want = int(idx[ref[k]]) if c is not None else MARK32
        assert int(out["call_of"][k]) == want, k
        if uniq[k]:
            cand_of[int(idx[k])] = k
    assert [int(x) for x in out["cand_of"]] == cand_of
    for j in range(total):
        k = cand_of[j]
        e, r, s, slot, info = model_call(slots[k], msgs[k // 3], keys)
        got = (bytes(out["e"][j]), bytes(out["r"][j]), bytes(out["s"][j]), int(out["slot"][j]),
               tuple(int(x) for x in out["info"][j].tolist()))
        assert got == (e, r, s, slot, info), (j, k, got, (e, r, s, slot, info))
        if slot == DEAD_SLOT:
            assert got[0] == got[1] == got[2] == bytes(32)
    for name in ("e", "r", "s"):
        assert (out[name][total:] == MARK8).all(), name  # nothing past the unique calls
    assert (out["slot"][total:] == MARK32).all()
    return slots, content


def der_sig(seed):
    """Valid DER of a signature-shaped (r, s) fixed by seed (70..72 bytes)."""
    d = hashlib.sha512(b"msg-stage-sig" + str(seed).encode()).digest()
    r = int.from_bytes(d[:32], "big") % (o.N - 1) + 1
    s = int.from_bytes(d[32:], "big") % (o.N - 1) + 1
    return o.der_encode_sig(r, s)
