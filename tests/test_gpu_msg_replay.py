"""The device message layer's optimistic replay (msg_kernels.hip
k_replay_caps, k_replay_cap_epoch, k_replay_eval, launched by
mbft_launch::msg_replay) over INJECTED state, through the test-only harness
tests/csrc/msg_stage_check.hip (replay_run), against a sequential replay in
Python.

End to end the three kernels only ever see streams built from real
signatures: at most 33 fingerprint groups, the check index always equal to
the candidate slot, nearly every call accepted and every epoch non-zero.
Here they get fabricated checks, call outcomes and epoch state: group counts
around the 64 threads of k_replay_cap_epoch's workgroup, message counts
around the 256 of the other two, checks that name another slot than their
index, pre-set context epochs that match and mismatch, captured epochs of 0,
tails and pre-decided outcomes, captures in, before and after the first
message that fails.

The reference goes message by message and check by check with the epoch
state changed in place (batch.cpp resolve_call, the check rules of
messages.cpp replay_tail), stops at the first message whose result is not 0
and keeps the state as it was before that message.  Asserted for every case:
first_bad, out up to and including it (what lies behind it the library
overwrites), which groups' captures msgdev.cpp would commit (cap_pos <
3 first_bad) and their epochs, no capture in a group the context had set,
the sentinels behind out and cap, and a second run giving the same bytes.

Three changes to the kernels cannot show in any result and so have no case
here: `<=` for `<` where a check reads its group's capture (the capturing
check would read back the epoch it computes on the unset state), cap_epoch
taking ui_epoch whatever the counter (a check with another counter than 1
captures only with ui_epoch 0), and the capture tested before epoch_set
(k_replay_caps leaves cap_pos of a set group at ~0, which is asserted)."""
import functools

import numpy as np
import pytest

from msg_stage_util import (CAP_MARK, CHK_CALL, CHK_FAIL, CHK_PANIC, CHK_ZERO, INFO, NO_CAPTURE, OUT_MARK, REPLAY_PAD,
                            load_harness, ptr, replay_run)
from oracle import p256 as o

pytestmark = pytest.mark.gpu

NS = [1, 3, 255, 256, 257, 700]   # k_replay_caps / k_replay_eval: 256 messages a workgroup
GS = [0, 1, 63, 64, 65, 200]      # k_replay_cap_epoch: 64 groups a workgroup
RATES = [0.0, 0.02, 0.2]
E1, E2 = 0x1122334455667788, 0xF0E0D0C0B0A09080  # (E2: the top bit set)
NONE = 0xFF                       # DevCallInfo pre / usig_tail: nothing decided
PRE_STATUSES = [o.MALFORMED_DER, o.UNKNOWN_KEY, o.BAD_KEY, o.BAD_CERT, o.UNKNOWN_ROLE]


@pytest.fixture(scope="module")
def h(lib):
    return load_harness()


class Case:
    """n messages' checks (msgs[i][q] = (kind, stage, slot): check index q,
    candidate slot 3 i + slot), call_of per candidate slot, the unique calls
    (info tuples in INFO's field order, verifier status) and the context's
    epoch state per fingerprint group."""

    def __init__(self, n, G, preset=()):
        self.n, self.G = n, G
        self.msgs = [[] for _ in range(n)]
        self.call_of = [None] * (3 * n)
        self.info, self.status = [], []
        self.epoch_set, self.epoch_val = [0] * G, [0] * G
        for g, v in dict(preset).items():
            self.epoch_set[g], self.epoch_val[g] = 1, v

    def ecdsa(self, status=o.ACCEPT, pre=NONE):
        self.info.append((pre, NONE, 0, o.ROLE_CLIENT, 0, 0, 0))
        self.status.append(status)
        return len(self.info) - 1

    def usig(self, g, epoch, counter=1, status=o.ACCEPT, tail=NONE, pre=NONE):
        assert g < self.G
        self.info.append((pre, tail, 1, o.ROLE_USIG, g, epoch, counter))
        self.status.append(status)
        return len(self.info) - 1

    def call(self, i, k, slot=None, stage=None):
        """The next check of message i: call k, found through candidate
        slot `slot` (default: the check's own index)."""
        q = len(self.msgs[i])
        slot = q if slot is None else slot
        assert q < 3 and slot < 3 and self.call_of[3 * i + slot] is None
        self.call_of[3 * i + slot] = k
        self.msgs[i].append((CHK_CALL, (o.ST_REQUEST_SIG, o.ST_PREPARE_UI, o.ST_COMMIT_UI)[q] if stage is None
                             else stage, slot))

    def fail(self, i, kind, stage):
        assert len(self.msgs[i]) < 3
        self.msgs[i].append((kind, stage, 0))

    def fill(self, k, skip=()):
        """Every message without a check (and not in skip) gets one: call k."""
        for i in range(self.n):
            if not self.msgs[i] and i not in skip:
                self.call(i, k)

    def arrays(self, decoy):
        """-> chk, call_of, info, status, epoch_set, epoch_val; a candidate
        slot no check names holds decoy(slot): a call index in range that a
        kernel reading the wrong slot would take."""
        chk = np.zeros(self.n, dtype=np.uint32)
        for i, cs in enumerate(self.msgs):
            w = len(cs)
            for q, (kind, stage, slot) in enumerate(cs):
                w |= (kind | (stage << 2) | (slot << 6)) << (8 + 8 * q)
            chk[i] = w
        call_of = np.array([decoy(c) if k is None else k for c, k in enumerate(self.call_of)], dtype=np.uint32)
        return (chk, call_of, np.array(self.info, dtype=INFO), np.array(self.status, dtype=np.uint8),
                np.array(self.epoch_set, dtype=np.uint8), np.array(self.epoch_val, dtype=np.uint64))


# --------------------------------------------------------------------------
# The reference: sequential, the state changed in place
def resolve_call(eset, eval_, p, g):
    """batch.cpp resolve_call: one call's outcome applied in order; the USIG
    epoch capture is the only state (crypto.go:219-236, sgx-usig.go:92-94)."""
    pre, tail, usig, _, fpg, ui_epoch, counter = p
    if pre != NONE:
        return pre
    if not usig:
        return g
    if eset[fpg]:
        epoch = eval_[fpg]
    else:
        epoch = ui_epoch if counter == 1 else 0
    if ui_epoch != epoch:
        return o.EPOCH_MISMATCH
    if tail != NONE:
        return tail
    if g == o.ACCEPT:
        eval_[fpg] = epoch
        eset[fpg] = 1
    return g


def run_message(case, i, eset, eval_, seen=None):
    """Message i's checks in order on the state (messages.cpp replay_tail's
    check rules) -> its result.  seen: collects (status, group) of every
    USIG call check that ran."""
    for kind, stage, slot in case.msgs[i]:
        if kind in (CHK_FAIL, CHK_PANIC):
            return stage << 8
        if kind == CHK_ZERO:
            return (stage << 8) | o.ZERO_COUNTER
        k = case.call_of[3 * i + slot]
        st = resolve_call(eset, eval_, case.info[k], case.status[k])
        if seen is not None and case.info[k][2]:
            seen.append((st, case.info[k][4]))
        if st != o.ACCEPT:
            return (stage << 8) | st
    return 0


def sequential(case):
    """-> f (the first message whose result is not 0, n if none), that
    result, the epoch state as it was before message f (after the last
    message if f == n), and what the walk met (for the coverage counts)."""
    eset, eval_ = list(case.epoch_set), list(case.epoch_val)
    seen = []
    f, res, snap = case.n, 0, None
    for i in range(case.n):
        before = (list(eset), list(eval_))
        r = run_message(case, i, eset, eval_, seen)
        if r != 0:
            f, res, snap = i, r, before
            break
    if snap is None:
        snap = (eset, eval_)
    new = {g: snap[1][g] for g in range(case.G) if snap[0][g] and not case.epoch_set[g]}
    # a capturing candidate at or after f: a USIG call check with only call
    # checks before it, its group unset in the snapshot, that captures when
    # it runs on that unset state
    later = False
    for i in range(f, case.n):
        for kind, _, slot in case.msgs[i]:
            if kind != CHK_CALL:
                break
            k = case.call_of[3 * i + slot]
            p = case.info[k]
            if p[2] and not snap[0][p[4]]:
                s1, v1 = [0] * case.G, [0] * case.G
                if resolve_call(s1, v1, p, case.status[k]) == o.ACCEPT and s1[p[4]]:
                    later = True
    return dict(f=f, res=res, new=new, later=later,
                preset_mismatch=any(st == o.EPOCH_MISMATCH and case.epoch_set[g] for st, g in seen),
                index_ne_slot=any(q != slot for cs in case.msgs[:f + 1] for q, (kind, _, slot) in enumerate(cs)
                                  if kind == CHK_CALL))


# --------------------------------------------------------------------------
def check(h, case, arrays, ref):
    n, G = case.n, case.G
    rc, out, cap = replay_run(h, *arrays)
    rc2, out2, cap2 = replay_run(h, *arrays)
    assert rc == 0 and rc2 == 0
    f = ref["f"]
    assert int(cap[2 * G]) == f, ("first_bad", int(cap[2 * G]), f)
    assert not out[:f].any(), ("a result before first_bad", np.nonzero(out[:f])[0][:5])
    if f < n:
        assert int(out[f]) == ref["res"], (f, hex(int(out[f])), hex(ref["res"]))
    for g in range(G):
        pos = int(cap[g])
        assert (pos < 3 * f) == (g in ref["new"]), ("commit", g, pos, f)
        if g in ref["new"]:
            assert int(cap[G + g]) == ref["new"][g], ("epoch", g, hex(int(cap[G + g])), hex(ref["new"][g]))
        if case.epoch_set[g]:
            assert pos == NO_CAPTURE, ("a capture in a group the context had set", g, pos)
    assert (out[n:] == OUT_MARK).all() and (cap[2 * G + 1:] == CAP_MARK).all()
    assert np.array_equal(out, out2) and np.array_equal(cap, cap2)  # the atomics are min-only
    return out, cap


# --------------------------------------------------------------------------
# Directed cases.  Each returns the case and what it must give, worked out
# by hand: f, message f's result, the committed groups' epochs and (some)
# groups' cap_pos -- asserted of the reference and of the kernels.
def _two_workgroups():
    """Two capturing candidates of one group at messages 5 and 300 (another
    workgroup), different epochs: the first wins, the second's message is an
    epoch mismatch."""
    c = Case(700, 3)
    c.call(5, c.usig(1, E1))
    c.call(10, c.usig(1, E1, counter=2))
    c.call(300, c.usig(1, E2))
    c.fill(c.ecdsa())
    return c, 300, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {1: E1}, {1: 15, 0: NO_CAPTURE, 2: NO_CAPTURE}


def _two_workgroups_late_first():
    """The same with the later message's candidate listed first among the
    calls and at check index 2: the order of the calls does not matter."""
    c = Case(700, 3)
    late, early = c.usig(1, E2), c.usig(1, E1)
    k = c.ecdsa()
    c.call(300, k)
    c.call(300, k, slot=2)
    c.call(300, late, slot=1)
    c.call(5, early)
    c.fill(k)
    return c, 300, (o.ST_COMMIT_UI << 8) | o.EPOCH_MISMATCH, {1: E1}, {1: 15}


def _same_message_second_sees_first():
    """Two checks of message 256 in one group: the second (another epoch)
    sees the first's capture -> mismatch; message f's own capture is not
    committed."""
    c = Case(257, 1)
    c.call(256, c.usig(0, E1))
    c.call(256, c.usig(0, E2))
    c.fill(c.ecdsa())
    return c, 256, (o.ST_PREPARE_UI << 8) | o.EPOCH_MISMATCH, {}, {0: 768}


def _same_message_second_needs_first():
    """The second check (counter 2, the same epoch) is accepted only on the
    first's capture; the first runs on the unset state, not on its own
    capture."""
    c = Case(257, 1)
    c.call(256, c.usig(0, E1))
    c.call(256, c.usig(0, E1, counter=2))
    c.fill(c.ecdsa())
    return c, 257, 0, {0: E1}, {0: 768}


def _shared_call():
    """One unique call (the embedded PREPARE UI) shared by every message."""
    c = Case(257, 2)
    k, ui = c.ecdsa(), c.usig(1, E2)
    for i in range(c.n):
        c.call(i, k)
        c.call(i, ui)
    return c, 257, 0, {1: E2}, {1: 1, 0: NO_CAPTURE}


def _index0_names_slot2():
    """The check at index 0 names slot 2: its position is 3 i + 0, the call
    comes from slot 2 (slots 0 and 1 hold a rejecting decoy)."""
    c = Case(3, 1)
    c.call(1, c.usig(0, E1), slot=2)
    c.call(2, c.usig(0, E1, counter=2), slot=1)
    c.fill(c.ecdsa())
    return c, 3, 0, {0: E1}, {0: 3}


def _permuted_triple():
    """Checks 0, 1, 2 name slots 2, 0, 1: check 1 (counter 2) needs check
    0's capture, which lies in a HIGHER slot than its own."""
    c = Case(3, 2)
    c.call(1, c.usig(0, E1), slot=2)
    c.call(1, c.usig(0, E1, counter=2), slot=0)
    c.call(1, c.usig(1, E2), slot=1)
    c.fill(c.ecdsa())
    return c, 3, 0, {0: E1, 1: E2}, {0: 3, 1: 5}


def _permuted_capture_after_reader():
    """Checks 0, 1 name slots 1, 0: check 0 (counter 2, unset state) is a
    mismatch although the capturing check behind it sits in a lower slot."""
    c = Case(3, 1)
    c.call(1, c.usig(0, E1, counter=2), slot=1)
    c.call(1, c.usig(0, E1), slot=0)
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {0: 4}


def _preset_equal():
    c = Case(3, 2, {0: E1})
    c.call(1, c.usig(0, E1, counter=7))
    c.fill(c.ecdsa())
    return c, 3, 0, {}, {0: NO_CAPTURE, 1: NO_CAPTURE}


def _preset_unequal():
    c = Case(3, 2, {1: E1})
    c.call(1, c.usig(1, E2))
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {1: NO_CAPTURE}


def _preset_zero():
    """The context's epoch 0 against ui_epoch 0 (accepted), then against a
    counter-1 UI of another epoch (the set state wins over counter == 1)."""
    c = Case(3, 1, {0: 0})
    c.call(0, c.usig(0, 0, counter=3))
    c.call(1, c.ecdsa())
    c.call(2, c.usig(0, E1))
    return c, 2, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {0: NO_CAPTURE}


def _captures_epoch_zero():
    """Counter 5 with ui_epoch 0 captures epoch 0; a later counter-1 UI with
    a non-zero epoch then mismatches."""
    c = Case(6, 1)
    c.call(2, c.usig(0, 0, counter=5))
    c.call(4, c.usig(0, E1))
    c.fill(c.ecdsa())
    return c, 4, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {0: 0}, {0: 6}


def _counter_not_one_unset():
    """Counter 2 with a non-zero ui_epoch on the unset state: a mismatch
    that captures nothing (the counter-1 UI behind it is the first capture)."""
    c = Case(6, 1)
    c.call(2, c.usig(0, E1, counter=2))
    c.call(3, c.usig(0, E1))
    c.fill(c.ecdsa())
    return c, 2, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {0: 9}


def _tail_epoch_matching():
    """usig_tail with the epoch matching: the tail, and no capture."""
    c = Case(4, 1)
    c.call(1, c.usig(0, E1, tail=o.DER_TRAILING))
    c.call(2, c.usig(0, E1))
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.DER_TRAILING, {}, {0: 6}


def _tail_epoch_mismatching_preset():
    """usig_tail with the epoch mismatching: the epoch is tested first."""
    c = Case(4, 1, {0: E2})
    c.call(1, c.usig(0, E1, tail=o.MALFORMED_DER))
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {0: NO_CAPTURE}


def _tail_epoch_mismatching_unset():
    c = Case(4, 1)
    c.call(1, c.usig(0, E1, counter=2, tail=o.DER_TRAILING))
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.EPOCH_MISMATCH, {}, {0: NO_CAPTURE}


def _pre_overrides():
    """pre set on a USIG call that would otherwise capture: pre is the
    result, nothing is captured."""
    c = Case(4, 2)
    c.call(0, c.usig(1, E1, pre=o.BAD_CERT))
    c.fill(c.ecdsa())
    return c, 0, (o.ST_REQUEST_SIG << 8) | o.BAD_CERT, {}, {0: NO_CAPTURE, 1: NO_CAPTURE}


def _pre_overrides_mismatch():
    """pre set on a USIG call whose epoch mismatches, whose tail is set and
    whose status rejects: pre is the result."""
    c = Case(4, 1, {0: E2})
    c.call(2, c.usig(0, E1, status=o.REJECT_SIG, tail=o.DER_TRAILING, pre=o.UNKNOWN_KEY))
    c.fill(c.ecdsa())
    return c, 2, (o.ST_REQUEST_SIG << 8) | o.UNKNOWN_KEY, {}, {}


def _rejected_never_captures():
    """A rejected UI captures nothing: the accepted one two messages on is
    the group's first capture."""
    c = Case(5, 1)
    c.call(1, c.usig(0, E2, status=o.REJECT_SIG))
    c.call(3, c.usig(0, E1))
    c.fill(c.ecdsa())
    return c, 1, (o.ST_REQUEST_SIG << 8) | o.REJECT_SIG, {}, {0: 9}


def _noncall_in_front(kind, stage, res):
    def build():
        c = Case(4, 1)
        c.fail(2, kind, stage)
        c.call(2, c.usig(0, E1))
        c.fill(c.ecdsa())
        return c, 2, res, {}, {0: NO_CAPTURE}
    build.__doc__ = "A non-call check in front of a capturing call check: the call never runs."
    return build


def _captures_in_f():
    """Message 6 captures in group 0, then fails, then would capture in
    group 1; message 2 captured in group 2.  Only group 2 is committed."""
    c = Case(9, 3)
    c.call(2, c.usig(2, E2))
    c.call(6, c.usig(0, E1))
    c.call(6, c.ecdsa(status=o.REJECT_SIG))
    c.call(6, c.usig(1, E2))
    c.fill(c.ecdsa())
    return c, 6, (o.ST_PREPARE_UI << 8) | o.REJECT_SIG, {2: E2}, {0: 18, 1: 20, 2: 6}


def _capture_after_f():
    """A capturing candidate after f in a group nothing before f touches."""
    c = Case(9, 3)
    c.call(1, c.usig(0, E1))
    c.call(3, c.ecdsa(status=o.REJECT_SIG))
    c.call(8, c.usig(2, E2))
    c.fill(c.ecdsa())
    return c, 3, (o.ST_REQUEST_SIG << 8) | o.REJECT_SIG, {0: E1}, {0: 3, 1: NO_CAPTURE, 2: 24}


def _first_bad_at(f):
    def build():
        n = 700
        c = Case(n, 2)
        bad = c.ecdsa(status=o.REJECT_SIG)
        new, pos = {}, {}
        if f is not None:
            c.call(f, bad, stage=o.ST_REPLY_SIG)
            c.call(f, c.usig(1, E2))       # behind the failing check
            if f + 1 < n:
                c.call(f + 1, bad)         # a later failure: the minimum counts
            if f + 300 < n:
                c.call(f + 300, bad)
            pos[1] = 3 * f + 1
        g0 = 0 if f is None else f - 1     # a capture in the message before f
        if g0 >= 0:
            k = c.ecdsa()
            c.call(g0, k)
            c.call(g0, k)
            c.call(g0, c.usig(0, E1))
            new[0], pos[0] = E1, 3 * g0 + 2
        c.fill(c.ecdsa())
        return c, n if f is None else f, 0 if f is None else (o.ST_REPLY_SIG << 8) | o.REJECT_SIG, new, pos
    build.__doc__ = "first_bad at %s of 700 (256 messages a workgroup), a capture right before it" % (f,)
    return build


def _zero_checks():
    """Messages with no check at all: result 0, around messages that
    capture."""
    c = Case(257, 1)
    c.call(100, c.usig(0, E1))
    c.call(256, c.usig(0, E1, counter=9))
    return c, 257, 0, {0: E1}, {0: 300}


def _groups_past_one_workgroup():
    """Captures in groups 0, 63, 64, 65 and 199 of 200 (64 groups a
    workgroup of k_replay_cap_epoch), each its own epoch, one of them 0."""
    c = Case(8, 200, {7: E1})
    new, pos = {}, {}
    for j, g in enumerate((199, 64, 0, 65, 63)):
        e = 0 if g == 65 else E1 + g
        c.call(j, c.usig(g, e, counter=3 if g == 65 else 1))
        new[g], pos[g] = e, 3 * j
    for g in (199, 64, 63):  # accepted only on the epochs captured above
        c.call(7, c.usig(g, E1 + g, counter=4))
    c.fill(c.ecdsa())
    return c, 8, 0, new, pos


DIRECTED = {
    "two_workgroups": _two_workgroups,
    "two_workgroups_late_first": _two_workgroups_late_first,
    "same_message_second_sees_first": _same_message_second_sees_first,
    "same_message_second_needs_first": _same_message_second_needs_first,
    "shared_call": _shared_call,
    "index0_names_slot2": _index0_names_slot2,
    "permuted_triple": _permuted_triple,
    "permuted_capture_after_reader": _permuted_capture_after_reader,
    "preset_equal": _preset_equal,
    "preset_unequal": _preset_unequal,
    "preset_zero": _preset_zero,
    "captures_epoch_zero": _captures_epoch_zero,
    "counter_not_one_unset": _counter_not_one_unset,
    "tail_epoch_matching": _tail_epoch_matching,
    "tail_epoch_mismatching_preset": _tail_epoch_mismatching_preset,
    "tail_epoch_mismatching_unset": _tail_epoch_mismatching_unset,
    "pre_overrides": _pre_overrides,
    "pre_overrides_mismatch": _pre_overrides_mismatch,
    "rejected_never_captures": _rejected_never_captures,
    "fail_in_front": _noncall_in_front(CHK_FAIL, o.ST_NOT_PRIMARY, o.ST_NOT_PRIMARY << 8),
    "zero_counter_in_front": _noncall_in_front(CHK_ZERO, o.ST_PREPARE_UI, (o.ST_PREPARE_UI << 8) | o.ZERO_COUNTER),
    "panic_in_front": _noncall_in_front(CHK_PANIC, o.ST_UNKNOWN_TYPE, o.ST_UNKNOWN_TYPE << 8),
    "captures_in_f": _captures_in_f,
    "capture_after_f": _capture_after_f,
    "first_bad_0": _first_bad_at(0),
    "first_bad_255": _first_bad_at(255),
    "first_bad_256": _first_bad_at(256),
    "first_bad_last": _first_bad_at(699),
    "first_bad_none": _first_bad_at(None),
    "zero_checks": _zero_checks,
    "groups_past_one_workgroup": _groups_past_one_workgroup,
}


@pytest.mark.parametrize("name", list(DIRECTED))
def test_directed(h, name):
    case, f, res, new, pos = DIRECTED[name]()
    poison = case.ecdsa(pre=o.BAD_KEY)  # what an unnamed candidate slot holds
    ref = sequential(case)
    assert (ref["f"], ref["res"], ref["new"]) == (f, res, new), (ref["f"], hex(ref["res"]), ref["new"])
    _, cap = check(h, case, case.arrays(lambda c: poison), ref)
    for g, p in pos.items():  # msg_dev.h: the group's first capturing check, 3 i + q (~0 = none)
        assert int(cap[g]) == p, (g, int(cap[g]), p)


# --------------------------------------------------------------------------
# Random cases
def random_case(n, G, rate, rng):
    """Messages [0, L) (L = n at rate 0, else anywhere in 0..n) only have
    call checks of calls that are accepted in message order; from L on a
    check is a non-call check at `rate`, and a call check takes a faulty
    call at `rate`.  A check's slot is a random one of its message's three,
    an unnamed slot holds a random call."""
    c = Case(n, G)
    ep = [0 if rng.random() < 0.1 else int(rng.integers(1, 1 << 64, dtype=np.uint64)) for _ in range(G)]
    wrong = [False] * G  # pre-set to another epoch than the group's calls carry
    for g in range(G):
        if rng.random() < 0.3:
            wrong[g] = rng.random() < rate
            c.epoch_set[g], c.epoch_val[g] = 1, ep[g] ^ (1 << int(rng.integers(64))) if wrong[g] else ep[g]
        else:
            c.epoch_val[g] = int(rng.integers(1 << 63))  # not set: never read
    good = [g for g in range(G) if not wrong[g]]
    clean, dirty = [], []
    for _ in range(max(2, n // 2)):
        if not good or rng.random() < 0.4:
            clean.append(c.ecdsa())
        else:
            g = good[int(rng.integers(len(good)))]
            free = c.epoch_set[g] or ep[g] == 0  # any counter is accepted
            clean.append(c.usig(g, ep[g], counter=int(rng.integers(1, 6)) if free else 1))
    for _ in range(max(2, n // 4) if rate else 0):
        kind = int(rng.integers(8))
        g = int(rng.integers(G)) if G else 0
        other = lambda: ep[g] ^ (1 << int(rng.integers(64)))  # noqa: E731
        if G == 0 or kind == 0:
            dirty.append(c.ecdsa(status=o.REJECT_SIG) if rng.random() < 0.5 else
                         c.ecdsa(pre=PRE_STATUSES[int(rng.integers(len(PRE_STATUSES)))]))
        elif kind == 1:
            dirty.append(c.usig(g, ep[g], pre=PRE_STATUSES[int(rng.integers(len(PRE_STATUSES)))]))
        elif kind == 2:
            dirty.append(c.usig(g, ep[g], status=o.REJECT_SIG))
        elif kind == 3:
            dirty.append(c.usig(g, ep[g], tail=o.DER_TRAILING))
        elif kind == 4:
            dirty.append(c.usig(g, other(), counter=int(rng.integers(1, 3)), tail=o.MALFORMED_DER))
        elif kind == 5:
            dirty.append(c.usig(g, other()))                  # captures another epoch where unset
        elif kind == 6:
            dirty.append(c.usig(g, 0, counter=int(rng.integers(2, 9))))  # captures epoch 0 where unset
        else:
            dirty.append(c.usig(g, ep[g] | 1, counter=int(rng.integers(2, 9))))
    L = n if rate == 0 else int(rng.integers(n + 1))
    for i in range(n):
        nchk = 0 if rng.random() < 0.05 else int(rng.integers(1, 4))
        slots = [int(s) for s in rng.permutation(3)[:nchk]]
        for slot in slots:
            if i >= L and rng.random() < rate:
                c.fail(i, (CHK_FAIL, CHK_ZERO, CHK_PANIC)[int(rng.integers(3))], int(rng.integers(1, 16)))
                continue
            pool = dirty if i >= L and rng.random() < rate else clean
            c.call(i, pool[int(rng.integers(len(pool)))], slot=slot, stage=int(rng.integers(1, 16)))
    nc = len(c.info)
    decoys = rng.integers(nc, size=3 * n)
    return c, c.arrays(lambda s: int(decoys[s]))


@functools.lru_cache(maxsize=None)
def random_cases(n):
    """n's cases (every G, every rate; one fixed seed per shape) with the
    sequential reference's answers: built once, shared, never changed."""
    cases = []
    for G in GS:
        rng = np.random.default_rng(1000 * n + G)
        for rate in RATES:
            case, arrays = random_case(n, G, rate, rng)
            cases.append((G, rate, case, arrays, sequential(case)))
    return cases


@pytest.mark.parametrize("n", NS)
def test_random(h, n):
    for G, rate, case, arrays, ref in random_cases(n):
        try:
            check(h, case, arrays, ref)
        except AssertionError as e:
            raise AssertionError("n=%d G=%d rate=%g: %s" % (n, G, rate, e)) from e


def test_random_cases_cover_every_property():
    """Counted from the reference alone, so that a change of the generator
    cannot hollow test_random out."""
    count = dict.fromkeys(("f == n", "0 < f < n", "commit", "candidate at or after f", "index != slot",
                           "pre-set mismatch"), 0)
    for n in NS:
        for _, _, case, _, ref in random_cases(n):
            count["f == n"] += ref["f"] == n
            count["0 < f < n"] += 0 < ref["f"] < n
            count["commit"] += bool(ref["new"])
            count["candidate at or after f"] += ref["later"]
            count["index != slot"] += ref["index_ne_slot"]
            count["pre-set mismatch"] += ref["preset_mismatch"]
    print("random cases: %d, of them %s" % (len(NS) * len(GS) * len(RATES), count))
    assert all(count.values()), count


# --------------------------------------------------------------------------
# Edge launches
def test_no_message_launches_nothing(h):
    """n == 0: success, out and cap exactly as they went in."""
    for G in (0, 3):
        c = Case(0, G, {1: E1} if G else {})
        c.ecdsa()
        rc, out, cap = replay_run(h, *c.arrays(lambda s: 0))
        assert rc == 0
        assert (out == OUT_MARK).all()
        assert (cap[:G] == NO_CAPTURE).all() and int(cap[2 * G]) == 0
        assert (cap[G:2 * G] == CAP_MARK).all() and (cap[2 * G + 1:] == CAP_MARK).all()


@pytest.mark.parametrize("n", [1, 257])
def test_no_group_no_usig_call(h, n):
    """G == 0 (k_replay_cap_epoch is not launched): ECDSA calls only, with
    and without a failing one; and no call at all."""
    for bad in (None, n - 1):
        c = Case(n, 0)
        if bad is not None:
            c.call(bad, c.ecdsa(status=o.REJECT_SIG))
        c.fill(c.ecdsa())
        ref = sequential(c)
        assert ref["f"] == (n if bad is None else bad)
        check(h, c, c.arrays(lambda s: 0), ref)
    c = Case(n, 0)  # not one unique call: only non-call checks
    c.fail(n - 1, CHK_ZERO, o.ST_COMMIT_UI)
    ref = sequential(c)
    assert (ref["f"], ref["res"]) == (n - 1, (o.ST_COMMIT_UI << 8) | o.ZERO_COUNTER)
    check(h, c, c.arrays(lambda s: 0), ref)


def test_harness_refuses_out_of_range_state(h):
    """replay_run checks every index before it launches: a call_of or a
    fingerprint group out of range, more than 3 checks, slot 3."""
    def run(chk, call_of, info, status, eset, eval_):
        n, G = len(chk), len(eset)
        out = np.full(n + REPLAY_PAD, OUT_MARK, dtype=np.int32)
        cap = np.full(2 * G + 1 + REPLAY_PAD, CAP_MARK, dtype=np.uint64)
        rc = np.full(1, -1, dtype=np.int32)
        r = h.replay_run(n, ptr(chk), ptr(call_of), ptr(info), ptr(status), len(info), G, ptr(eset), ptr(eval_),
                         ptr(out), len(out), ptr(cap), len(cap), ptr(rc))
        assert (out == OUT_MARK).all() and (cap == CAP_MARK).all() and rc[0] == -1  # nothing ran
        return r

    def base():
        c = Case(2, 1)
        c.call(0, c.usig(0, E1))
        c.call(1, c.ecdsa())
        return [a.copy() for a in c.arrays(lambda s: 0)]

    a = base()
    a[1][4] = 2          # call_of >= nc
    assert run(*a) == -1
    a = base()
    a[2][0]["fpg"] = 1   # a USIG call's group >= G
    assert run(*a) == -1
    a = base()
    a[0][0] = 4          # four checks
    assert run(*a) == -1
    a = base()
    a[0][0] |= 3 << 14   # check 0 names slot 3
    assert run(*a) == -1
