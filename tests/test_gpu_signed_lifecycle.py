"""The life of a key after registration with the signed compact class among
the classes (``_lib.KEY_CLASS_SIGNED_TEETH(t)``), through the C-ABI: one golden
key set walked window 0 -> signed 3 -> unsigned 4 -> signed 9 -> W = 8 ->
signed 2 with every status unchanged at each stop, mbft_get_key_class and
mbft_key_memory at each stop; removal and reuse of a released signed piece;
promotion by count into signed 5 with accounting on; the codes next to the
class's range stay refused.  Helpers from tests/test_gpu_key_lifecycle.py.
"""
import random

import numpy as np
import pytest

from golden_util import prehashed_arrays
from test_gpu_key_lifecycle import (ACCEPT, REJECT, ROLE_CLIENT, T, _chain, _crafted, _register_ids, _run_sizes,
                                    _xy, class_bytes)

pytestmark = pytest.mark.gpu


def S(t):
    return 0x200 | t


def cbytes(cls):
    return 64 << ((cls & 0xFF) - 1) if cls >= 0x200 else class_bytes(cls)


def test_reclass_walk_through_signed_classes(lib):
    from minbft_amd.authenticator import Authenticator
    xy, e, r, s, exp, labels = prehashed_arrays()
    assert len(labels) == 551
    with Authenticator(0) as a:
        a.set_key_window(0)
        slots, slot_of, nk = _register_ids(a, xy)
        _run_sizes(a, e, r, s, slots, exp, labels, "registered")
        blocks = a.key_memory()[2]
        for cls in (S(3), T(4), S(9), 8, S(2)):
            a.set_slot_classes(slot_of[:-1], cls)
            assert a.key_class(ROLE_CLIENT, nk - 1)[0] != cls  # (the bulk call named the others only)
            a.set_key_class(ROLE_CLIENT, nk - 1, cls)
            for k in range(nk):
                assert a.key_class(ROLE_CLIENT, k) == (cls, cbytes(cls)), (cls, k)
            live, listed, held = a.key_memory()
            assert live == nk * cbytes(cls)
            assert held >= blocks and held >= live + listed
            blocks = held
            _run_sizes(a, e, r, s, slots, exp, labels, "class %#x" % cls)
        assert [cbytes(S(t)) for t in range(2, 10)] == [128, 256, 512, 1024, 2048, 4096, 8192, 16384]


def test_codes_next_to_the_range_are_refused(lib):
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        a.set_key_window(0)
        a.set_public_key(ROLE_CLIENT, 0, _xy(_chain(1)[0]))
        sl = np.array([a.key_slot(ROLE_CLIENT, 0)], dtype=np.uint32)
        mem = a.key_memory()
        for bad in (0x200, 0x201, 0x20A, 0x2FF, 0x300, 0x302):
            assert a.lib.mbft_set_slot_classes(a.ctx, sl.ctypes.data, 1, bad) == _lib.ERR_ARG
            assert a.lib.mbft_set_key_class(a.ctx, ROLE_CLIENT, 0, bad) == _lib.ERR_ARG
        assert a.key_memory() == mem and a.key_class(ROLE_CLIENT, 0) == (0, 64)
        for t in range(2, 10):
            a.set_key_class(ROLE_CLIENT, 0, S(t))
            assert a.key_class(ROLE_CLIENT, 0) == (S(t), 64 << (t - 1))


def test_removal_reuses_a_signed_piece(lib):
    """100 rounds of register-one and remove-one at signed 5: after the first
    round the key blocks held and the highest slot number stay what they are,
    and the newcomer verifies in the reused slot and storage."""
    from minbft_amd.authenticator import Authenticator
    cls = S(5)
    pts = _chain(102)
    e, r, s = _crafted(pts, 2, range(102), random.Random(cls))
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        a.set_key_signed_teeth(5)
        a.set_public_key(ROLE_CLIENT, 0, _xy(pts[0]))  # a resident of the store, beside the churn
        held = top = None
        for k in range(1, 101):
            a.set_public_key(ROLE_CLIENT, k, _xy(pts[k]))
            sl = a.key_slot(ROLE_CLIENT, k)
            if k % 25 == 1:
                st = a.verify_prehashed(e[[0, k, k]], r[[0, k, k]], s[[0, k - 1, k]],
                                        np.array([a.key_slot(ROLE_CLIENT, 0), sl, sl]))
                assert st.tolist() == [ACCEPT, REJECT, ACCEPT], k
            a.remove_public_key(ROLE_CLIENT, k)
            live, listed, blocks = a.key_memory()
            assert (live, listed) == (1024, 1024)
            if k == 1:
                held, top = blocks, sl
            assert (blocks, sl) == (held, top), k
        # the last queued-class key leaves: large batches under W = 8 keys still verify
        a.remove_public_key(ROLE_CLIENT, 0)
        a.set_key_window(8)
        a.set_public_key(ROLE_CLIENT, 200, _xy(pts[101]))
        sl = a.key_slot(ROLE_CLIENT, 200)
        idx = np.full(4200, 101)
        st = a.verify_prehashed(e[idx], r[idx], s[idx], np.full(4200, sl, dtype=np.uint32))
        assert (st == ACCEPT).all()


def test_promotion_into_signed_teeth(lib):
    """64 table-free keys; key 7 signs 3,000 of 4,200 items, key 9 signs 600.
    mbft_promote_hot_keys into signed 5 moves exactly those two; an unsigned 4
    key (the same bytes) is not promoted into it, nor the other way."""
    from minbft_amd.authenticator import Authenticator
    nkeys, n = 64, 4200
    pts = _chain(nkeys)
    rest = [k for k in range(nkeys) if k not in (7, 9)]
    key = np.array([7] * 3000 + [9] * 600 + [rest[i % len(rest)] for i in range(600)])
    np.random.default_rng(3).shuffle(key)
    e, r, s = _crafted(pts, 2, key, random.Random(8))
    tam = np.arange(n) % 9 == 0
    e[tam, 31] ^= 1
    want = np.where(tam, REJECT, ACCEPT)
    with Authenticator(0) as a:
        a.add_role(ROLE_CLIENT)
        a.set_key_window(0)
        for k in range(nkeys):
            a.set_public_key(ROLE_CLIENT, k, _xy(pts[k]))
        a.set_key_class(ROLE_CLIENT, 11, T(4))       # 1 KiB, like signed 5
        slots = np.array([a.key_slot(ROLE_CLIENT, k) for k in range(nkeys)], dtype=np.uint32)[key]
        a.set_key_accounting(True)
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
        assert a.promote_hot_keys(S(5), 2, 3001) == 0
        assert a.promote_hot_keys(S(5), 2, 500) == 2
        for k in range(nkeys):
            assert a.key_class(ROLE_CLIENT, k) == ((S(5), 1024) if k in (7, 9) else (T(4), 1024) if k == 11
                                                   else (0, 64)), k
        assert a.key_memory()[0] == 3 * 1024 + 61 * 64
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
        assert a.promote_hot_keys(T(4), nkeys, 3000) == 0   # key 7 ties in bytes: not moved back
        assert a.promote_hot_keys(S(5), nkeys, 0) == 61     # everyone cheaper; key 11 ties and stays
        assert a.key_class(ROLE_CLIENT, 11) == (T(4), 1024)
        assert a.promote_hot_keys(S(6), nkeys, 0) == 64     # 2 KiB: all of them, key 11 included
        assert a.key_memory()[0] == nkeys * 2048
        assert (a.verify_prehashed(e, r, s, slots) == want).all()
