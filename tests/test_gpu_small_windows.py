"""Comb windows 4 to 7 through every verify form, with crafted vectors.

tests/golden/small_windows.json (make_golden.make_small_windows; checked on
its own by test_small_windows_fixture.py) holds, for W = 4 .. 7: the corners
of the signed-digit recoding (the carry into the top window -- at W = 4 the
entry of digit 2^W, the last of the last table --, every window 2^(W-1) and
its neighbours, 2^255 - 1), four scalars at every window at which a form
starts a range or leaves comb_range_uniform's preload of 16 windows (a carry
entering it, zero digits at it, digit 2^(W-1) on both sides), scalars whose
low or high half of the windows is zero, and accumulator collisions of the
one-lane comb.  Windows below 8 reach what W >= 8 cannot: the split and
resident one-workgroup forms give a wave ceil(S / 2) = 32, 26, 22, 19 windows,
so every window past the 16th is read from the table as the sum goes; a
quad's high lane replays up to 32 carries; every form recodes 64 .. 37
windows a scalar.

Vectors labelled w<W> run at key window W, those labelled any at every W;
generator windows 4 and 7 against key windows 4 .. 7, generator window 20
against 4 and 7.  Every status is compared with the fixture's expectation
(the oracle's); no vector is left out.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import load, prehashed_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "small_windows.json"
PAIRS = [(wg, wq) for wg in (4, 7) for wq in (4, 5, 6, 7)] + [(20, 4), (20, 7)]


def _check(st, exp, labels, what=""):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i], int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, len(bad), bad[:20])
    assert set(np.unique(st).tolist()) <= {0, 1}, what


def vectors_of(W):
    """The fixture's arrays cut down to the vectors that run at key window W."""
    xy, e, r, s, exp, labels = prehashed_arrays(NAME)
    keep = np.array([i for i, l in enumerate(labels) if l.startswith(("any:", "w%d:" % W))])
    return xy[keep], e[keep], r[keep], s[keep], exp[keep], [labels[i] for i in keep]


def resident_vectors(W):
    """At most 64 of window W's vectors under the fixture key, for the lone
    calls: the top-window and seam-carry scalars as u2, the zero pairs at
    every seam, then single zero digits while there is room."""
    vecs = [v for v in load(NAME) if v["label"].startswith(("any:", "w%d:" % W)) and ":comb_" not in v["label"]]
    order = []
    for pick in (lambda n, r: n.startswith("top_") and r == "u2", lambda n, r: n.endswith("_carry") and r == "u2",
                 lambda n, r: n.endswith(("_z01", "_z1")), lambda n, r: n.endswith("_z0")):
        order += [v for v in vecs if pick(*v["label"].split(":")[1:3])]
    assert len(order) >= 30 and len({v["qx"] for v in order}) == 1
    return order[:64]


@pytest.fixture(scope="module")
def small():
    xy, e, r, s, exp, labels = prehashed_arrays(NAME)
    assert len(labels) == 544 and exp.sum() == 298
    return {W: vectors_of(W) for W in (4, 5, 6, 7)}


@pytest.fixture(scope="module")
def context(lib):
    """One context per generator window, made when first asked for (the
    W = 4 and 7 tables are a few KB; W = 20 is 388 MiB, built once)."""
    from minbft_amd.authenticator import Authenticator
    made = {}

    def get(wg):
        if wg not in made:
            made[wg] = Authenticator(0)
            made[wg].set_generator_window(wg)
        assert made[wg].windows()[0] == wg
        return made[wg]

    yield get
    for a in made.values():
        a.close()


def _register(a, xy, wq):
    a.clear_keys()
    a.set_key_window(wq)
    assert a.windows()[1] == wq
    slots, valid = a.register_points(xy)
    assert valid.all()
    return slots


@pytest.mark.parametrize("wg,wq", PAIRS)
def test_split(context, small, wg, wq):
    """k_verify_split, at most 200 items a call so that each takes it: waves
    0 / 1 sum G's windows [0, mid) / [mid, S), waves 2 / 3 Q's.  A range is
    32, 26, 22, 19 windows at W = 4 .. 7, longer than comb_range_uniform's
    preload of 16, so by construction every item reads its later windows
    through entry()'s direct arm, and the seam vectors put a carry, zero
    digits and the largest digit at windows lo + 16 and mid."""
    a = context(wg)
    xy, e, r, s, exp, labels = small[wq]
    slots = _register(a, xy, wq)
    a.set_small_batch_form(256)
    try:
        st = np.concatenate([a.verify_prehashed(e[k:k + 200], r[k:k + 200], s[k:k + 200], slots[k:k + 200])
                             for k in range(0, len(labels), 200)])
    finally:
        a.set_small_batch_form(-1)
    _check(st, exp, labels, "split wg=%d wq=%d" % (wg, wq))


@pytest.mark.parametrize("wg,wq", PAIRS)
def test_pairs_and_quads(context, small, wg, wq):
    """Past the split kernel's range (tiled past 256 items): lane pairs
    inverting per lane (0) and on the s^-1 planes (1), lane quads inline (2)
    and on the planes (3).  The G lane runs the generator's S steps beside the
    Q lane's 64 .. 37; a quad's high lanes replay the carries of windows
    [0, mid) -- up to 32 -- before their first window."""
    a = context(wg)
    xy, e, r, s, exp, labels = small[wq]
    slots = _register(a, xy, wq)
    reps = 256 // len(labels) + 1
    tile = lambda x: np.concatenate([x] * reps)  # noqa: E731
    assert 256 < len(labels) * reps <= 512
    a.set_small_batch_form(0)
    try:
        for form in (0, 1, 2, 3):
            a.set_small_batch_inverse(form)
            st = a.verify_prehashed(tile(e), tile(r), tile(s), tile(slots))
            _check(st, tile(exp), labels * reps, "form %d wg=%d wq=%d" % (form, wg, wq))
    finally:
        a.set_small_batch_inverse(-1)
        a.set_small_batch_form(-1)


@pytest.mark.parametrize("wg,wq", PAIRS)
def test_large(context, small, monkeypatch, wg, wq):
    """k_verify (4,096 items plus one pass over the vectors): G and then Q on
    one lane through comb_step, which is where the collision vectors bring the
    accumulator onto +-the addend at windows 0, 1, 2, mid - 1, mid, S - 2 and
    S - 1; both batched inverse forms."""
    a = context(wg)
    xy, e, r, s, exp, labels = small[wq]
    slots = _register(a, xy, wq)
    n = 4096 + len(labels)
    idx = np.arange(n) % len(labels)
    for form in ("local", "levels"):
        monkeypatch.setenv("MBFT_NINV", form)
        st = a.verify_prehashed(e[idx], r[idx], s[idx], slots[idx])
        _check(st, exp[idx], [labels[i] for i in idx], "%s wg=%d wq=%d" % (form, wg, wq))


@pytest.mark.parametrize("form,host_u,hjm", [("two", "1", "4"), ("one", "1", "4"), ("two", "0", "4"),
                                             ("two", "1", "0"), ("one", "1", "0")])
@pytest.mark.parametrize("wq", (4, 7))
def test_resident(lib, monkeypatch, wq, form, host_u, hjm):
    """Resident lone calls (k_verify_server), msg = e and tag = DER(r, s).
    One workgroup: two ranges of ceil(S / 2) windows a scalar, past the
    preload.  Two workgroups: four ranges of S / 4 a scalar, the last window
    of each handed out on its own (`extra`); u1 / u2 from the host or the
    waves, the partial sums joined on the host or the GPU."""
    from minbft_amd.authenticator import ROLE_CLIENT, Authenticator
    from oracle import p256 as o
    monkeypatch.setenv("MBFT_RESIDENT_FORM", form)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_U", host_u)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_JOIN_MAX", hjm)
    vecs = resident_vectors(wq)
    a = Authenticator(0)
    try:
        a.set_key_window(wq)
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, bytes.fromhex(vecs[0]["qx"] + vecs[0]["qy"]))
        assert a.key_class(ROLE_CLIENT, 0)[0] == wq
        a.set_resident(8)
        got = [a.verify_status(ROLE_CLIENT, 0, bytes.fromhex(v["e"]),
                               o.der_encode_sig(int(v["r"], 16), int(v["s"], 16))) for v in vecs]
        assert a.resident_stats()["calls"] == len(vecs)
    finally:
        a.close()
    bad = [(v["label"], g) for v, g in zip(vecs, got) if g != (0 if v["expect"] else 1)]
    assert not bad, bad[:10]


SEQUENTIAL_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import torch
torch.cuda.init()
import test_gpu_small_windows as t
from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
from oracle import p256 as o
for wq in (4, 7):
    xy, e, r, s, exp, labels = t.vectors_of(wq)
    with Authenticator(0) as a:
        a.set_generator_window(wq)
        a.set_key_window(wq)
        slots, valid = a.register_points(xy)
        assert valid.all()
        a.set_small_batch_form(256)
        st = np.concatenate([a.verify_prehashed(e[k:k + 200], r[k:k + 200], s[k:k + 200], slots[k:k + 200])
                             for k in range(0, len(labels), 200)])
        bad = [(wq, labels[i], int(st[i])) for i in range(len(e)) if int(st[i] == 0) != exp[i]]
        assert not bad, bad
    vecs = t.resident_vectors(wq)
    with Authenticator(0) as a:
        a.set_key_window(wq)
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, bytes.fromhex(vecs[0]["qx"] + vecs[0]["qy"]))
        a.set_resident(8)
        got = [a.verify_status(ROLE_CLIENT, 0, bytes.fromhex(v["e"]),
                               o.der_encode_sig(int(v["r"], 16), int(v["s"], 16))) for v in vecs]
        assert a.resident_stats()["calls"] == len(vecs)
        bad = [(wq, v["label"], g) for v, g in zip(vecs, got) if (g == 0) != bool(v["expect"])]
        assert not bad, bad
print("small windows sequential ok")
"""


def test_split_sequential(lib):
    """The sequential additions of the split form and of the resident
    one-workgroup form (MBFT_SPLIT_WIDE=0, read once per process: one
    subprocess) at W = 4 and 7, generator and key: k_verify_split<false> and
    k_verify_server<false, *> over the same ranges."""
    env = dict(os.environ, MBFT_SPLIT_WIDE="0", MBFT_RESIDENT_FORM="one")
    p = subprocess.run([sys.executable, "-c", SEQUENTIAL_SCRIPT, ROOT], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "small windows sequential ok" in p.stdout


def test_mixed_windows_in_one_wave(context, monkeypatch):
    """Windows 4, 7 and 16, a table-free and a compact (4 teeth) key side by
    side under a W = 20 generator (13 steps): the items' keys rotate item by
    item, so every lane quad and pair of a wave runs a comb of another length
    (64, 37, 16 steps) beside the ladder classes' dead lanes.  A context
    stores a point once, so five keys take the five classes -- the fixture
    key with its 492 crafted vectors, three keys of prehashed.json, the key of
    teeth_edges.json -- and the classes rotate over the keys from run to run
    (set_slot_classes): every key's vectors meet every class.  130 items
    through the pairs and quads (forms 0 .. 3), 4,096 + 130 through k_verify
    and its queues (both inverse forms); every status is the fixture's, and
    the same as with every key at W = 16."""
    from minbft_amd._lib import key_class_teeth
    a = context(20)
    parts = []
    sx, se, sr, ss, sexp, slab = prehashed_arrays(NAME)
    mine = np.array([":comb_" not in l for l in slab])
    parts.append(tuple(v[mine] for v in (sx, se, sr, ss, sexp)))
    fixture_key = bytes(sx[0])
    px, pe, pr, ps, pexp, _ = prehashed_arrays()
    keys, cnt = np.unique(px, axis=0, return_counts=True)
    others = [k for k, c in zip(keys, cnt) if c >= 60 and bytes(k) != fixture_key][:3]
    assert len(others) == 3
    for k in others:
        m = (px == k).all(axis=1)
        parts.append(tuple(v[m] for v in (px, pe, pr, ps, pexp)))
    tx, te, tr, ts, texp, _ = prehashed_arrays("teeth_edges.json")
    m = (tx == tx[0]).all(axis=1)
    assert m.sum() >= 200 and bytes(tx[0]) != fixture_key
    parts.append(tuple(v[m] for v in (tx, te, tr, ts, texp)))
    nk = len(parts)
    assert len(parts[0][4]) == 492 and len({bytes(p[0][0]) for p in parts}) == nk
    classes = [4, 7, 16, 0, key_class_teeth(4)]

    def batch(n, shift):
        """Item i: key i % nk, that key's vector number i // nk + shift."""
        rows = [(i % nk, (i // nk + shift) % len(parts[i % nk][4])) for i in range(n)]
        e, r, s, exp = (np.stack([parts[k][c][j] for k, j in rows]) for c in (1, 2, 3, 4))
        return e, r, s, exp, np.array([k for k, _ in rows])

    def run(slot_of, what):
        out = []
        a.set_small_batch_form(0)
        try:
            for form in (0, 1, 2, 3):
                a.set_small_batch_inverse(form)
                # (another 26 vectors of each key for every form)
                e, r, s, exp, key = batch(130, 26 * form)
                st = a.verify_prehashed(e, r, s, slot_of[key])
                _check(st, exp, ["key%d" % k for k in key], "%s form %d" % (what, form))
                out.append(st)
        finally:
            a.set_small_batch_inverse(-1)
            a.set_small_batch_form(-1)
        e, r, s, exp, key = batch(4096 + 130, 0)
        for form in ("local", "levels"):
            monkeypatch.setenv("MBFT_NINV", form)
            st = a.verify_prehashed(e, r, s, slot_of[key])
            _check(st, exp, ["key%d" % k for k in key], "%s %s" % (what, form))
            out.append(st)
        return out

    a.clear_keys()
    a.set_key_window(16)
    slots, valid = a.register_points(np.stack([p[0][0] for p in parts]))
    assert valid.all() and len(set(slots.tolist())) == nk
    want = run(slots, "all W=16")
    for rot in range(nk):
        for k in range(nk):
            a.set_slot_classes(slots[k:k + 1], classes[(k + rot) % nk])
        got = run(slots, "rotation %d" % rot)
        assert all((g == w).all() for g, w in zip(got, want)), rot
