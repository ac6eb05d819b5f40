"""The corners of the comb's signed-digit recoding through every verify form.

tests/golden/scalar_edges.json holds signatures crafted from chosen
(u1, u2) under one key (make_golden.make_scalar_edges): scalars in
[N - 2^200, N), whose recoding carries into the top window and reads the LAST
entry of the comb table (digit 2^L) at every window; windows exactly 2^(W-1),
the largest positive digit and the last entry of a non-top window; a window
of all ones plus a carry (a zero digit that still carries); 0x81.. / 0x7f..
around the recoding threshold; 1 and 2 -- as u1, as u2 and as both, each
followed by the same with a flipped digest.  An attacker who picks s chooses
u2, and no other golden vector has such scalars.

Every kernel form recodes on its own (comb_step in k_verify, verify_pair,
verify_quad's high lanes, comb_range_uniform in k_verify_split, the resident
kernel with host or device u1 / u2), so the whole file runs through each of
them at key windows 8, 13 (partial last window, L = 9) and 16 and generator
windows 16 and 20 (L = 16 < W).  A form that mis-carries into the top
window, clamps a digit, or reads one entry short of a window's end rejects
an accepting vector here.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import load, prehashed_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "scalar_edges.json"
KEY_WINDOWS = (8, 13, 16)
GEN_WINDOWS = (16, 20)


def _check(st, exp, labels):
    got = (st == 0).astype(np.int64)
    bad = [(labels[i], int(st[i]), int(exp[i])) for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, bad[:20]


@pytest.fixture(scope="module")
def edges():
    xy, e, r, s, exp, labels = prehashed_arrays(NAME)
    assert len(labels) == 54 and exp.sum() == 27 and (xy == xy[0]).all()
    return xy, e, r, s, exp, labels


@pytest.fixture(scope="module", params=GEN_WINDOWS)
def auth(lib, request):
    """One context per generator window (the W = 20 table is 388 MiB, built
    once for all the forms below)."""
    from minbft_amd.authenticator import Authenticator
    a = Authenticator(0)
    a.set_generator_window(request.param)
    yield a
    a.close()


def _register(a, xy, wq):
    a.clear_keys()
    a.set_key_window(wq)
    assert a.windows()[1] == wq
    slots, valid = a.register_points(xy[:1])
    assert valid.all()
    return slots[0]


@pytest.mark.parametrize("wq", KEY_WINDOWS)
def test_split_kernel(auth, edges, wq):
    """k_verify_split (one item per workgroup, comb_range_uniform): a wrong
    digit or index at a window's last entry in the wave-uniform recoding."""
    xy, e, r, s, exp, labels = edges
    slot = _register(auth, xy, wq)
    auth.set_small_batch_form(256)
    try:
        st = auth.verify_prehashed(e, r, s, np.full(len(e), slot, dtype=np.uint32))
    finally:
        auth.set_small_batch_form(-1)
    _check(st, exp, labels)


@pytest.mark.parametrize("wq", KEY_WINDOWS)
def test_pairs_and_quads(auth, edges, wq):
    """Past the split kernel's range (the file tiled to 324 items): lane pairs
    inverting per lane (0), lane pairs on the s^-1 planes (1), lane quads
    inline (2) and on the planes (3).  verify_pair splits the windows between
    two lanes and verify_quad's high lanes replay the carry chain up to their
    first window: a carry lost at that seam rejects an accepting vector."""
    xy, e, r, s, exp, labels = edges
    slot = _register(auth, xy, wq)
    reps = 6
    tile = lambda x: np.concatenate([x] * reps)  # noqa: E731
    assert len(labels) * reps > 256
    auth.set_small_batch_form(0)
    try:
        for form in (0, 1, 2, 3):
            auth.set_small_batch_inverse(form)
            st = auth.verify_prehashed(tile(e), tile(r), tile(s),
                                       np.full(len(e) * reps, slot, dtype=np.uint32))
            _check(st, tile(exp), [f"form{form}:{l}" for l in labels * reps])
    finally:
        auth.set_small_batch_inverse(-1)
        auth.set_small_batch_form(-1)


@pytest.mark.parametrize("wq", KEY_WINDOWS)
def test_large_batch(auth, edges, monkeypatch, wq):
    """k_verify's comb_step (the file tiled past 4,096 items), on the s^-1
    planes of both batched inverse forms."""
    xy, e, r, s, exp, labels = edges
    slot = _register(auth, xy, wq)
    n = 4096 + 54
    idx = np.tile(np.arange(len(labels)), -(-n // len(labels)))[:n]
    for form in ("local", "levels"):
        monkeypatch.setenv("MBFT_NINV", form)
        st = auth.verify_prehashed(e[idx], r[idx], s[idx], np.full(n, slot, dtype=np.uint32))
        _check(st, exp[idx], [f"{form}:{labels[i]}" for i in idx])


def _resident_calls(a, vecs):
    from minbft_amd.authenticator import ROLE_CLIENT
    from oracle import p256 as o
    a.add_role(ROLE_CLIENT)
    a.set_public_key(ROLE_CLIENT, 0, bytes.fromhex(vecs[0]["qx"] + vecs[0]["qy"]))
    calls = [(ROLE_CLIENT, 0, bytes.fromhex(v["e"]), o.der_encode_sig(int(v["r"], 16), int(v["s"], 16)))
             for v in vecs]
    return calls, [0 if v["expect"] else 1 for v in vecs]


@pytest.mark.parametrize("form,host_u,hjm", [("two", "1", "4"), ("one", "1", "4"), ("two", "0", "4"),
                                             ("two", "1", "0"), ("one", "1", "0")])
@pytest.mark.parametrize("wq", KEY_WINDOWS)
def test_resident_calls(lib, monkeypatch, wq, form, host_u, hjm):
    """Resident single calls (k_verify_server), msg = e and tag = DER(r, s):
    one or two workgroups per item, u1 / u2 from the host or computed by the
    waves, partial sums joined on the host or on the GPU.  Each wave recodes
    its own window range from the scalar's words."""
    from minbft_amd.authenticator import Authenticator
    monkeypatch.setenv("MBFT_RESIDENT_FORM", form)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_U", host_u)
    monkeypatch.setenv("MBFT_RESIDENT_HOST_JOIN_MAX", hjm)
    vecs = load(NAME)
    a = Authenticator(0)
    try:
        a.set_key_window(wq)
        calls, want = _resident_calls(a, vecs)
        a.set_resident(8)
        got = [a.verify_status(*c) for c in calls]
        assert a.resident_stats()["calls"] == len(calls)
    finally:
        a.close()
    bad = [(vecs[i]["label"], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:10]


SEQUENTIAL_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import torch
torch.cuda.init()
from golden_util import load, prehashed_arrays
from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
from oracle import p256 as o
xy, e, r, s, exp, labels = prehashed_arrays("scalar_edges.json")
vecs = load("scalar_edges.json")
for wq in (8, 13, 16):
    with Authenticator(0) as a:
        a.set_key_window(wq)
        slots, valid = a.register_points(xy[:1])
        assert valid.all()
        a.set_small_batch_form(256)
        st = a.verify_prehashed(e, r, s, np.full(len(e), slots[0], dtype=np.uint32))
        bad = [(wq, labels[i], int(st[i])) for i in range(len(e)) if int(st[i] == 0) != exp[i]]
        assert not bad, bad
    with Authenticator(0) as a:
        a.set_key_window(wq)
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, bytes.fromhex(vecs[0]["qx"] + vecs[0]["qy"]))
        a.set_resident(8)
        got = [a.verify_status(ROLE_CLIENT, 0, bytes.fromhex(v["e"]),
                               o.der_encode_sig(int(v["r"], 16), int(v["s"], 16))) for v in vecs]
        bad = [(wq, v["label"], g) for v, g in zip(vecs, got) if (g == 0) != bool(v["expect"])]
        assert not bad, bad
print("scalar edges sequential ok")
"""


def test_split_sequential_additions(lib):
    """The split and resident kernels' sequential additions
    (MBFT_SPLIT_WIDE=0, read once per process: a subprocess, as
    test_gpu_env_limits does) take the same recoding through
    k_verify_split<false> / k_verify_server<false, *>."""
    env = dict(os.environ, MBFT_SPLIT_WIDE="0")
    p = subprocess.run([sys.executable, "-c", SEQUENTIAL_SCRIPT, ROOT], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "scalar edges sequential ok" in p.stdout
