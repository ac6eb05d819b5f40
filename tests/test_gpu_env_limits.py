"""Environment knobs cannot push a batch into a staging layout it does not
have (batch.cpp host_inv_max): MBFT_HOST_INV_MAX far above the
zero-copy batch size used to make a 5,000-call batch write its host s^-1
planes past the end of the split staging.  It is clamped to the zero-copy
batches; a subprocess (the knob is read once per process) verifies batches
of 1, 50, 64, 65, 4,096 and 5,000 calls -- tampered ones among them -- with
the knob at 100,000, every status against the construction.

MBFT_LANE_INV_MAX below MBFT_HOST_INV_MAX cannot leave a batch on the host's
planes short of spill scratch either (the launch plan sizes it,
verify_plan.h; tests/test_verify_plan.py holds the sizes): with the lane
limit at 0, host planes up to 512 calls and the split kernel off, batches of
65, 256, 257 and 300 calls take the lane quads on the host's planes; among
them the zero-digit items of tests/golden/scalar_edges.json, whose comb steps
spill, under key window 8."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
sizes, split_max, with_edges = [int(x) for x in sys.argv[2].split(",")], int(sys.argv[3]), sys.argv[4] == "1"
import torch
torch.cuda.init()
from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
from oracle import p256 as o
d = int.from_bytes(hashlib.sha256(b"env limits").digest(), "big") % o.N
calls = []
for k in range(64):
    msg = o.authen_request(k + 1, bytes([k]) * 100)
    r, s = o.ecdsa_sign(d, o.quirk_digest(msg))
    calls.append((7, msg, o.der_encode_sig(r, s), None))
edges = []
if with_edges:
    # msg = e (the digest is the message's first 32 bytes), tag = DER(r, s); never tampered
    from golden_util import load
    edges = load("scalar_edges.json")
    calls = [(8, bytes.fromhex(v["e"]), o.der_encode_sig(int(v["r"], 16), int(v["s"], 16)),
              0 if v["expect"] else 1) for v in edges] + calls
with Authenticator(0) as a:
    a.set_key_window(8)
    a.add_role(ROLE_CLIENT)
    a.set_public_key(ROLE_CLIENT, 7, o.pkix_encode(o.pubkey(d)))
    if edges:
        a.set_public_key(ROLE_CLIENT, 8, bytes.fromhex(edges[0]["qx"] + edges[0]["qy"]))
    a.set_small_batch_form(split_max)
    for n in sizes:
        items, want = [], []
        for i in range(n):
            key, msg, tag, fixed = calls[i % len(calls)]
            if fixed is not None:
                want.append(fixed)
            elif i % 7 == 3:
                msg = bytes([msg[0] ^ 1]) + msg[1:]
                want.append(1)
            else:
                want.append(0)
            items.append((ROLE_CLIENT, key, msg, tag))
        got = [int(x) for x in a.verify_batch(items)]
        assert got == want, (n, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:10])
print("env limits ok")
"""


def _run(env, sizes, split_max, with_edges):
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, ",".join(map(str, sizes)), str(split_max),
                        "1" if with_edges else "0"], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "env limits ok" in p.stdout


def test_host_inv_max_clamped(lib):
    _run({"MBFT_HOST_INV_MAX": "100000"}, (1, 50, 64, 65, 4096, 5000), -1, False)


def test_host_planes_past_lane_inv_max(lib):
    _run({"MBFT_LANE_INV_MAX": "0", "MBFT_HOST_INV_MAX": "512"}, (65, 256, 257, 300), 0, True)
