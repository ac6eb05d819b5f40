"""What the inline-key class (mbft_verify_prehashed_keys*)
costs on one MI355X, beside its yardstick:

  (a) mbft_verify_prehashed_keys_device at n = 4,096, 65,536 and 1,048,576
      items, device to device, 64 signer keys given inline, generator at the
      default window;
  (b) THE SAME items under the same keys registered table-free (key window 0)
      through mbft_verify_prehashed_device, in the same process -- the existing
      path that runs the same ladder;
  (c) one lone call: the scheme form and the host prehashed form with one item
      under an inline key, and VerifyMessageAuthenTag under the same key
      registered table-free.

Each figure: warm-up calls first, then `--reps` timed calls (host clock around
a call that ends in a device synchronise); reported as the median with the
minimum and maximum.  Writes one JSON document.

    python tools/inline_keys_probe.py [--out profiles/inline_keys_probe.json] [--reps 9]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 65536, 1 << 20)
KEYS = 64  # distinct signer keys of the verify batches
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def summary(ts, n=None):
    med = statistics.median(ts)
    out = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "reps": len(ts)}
    if n:
        out["mverify_per_s"] = n / med / 1e6
        out["us_per_item"] = med / n * 1e6
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inline_keys_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inline_keys_probe needs a GPU")
    torch.cuda.init()
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT
    from oracle import p256 as o
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)

    ds = [int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(KEYS)]
    priv = np.array([list(d.to_bytes(32, "big")) for d in ds], dtype=np.uint8)
    xy = np.array([list(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")) for q in map(o.pubkey, ds)],
                  dtype=np.uint8)
    nmax = max(SIZES)
    e = rng.integers(0, 256, size=(nmax, 32), dtype=np.uint8)
    kidx = (np.arange(nmax) % KEYS).astype(np.uint32)
    with Authenticator(0) as a:  # signatures of the whole pool, once
        r, s = a.sign_prehashed(priv, e, kidx)
    d_e, d_r, d_s = (torch.from_numpy(v).to(dev) for v in (e, r, s))
    d_xy = torch.from_numpy(np.ascontiguousarray(xy[kidx])).to(dev)

    def timed(call, d_st, n):
        for _ in range(3):
            call()
        assert int((d_st != 0).sum()) == 0, "a valid signature was not accepted"
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return summary(ts, n)

    doc = {"sizes": list(SIZES), "keys": KEYS, "reps": args.reps, "verify": {"inline": {}, "registered_table_free": {}},
           "lone_call": {}}
    st = torch.cuda.current_stream().cuda_stream
    with Authenticator(0) as inl, Authenticator(0) as reg:
        reg.set_key_window(0)
        slots, valid = reg.register_points(xy)
        assert valid.all()
        d_sl = torch.from_numpy(slots[kidx].astype(np.uint32).view(np.int32)).to(dev)
        doc["windows"] = {"inline": list(inl.windows()), "registered_table_free": list(reg.windows())}
        for n in SIZES:  # the two forms in turn at each size, so that they see the same clocks
            d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)

            def call_inline():
                inl.verify_prehashed_keys_device(d_e.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_xy.data_ptr(), n,
                                                 d_st.data_ptr(), st)
                torch.cuda.synchronize()

            def call_registered():
                reg.verify_prehashed_device(d_e.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_sl.data_ptr(), n,
                                            d_st.data_ptr(), st)
                torch.cuda.synchronize()
            doc["verify"]["registered_table_free"][str(n)] = timed(call_registered, d_st, n)
            d_st.fill_(0xAA)
            doc["verify"]["inline"][str(n)] = timed(call_inline, d_st, n)
            print(n, json.dumps({k: doc["verify"][k][str(n)] for k in doc["verify"]}), flush=True)

        # (c) one lone call
        msg = o.authen_request(1, bytes(range(256)))
        rr, ss = o.ecdsa_sign(ds[0], o.quirk_digest(msg))
        tag = o.der_encode_sig(rr, ss)
        e1 = np.frombuffer(o.quirk_digest(msg)[:32], dtype=np.uint8)[None]
        r1 = np.frombuffer(rr.to_bytes(32, "big"), dtype=np.uint8)[None]
        s1 = np.frombuffer(ss.to_bytes(32, "big"), dtype=np.uint8)[None]
        reg.add_role(ROLE_CLIENT)
        reg.set_public_key(ROLE_CLIENT, 7, bytes(xy[0]))
        forms = {
            "inline_scheme_verify": lambda: int(inl.scheme_verify([(msg, tag, bytes(xy[0]))])[0]),
            "inline_prehashed_host": lambda: int(inl.verify_prehashed_keys(e1, r1, s1, xy[:1])[0]),
            "registered_table_free": lambda: reg.verify_status(ROLE_CLIENT, 7, msg, tag),
        }
        for name, f in forms.items():
            for _ in range(20):
                assert f() == 0
            ts = []
            for _ in range(max(args.reps, 50)):
                t0 = time.perf_counter()
                f()
                ts.append(time.perf_counter() - t0)
            doc["lone_call"][name] = summary(ts)
        print("lone", json.dumps(doc["lone_call"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
