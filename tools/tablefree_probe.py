"""What the table-free key class (key window 0) costs and buys on
one MI355X:

  (a) mbft_verify_prehashed_device at n = 4,096, 65,536 and 1,048,576 items,
      device to device, for: every item under table-free keys; 1 % of the
      items table-free among W = 29 / 29 items; and the same keys at W = 4
      and W = 8 (generator at the default window for the first and the last
      two, at 29 for the 1 % mix);
  (b) one VerifyMessageAuthenTag call under a table-free key and under a
      W = 16 key;
  (c) registration of 100,000 keys in one call at window 0 and at W = 4.

Each figure: warm-up calls first, then `--reps` timed calls (host clock
around a call that ends in a device synchronise); reported as the median with
the minimum and maximum.  Writes one JSON document.

    python tools/tablefree_probe.py [--out profiles/tablefree_probe.json] [--reps 9]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tablefree_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-w29", action="store_true", help="leave the 1 % mix among W = 29 / 29 items out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tablefree_probe needs a GPU")
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

    def timed(a, slots, n):
        d_sl = torch.from_numpy(slots[:n].astype(np.uint32).view(np.int32)).to(dev)
        d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call():
            a.verify_prehashed_device(d_e.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_sl.data_ptr(), n,
                                      d_st.data_ptr(), st)
            torch.cuda.synchronize()
        for _ in range(3):
            call()
        assert int((d_st != 0).sum()) == 0, "a valid signature was not accepted"
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return summary(ts, n)

    doc = {"sizes": list(SIZES), "keys": KEYS, "reps": args.reps, "verify": {}, "lone_call": {}, "register": {}}
    for name, w in (("all_table_free", 0), ("all_w4", 4), ("all_w8", 8)):
        with Authenticator(0) as a:
            a.set_key_window(w)
            slots, valid = a.register_points(xy)
            assert valid.all()
            doc["verify"][name] = {str(n): timed(a, slots[kidx], n) for n in SIZES}
            doc["verify"][name]["windows"] = list(a.windows())
        print(name, json.dumps(doc["verify"][name]), flush=True)
    if not args.skip_w29:
        # 1 % of the items under table-free keys, the rest under ONE W = 29 key, generator at 29
        with Authenticator(0) as a:
            a.set_generator_window(29)
            a.set_key_window(29)
            s29, _ = a.register_points(xy[:1])
            a.set_key_window(0)
            s0, _ = a.register_points(xy[1:])
            d1 = np.array(list(ds[0].to_bytes(32, "big")), dtype=np.uint8)[None, :]
            mix = np.where(np.arange(nmax) % 100 == 0, 1 + (np.arange(nmax) // 100) % (KEYS - 1), 0)
            r2, s2 = a.sign_prehashed(priv, e, mix.astype(np.uint32))
            d_r.copy_(torch.from_numpy(r2))
            d_s.copy_(torch.from_numpy(s2))
            slots = np.where(mix == 0, s29[0], s0[np.maximum(mix, 1) - 1]).astype(np.uint32)
            doc["verify"]["one_percent_table_free_among_w29"] = {str(n): timed(a, slots, n) for n in SIZES}
            slots = np.full(nmax, s29[0], dtype=np.uint32)
            r3, s3 = a.sign_prehashed(d1, e)
            d_r.copy_(torch.from_numpy(r3))
            d_s.copy_(torch.from_numpy(s3))
            doc["verify"]["all_w29"] = {str(n): timed(a, slots, n) for n in SIZES}
        print("w29", json.dumps({k: doc["verify"][k] for k in ("one_percent_table_free_among_w29", "all_w29")}),
              flush=True)

    # (b) a lone VerifyMessageAuthenTag call
    msg = o.authen_request(1, bytes(range(256)))
    rr, ss = o.ecdsa_sign(ds[0], o.quirk_digest(msg))
    tag = o.der_encode_sig(rr, ss)
    for name, w in (("table_free", 0), ("w16", 16)):
        with Authenticator(0) as a:
            a.set_key_window(w)
            a.add_role(ROLE_CLIENT)
            a.set_public_key(ROLE_CLIENT, 7, bytes(xy[0]))
            for _ in range(20):
                assert a.verify_status(ROLE_CLIENT, 7, msg, tag) == 0
            ts = []
            for _ in range(max(args.reps, 50)):
                t0 = time.perf_counter()
                a.verify_status(ROLE_CLIENT, 7, msg, tag)
                ts.append(time.perf_counter() - t0)
            doc["lone_call"][name] = summary(ts)
    print("lone", json.dumps(doc["lone_call"]), flush=True)

    # (c) 100,000 keys in one registration call: multiples of G
    pts, p = [], o.G
    for _ in range(100000):
        p = o.point_add(p, o.G)
        pts.append(p)
    kxy = np.array([list(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")) for q in pts], dtype=np.uint8)
    for name, w in (("window_0", 0), ("w4", 4)):
        ts = []
        for _ in range(3):
            with Authenticator(0) as a:
                a.set_key_window(w)
                t0 = time.perf_counter()
                _, valid = a.register_points(kxy)
                ts.append(time.perf_counter() - t0)
                assert valid.all()
        doc["register"][name] = dict(summary(ts), keys=len(pts))
    print("register", json.dumps(doc["register"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
