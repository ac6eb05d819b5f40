"""What the signed compact key class (mbft_set_key_signed_teeth, DESIGN.md
§4.10) costs and buys on one MI355X, beside the unsigned compact class AT
EQUAL BYTES PER KEY and beside the table-free class.  The method of
tools/compact_keys_probe.py, in ONE process:

  (a) mbft_verify_prehashed_device at n = 4,096, 65,536 and 1,048,576 items,
      device to device, for: every item signed compact at t = 2 .. 9; the
      same keys unsigned compact at t = 2 .. 8 (signed t and unsigned t - 1
      take the same bytes); the same keys at window 0; a 50 / 50 mix of
      signed 5 and unsigned 4 items (alternating, so every wave holds both:
      the shared body should bring it near the slower of its parts) -- each
      with 64 signer keys (the tables stay in cache) and again with 100,000
      (the per-lane gathers leave it);
  (b) registration of 100,000 keys in one call at signed 5 and at unsigned 4
      (both 1 KiB a key): time and device memory taken.

Each figure: warm-up calls first, then `--reps` timed calls (host clock
around a call that ends in a device synchronise); reported as the median with
the minimum and maximum.  The yardstick of a signed row is the unsigned row of
the same bytes in the same run; the ratio is set beside the one the reduction
counts predict.  Writes one JSON document.

    python tools/signed_teeth_probe.py [--out profiles/signed_teeth_probe.json] [--reps 9]
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
POOLS = (64, 100000)  # distinct signer keys of the verify batches
STEETH = tuple(range(2, 10))
TEETH = tuple(range(2, 9))
# field reductions for u2 Q by the formulas (include/minbft_gpu.h); window 0: ~2,900
PREDICTED_SIGNED = {2: 2286, 3: 1530, 4: 1134, 5: 918, 6: 756, 7: 648, 8: 558, 9: 504}
PREDICTED_UNSIGNED = {2: 1980, 3: 1430, 4: 1100, 5: 912, 6: 760, 7: 655, 8: 570}


def summary(ts, n=None):
    med = statistics.median(ts)
    out = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "reps": len(ts)}
    if n:
        out["mverify_per_s"] = n / med / 1e6
        out["ns_per_item"] = med / n * 1e9
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_teeth_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("signed_teeth_probe needs a GPU")
    torch.cuda.init()
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    nmax = max(SIZES)
    e = rng.integers(0, 256, size=(nmax, 32), dtype=np.uint8)
    d_e = torch.from_numpy(e).to(dev)

    def xy_of(pts):
        return np.array([list(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")) for q in pts], dtype=np.uint8)

    def priv_of(ds):
        return np.array([list(d.to_bytes(32, "big")) for d in ds], dtype=np.uint8)

    # key i is (i + 2) G with private key i + 2, by repeated addition; a pool is the first K of them
    pts, p = [], o.G
    for _ in range(max(POOLS)):
        p = o.point_add(p, o.G)
        pts.append(p)
    ds_all = list(range(2, 2 + max(POOLS)))

    def timed(a, d_r, d_s, slots, n):
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

    setter = {"s": "set_key_signed_teeth", "t": "set_key_teeth", "w": "set_key_window"}
    doc = {"sizes": list(SIZES), "pools": list(POOLS), "reps": args.reps,
           "predicted_reductions_u2Q": {"signed": PREDICTED_SIGNED, "unsigned": PREDICTED_UNSIGNED, "window_0": 2900},
           "verify": {}, "register": {}}
    for K in POOLS:
        xy, priv = xy_of(pts[:K]), priv_of(ds_all[:K])
        kidx = (np.arange(nmax) % K).astype(np.uint32)
        with Authenticator(0) as a:  # signatures of the whole pool, once
            r, s = a.sign_prehashed(priv, e, kidx)
        d_r, d_s = torch.from_numpy(r).to(dev), torch.from_numpy(s).to(dev)
        res = {}
        cases = [("window_0", [("w", 0)])]
        for t in STEETH:  # each signed row next to the unsigned row of the same bytes
            cases.append(("signed_%d" % t, [("s", t)]))
            if t - 1 in TEETH:
                cases.append(("teeth_%d" % (t - 1), [("t", t - 1)]))
        cases.append(("half_signed_5_half_teeth_4", [("s", 5), ("t", 4)]))
        for name, classes in cases:
            with Authenticator(0) as a:
                slots = np.zeros(K, dtype=np.uint32)
                for ci, (kind, v) in enumerate(classes):  # key i takes class i mod len(classes)
                    getattr(a, setter[kind])(v)
                    sl, valid = a.register_points(xy[ci::len(classes)])
                    assert valid.all()
                    slots[ci::len(classes)] = sl
                res[name] = {str(n): timed(a, d_r, d_s, slots[kidx], n) for n in SIZES}
            print(K, name, json.dumps(res[name]), flush=True)
        # measured ratios against the unsigned row of the same bytes and against window 0, per size
        ratios = {}
        for t in STEETH:
            row = {"bytes_per_key": 64 << (t - 1)}
            for n in SIZES:
                m = res["signed_%d" % t][str(n)]["median_ms"]
                row["to_window_0_at_%d" % n] = m / res["window_0"][str(n)]["median_ms"]
                if t - 1 in TEETH:
                    row["to_unsigned_equal_bytes_at_%d" % n] = m / res["teeth_%d" % (t - 1)][str(n)]["median_ms"]
            if t - 1 in TEETH:
                row["predicted_to_unsigned_equal_bytes"] = PREDICTED_SIGNED[t] / PREDICTED_UNSIGNED[t - 1]
            row["predicted_to_window_0"] = PREDICTED_SIGNED[t] / 2900
            ratios["signed_%d" % t] = row
        res["ratios"] = ratios
        doc["verify"]["keys_%d" % K] = res

    # (b) 100,000 keys in one registration call, 1 KiB a key both ways
    kxy = xy_of(pts[:100000])
    for name, kind, v in (("signed_5", "s", 5), ("teeth_4", "t", 4)):
        ts, mem = [], []
        for _ in range(3):
            with Authenticator(0) as a:
                getattr(a, setter[kind])(v)
                torch.cuda.synchronize()
                free0 = torch.cuda.mem_get_info(0)[0]
                t0 = time.perf_counter()
                _, valid = a.register_points(kxy)
                ts.append(time.perf_counter() - t0)
                mem.append(free0 - torch.cuda.mem_get_info(0)[0])
                assert valid.all()
        doc["register"][name] = dict(summary(ts), keys=len(kxy), device_bytes_taken=int(statistics.median(mem)))
    print("register", json.dumps(doc["register"]), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
