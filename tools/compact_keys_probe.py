"""What the compact key class (mbft_set_key_teeth) costs and
buys on one MI355X, beside the table-free class and the smallest comb window.
The method of tools/tablefree_probe.py, in ONE process:

  (a) mbft_verify_prehashed_device at n = 4,096, 65,536 and 1,048,576 items,
      device to device, for: every item compact at t = 2, 3, 4, 6, 8; the same
      keys at window 0; the same keys at W = 4; a 50 / 50 mix of window-0 and
      t = 4 items (alternating, so every wave holds both: the shared queue's
      divergence cost); 1 % compact (t = 4) among W = 29 / 29 items --
      each with 64 signer keys (the tables stay in cache) and again with
      100,000 (the per-lane gathers leave it);
  (b) registration of 100,000 keys in one call at t = 4, at window 0 and at
      W = 4: time and device memory taken.

Each figure: warm-up calls first, then `--reps` timed calls (host clock
around a call that ends in a device synchronise); reported as the median with
the minimum and maximum.  The yardstick of every ratio is the window-0 row of
the same run.  Writes one JSON document.

    python tools/compact_keys_probe.py [--out profiles/compact_keys_probe.json] [--reps 9]
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
TEETH = (2, 3, 4, 6, 8)
# field reductions for u2 Q by the formulas, window 0: ~2,900
PREDICTED = {2: 1980, 3: 1430, 4: 1100, 6: 760, 8: 570, 0: 2900}
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def summary(ts, n=None):
    med = statistics.median(ts)
    out = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "reps": len(ts)}
    if n:
        out["mverify_per_s"] = n / med / 1e6
        out["ns_per_item"] = med / n * 1e9
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_keys_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-w29", action="store_true", help="leave the 1 % mix among W = 29 / 29 items out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compact_keys_probe needs a GPU")
    torch.cuda.init()
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
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
    d29 = int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1  # the one W = 29 key of the 1 % mix
    xy29 = xy_of([o.pubkey(d29)])

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

    doc = {"sizes": list(SIZES), "pools": list(POOLS), "reps": args.reps,
           "predicted_reductions_u2Q": {str(k): v for k, v in PREDICTED.items()}, "verify": {}, "register": {}}
    w29 = None
    if not args.skip_w29:
        w29 = Authenticator(0)
        w29.set_generator_window(29)
        w29.set_key_window(29)
        s29, v29 = w29.register_points(xy29)
        assert v29.all()
    for K in POOLS:
        xy, priv = xy_of(pts[:K]), priv_of(ds_all[:K])
        kidx = (np.arange(nmax) % K).astype(np.uint32)
        with Authenticator(0) as a:  # signatures of the whole pool, once
            r, s = a.sign_prehashed(priv, e, kidx)
        d_r, d_s = torch.from_numpy(r).to(dev), torch.from_numpy(s).to(dev)
        res = {}
        cases = [("teeth_%d" % t, [("t", t)]) for t in TEETH] + [("window_0", [("w", 0)]), ("w4", [("w", 4)]),
                                                                  ("half_window_0_half_teeth_4", [("w", 0), ("t", 4)])]
        for name, classes in cases:
            with Authenticator(0) as a:
                slots = np.zeros(K, dtype=np.uint32)
                for ci, (kind, v) in enumerate(classes):  # key i takes class i mod len(classes)
                    (a.set_key_teeth if kind == "t" else a.set_key_window)(v)
                    sl, valid = a.register_points(xy[ci::len(classes)])
                    assert valid.all()
                    slots[ci::len(classes)] = sl
                res[name] = {str(n): timed(a, d_r, d_s, slots[kidx], n) for n in SIZES}
            print(K, name, json.dumps(res[name]), flush=True)
        if w29 is not None:
            # 1 % of the items under compact keys (t = 4), the rest under ONE W = 29 key, generator at 29
            w29.set_key_teeth(4)
            s4, v4 = w29.register_points(xy)
            assert v4.all()
            mixk = np.where(np.arange(nmax) % 100 == 0, (np.arange(nmax) // 100) % K, K).astype(np.uint32)
            r2, s2 = w29.sign_prehashed(np.concatenate([priv, priv_of([d29])]), e, mixk)
            slots = np.concatenate([s4, s29]).astype(np.uint32)[mixk]
            res["one_percent_teeth_4_among_w29"] = {
                str(n): timed(w29, torch.from_numpy(r2).to(dev), torch.from_numpy(s2).to(dev), slots, n)
                for n in SIZES}
            if K == POOLS[0]:
                r3, s3 = w29.sign_prehashed(priv_of([d29]), e)
                res["all_w29"] = {
                    str(n): timed(w29, torch.from_numpy(r3).to(dev), torch.from_numpy(s3).to(dev),
                                  np.full(nmax, s29[0], dtype=np.uint32), n) for n in SIZES}
            print(K, "w29", json.dumps({k: v for k, v in res.items() if "w29" in k}), flush=True)
        # measured ratios against the window-0 row of THIS run, beside the reduction counts' prediction
        big = str(max(SIZES))
        base = res["window_0"][big]["median_ms"]
        res["ratio_to_window_0_at_1M"] = {
            name: {"measured": res[name][big]["median_ms"] / base,
                   "predicted": (PREDICTED[int(name.split("_")[1])] / PREDICTED[0]) if name.startswith("teeth_") else None}
            for name in res if name != "window_0" and big in res[name]}
        doc["verify"]["keys_%d" % K] = res
    if w29 is not None:
        w29.close()

    # (b) 100,000 keys in one registration call
    kxy = xy_of(pts[:100000])
    for name, kind, v in (("teeth_4", "t", 4), ("window_0", "w", 0), ("w4", "w", 4)):
        ts, mem = [], []
        for _ in range(3):
            with Authenticator(0) as a:
                (a.set_key_teeth if kind == "t" else a.set_key_window)(v)
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
