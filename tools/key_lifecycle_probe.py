"""What the life of a key after registration costs and buys
on one MI355X.  The method of tools/compact_keys_probe.py: medians of `--reps`
timed calls after warm-up with the minimum and maximum, a verify being
mbft_verify_prehashed_device ending in a device synchronise.

The yardstick of the accounting cost and of the descriptor upload is the
PARENT commit's build, run alternately with this one on the same box: give a
built checkout of the parent with --yardstick-root and every round runs one
worker process on each tree (`--rounds` rounds, the medians of all of a
tree's calls pooled per figure).

  (a) cost of accounting: 1M items W = 29 / 29 under one key (the most
      contended), 1M items over 100,000 t = 4 keys (the most spread), 4,096
      items of each -- accounting off on both trees, on on this one;
  (b) one key registered among 100,000 and 1,000,000 slots (both trees: the
      whole-array descriptor upload against the partial one), and on this tree
      one key of them re-classed into window 0, t = 4 and W = 8;
  (c) bulk re-class of 1,000 keys in one call, window 0 -> t = 8 and window 0 ->
      W = 8: the first call (fresh storage, one launch) and the later ones
      (every key takes a released piece);
  (d) the pay-off: 1 % of a 1M W = 29 / 29 batch under table-free keys, and a
      lone VerifyMessageAuthenTag under such a key, before and after
      mbft_promote_hot_keys moves those keys to W = 16.

    python tools/key_lifecycle_probe.py [--yardstick-root DIR] [--out profiles/key_lifecycle_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
BIG, SMALL = 1 << 20, 4096
ROLE_CLIENT = 3


def summary(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "reps": len(ts)}


def worker(args):
    """One tree's figures (args.tree on sys.path), raw times in seconds."""
    sys.path.insert(0, args.tree)
    import torch
    torch.cuda.init()
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    dev = torch.device("cuda", 0)
    new = hasattr(Authenticator, "set_key_accounting")
    pts_xy = np.load(args.points)  # (i + 2) G, 64 bytes each
    rng = np.random.default_rng(11)
    e = rng.integers(0, 256, size=(BIG, 32), dtype=np.uint8)
    d_e = torch.from_numpy(e).to(dev)
    out = {}

    def priv_of(ds):
        return np.array([list(int(d).to_bytes(32, "big")) for d in ds], dtype=np.uint8)

    def timed_verify(a, r, s, slots, n, reps=args.reps):
        d_r, d_s = torch.from_numpy(r[:n].copy()).to(dev), torch.from_numpy(s[:n].copy()).to(dev)
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
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return ts

    def timed(fn, reps=args.reps):
        ts = []
        for k in range(reps):
            t0 = time.perf_counter()
            fn(k)
            ts.append(time.perf_counter() - t0)
        return ts

    # (a) and (d): one W = 29 key under a W = 29 generator, 100 table-free keys beside it
    d29 = int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1
    q29 = o.pubkey(d29)
    xy29 = np.array([list(q29[0].to_bytes(32, "big") + q29[1].to_bytes(32, "big"))], dtype=np.uint8)
    K = 100
    with Authenticator(0) as a:
        a.set_generator_window(29)
        a.set_key_window(29)
        s29, v = a.register_points(xy29)
        r, s = a.sign_prehashed(priv_of([d29]), e)
        one = np.full(BIG, s29[0], dtype=np.uint32)
        for n in (BIG, SMALL):
            out["w29_one_key_%d_off" % n] = timed_verify(a, r, s, one, n)
        if new:
            a.set_key_accounting(True)
            for n in (BIG, SMALL):
                out["w29_one_key_%d_on" % n] = timed_verify(a, r, s, one, n)
            a.set_key_accounting(False)
            # (d) 1 % of the items under table-free keys, before and after promotion to W = 16
            a.add_role(ROLE_CLIENT)
            a.set_key_window(0)
            for k in range(K):
                a.set_public_key(ROLE_CLIENT, k, bytes(pts_xy[k]))
            tf = np.array([a.key_slot(ROLE_CLIENT, k) for k in range(K)], dtype=np.uint32)
            mixk = np.where(np.arange(BIG) % 100 == 0, (np.arange(BIG) // 100) % K, K).astype(np.uint32)
            r2, s2 = a.sign_prehashed(np.concatenate([priv_of(range(2, 2 + K)), priv_of([d29])]), e, mixk)
            slots = np.concatenate([tf, s29]).astype(np.uint32)[mixk]
            a.set_private_key(ROLE_CLIENT, (2).to_bytes(32, "big"))  # key 0 is 2 G
            msg = o.authen_request(1, bytes(range(64)))
            tag = a.GenerateMessageAuthenTag(ROLE_CLIENT, msg)

            def lone(_k):
                assert a.verify_status(ROLE_CLIENT, 0, msg, tag) == 0
            a.set_key_accounting(True)
            out["one_percent_window0_1M_before"] = timed_verify(a, r2, s2, slots, BIG)
            timed(lone, 3)
            out["lone_call_before"] = timed(lone, 5 * args.reps)
            t0 = time.perf_counter()
            got = a.promote_hot_keys(16, K, 1)
            out["promote_%d_keys_to_w16" % K] = [time.perf_counter() - t0]
            assert got == K and a.key_class(ROLE_CLIENT, 0)[0] == 16
            out["one_percent_window0_1M_after"] = timed_verify(a, r2, s2, slots, BIG)
            timed(lone, 3)
            out["lone_call_after"] = timed(lone, 5 * args.reps)

    # (a) the most spread: 100,000 t = 4 keys
    K = 100000
    with Authenticator(0) as a:
        a.set_key_teeth(4)
        sl, v = a.register_points(pts_xy[:K])
        kidx = (np.arange(BIG) % K).astype(np.uint32)
        r, s = a.sign_prehashed(priv_of(range(2, 2 + K)), e, kidx)
        for n in (BIG, SMALL):
            out["t4_100k_keys_%d_off" % n] = timed_verify(a, r, s, sl[kidx], n)
        if new:
            a.set_key_accounting(True)
            for n in (BIG, SMALL):
                out["t4_100k_keys_%d_on" % n] = timed_verify(a, r, s, sl[kidx], n)

    # (b), (c): one key among many slots
    for pop in (100000, 1000000):
        with Authenticator(0) as a:
            a.add_role(ROLE_CLIENT)
            a.set_key_window(0)
            sl, v = a.register_points(pts_xy[:pop])
            extra = pts_xy[pop:pop + 3 + args.reps]

            def reg(k):
                a.set_public_key(ROLE_CLIENT, k, bytes(extra[k]))
            out["register_one_among_%d" % pop] = timed(reg, 3 + args.reps)[3:]
            if new:
                for name, cls, back in (("window0", 0, 0x104), ("t4", 0x104, 0), ("w8", 8, 0)):
                    def rec(k, cls=cls, back=back):
                        a.set_key_class(ROLE_CLIENT, 0, cls)
                    ts = []
                    for k in range(3 + args.reps):
                        a.set_key_class(ROLE_CLIENT, 0, back)
                        ts += timed(rec, 1)
                    out["reclass_one_among_%d_into_%s" % (pop, name)] = ts[3:]
                if pop == 100000:
                    # (c) the first call of a class finds no released storage: one fresh run, one
                    # launch; every later one takes the 1,000 pieces the way back released
                    for name, cls in (("t8", 0x108), ("w8", 8)):
                        ts = []
                        for k in range(1 + args.reps):
                            a.set_slot_classes(sl[:1000], 0)
                            t0 = time.perf_counter()
                            a.set_slot_classes(sl[:1000], cls)
                            ts.append(time.perf_counter() - t0)
                        out["bulk_reclass_1000_keys_window0_to_%s_fresh" % name] = ts[:1]
                        out["bulk_reclass_1000_keys_window0_to_%s_reused" % name] = ts[1:]
    json.dump(out, sys.stdout)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_lifecycle_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--yardstick-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--points", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.worker:
        return worker(args)

    sys.path.insert(0, ROOT)
    from oracle import p256 as o
    count = 1000000 + 3 + args.reps
    xy = np.zeros((count, 64), dtype=np.uint8)
    p = o.G
    for i in range(count):  # key i is (i + 2) G
        p = o.point_add(p, o.G)
        xy[i] = np.frombuffer(p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big"), dtype=np.uint8)
    fd, points = tempfile.mkstemp(suffix=".npy")
    os.close(fd)
    np.save(points, xy)
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(args.yardstick_root))] if args.yardstick_root else [])
    raw = {name: {} for name, _ in trees}
    try:
        for _ in range(args.rounds):
            for name, tree in reversed(trees):  # alternately, the yardstick first
                env = dict(os.environ)
                env.pop("MBFT_LIB_PATH", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree,
                                    "--points", points, "--reps", str(args.reps)],
                                   stdout=subprocess.PIPE, env=env, check=True, timeout=900)
                for k, ts in json.loads(p.stdout.decode().strip().splitlines()[-1]).items():
                    raw[name].setdefault(k, []).extend(ts)
                print(name, "done", flush=True)
    finally:
        os.unlink(points)
    doc = {"reps": args.reps, "rounds": args.rounds,
           "figures": {name: {k: summary(ts) for k, ts in fig.items()} for name, fig in raw.items()}}
    if "parent" in raw:
        cmp_ = {}
        for k, v in doc["figures"]["parent"].items():
            t = doc["figures"]["this"].get(k)
            if t is None:
                continue
            row = {"parent_median_ms": v["median_ms"], "parent_min_ms": v["min_ms"], "parent_max_ms": v["max_ms"],
                   "this_median_ms": t["median_ms"], "inside_parent_min_max": v["min_ms"] <= t["median_ms"] <= v["max_ms"]}
            on = doc["figures"]["this"].get(k[:-4] + "_on") if k.endswith("_off") else None
            if on:
                row["accounting_on_median_ms"] = on["median_ms"]
                row["excess_over_parent_ms"] = on["median_ms"] - v["median_ms"]
                row["allowance_ms"] = (v["max_ms"] - v["min_ms"]) + 0.02 * v["median_ms"]
            cmp_[k] = row
        doc["against_parent"] = cmp_
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("against_parent", doc["figures"]), indent=1))


if __name__ == "__main__":
    main()
