"""What the key memory budget's ranking costs on one MI355X,
at 10,000, 100,000 and 1,000,000 registered table-free keys.  Medians of
`--reps` timed calls after warm-up, with the minimum and maximum; wall time of
the C-ABI call, which ends synchronized.

  rank_no_move      mbft_rebalance_keys where no key moves: stream synchronize,
                    k_key_hist, the 16-KB histogram down, the plan (the call
                    ends there: with nothing to move no list is made);
  cold_pick         mbft_cold_keys(0, 1000): k_key_pick in cold mode and its
                    list down -- 99 % of the slots are cold, so the call makes
                    the second pass with room for all, then sorts;
  host_choice       the parent commit's path for the same decision, unchanged
                    in this tree: mbft_promote_hot_keys with max_keys 0 --
                    mbft_key_usage's download of both counters of every slot,
                    the candidates sorted on the host, nothing re-classed;
  rebalance_1pct_up / _down
                    one full mbft_rebalance_keys that moves 1 % of the keys
                    from table-free to signed 3 teeth, and back after the
                    counts were aged to zero.

    python tools/key_budget_probe.py [--out profiles/key_budget_probe.json]
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
S3 = 0x203
POPS = (10000, 100000, 1000000)


def summary(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "reps": len(ts)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_budget_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args(argv)
    from minbft_amd.authenticator import Authenticator
    from oracle import p256 as o
    xy = np.zeros((max(POPS), 64), dtype=np.uint8)
    p = o.G
    for i in range(len(xy)):  # key i is (i + 2) G
        p = o.point_add(p, o.G)
        xy[i] = np.frombuffer(p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big"), dtype=np.uint8)
    rng = np.random.default_rng(3)
    doc = {"reps": args.reps, "figures": {}}
    for pop in POPS:
        fig = {}
        with Authenticator(0) as a:
            a.set_key_window(0)
            slots, valid = a.register_points(xy[:pop])
            assert valid.all()
            a.set_key_accounting(True)
            hot = slots[:: 100]                      # 1 % of the keys
            n = 16 * len(hot)
            # (the counts do not ask for valid signatures: a rejected item is a use of its key)
            e, r, s = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(3))
            load_slots = np.tile(hot, 16)

            def load():
                a.verify_prehashed(e, r, s, load_slots)
            load()
            ladder = [0, S3]
            a.set_key_budget(64 * pop + 192 * len(hot))
            # no key moves: a floor on the uses nobody reaches
            for k in range(3 + args.reps):
                fig.setdefault("rank_no_move", []).append(timed(lambda: a.rebalance_keys(ladder, 1 << 40)))
                fig.setdefault("cold_pick", []).append(timed(lambda: a.cold_keys(0, 1000)))
                fig.setdefault("host_choice", []).append(timed(lambda: a.promote_hot_keys(S3, 0, 1)))
            assert a.cold_keys(0, 1)[1] == pop - len(hot) and a.key_memory()[0] == 64 * pop
            for k in range(1 + args.reps):
                res = {}
                fig.setdefault("rebalance_1pct_up", []).append(timed(lambda: res.update(a.rebalance_keys(ladder))))
                assert res["promoted"] == len(hot) and res["demoted"] == 0, res
                a.age_key_usage(63)
                fig.setdefault("rebalance_1pct_down", []).append(timed(lambda: res.update(a.rebalance_keys(ladder))))
                assert res["demoted"] == len(hot) and res["live_after"] == 64 * pop, res
                load()
        skip = {"rank_no_move": 3, "cold_pick": 3, "host_choice": 3, "rebalance_1pct_up": 1, "rebalance_1pct_down": 1}
        doc["figures"][str(pop)] = {k: summary(ts[skip[k]:]) for k, ts in fig.items()}
        print(pop, json.dumps(doc["figures"][str(pop)]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
