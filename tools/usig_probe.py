"""Throughput of the software USIG on one MI355X, at n = 4,096,
65,536 and 1,048,576 UIs per call, host to host, into preallocated outputs:

  (u) mbft_usig_create_uis_digests: 32-byte digests up, k_usig_uis, 88-byte
      UI slots and lengths down;
  (m) mbft_usig_sign_messages_flat: PREPARE records with 256-byte operations
      (records and arena up; SHA-256 of the operation, AuthenBytes, the digest
      chain, signature and UI on the GPU);
  (t) mbft_generate_tags_prehashed in the same process -- the ECDSA roles'
      batch generator, unchanged by the USIG work: the yardstick;
  (k) mbft_generate_tags_prehashed_device (k_sign_tags alone, device to
      device, window 5) -- to compare with profiles/sign_probe.json, since the
      two kernels now share one signer function.

Each figure: 2 warm-up calls, then `--reps` timed calls (host clock around a
call that returns after its device synchronise), the four alternating round by
round; reported as the median with the minimum and maximum.  Writes one JSON
document.

    python tools/usig_probe.py [--out profiles/usig_probe.json] [--reps 9]
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4096, 65536, 1 << 20)
N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def summary(ts, n):
    med = statistics.median(ts)
    return {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "reps": len(ts), "m_per_s": n / med / 1e6}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usig_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("usig_probe needs a GPU")
    torch.cuda.init()
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator, ROLE_REPLICA

    dev = torch.device("cuda", 0)
    d = int.from_bytes(hashlib.sha256(b"usig-probe").digest(), "big") % (N_ORDER - 1) + 1
    per_round = max(1, args.reps // args.rounds)
    res = {"device": torch.cuda.get_device_name(0), "sizes": list(SIZES),
           "u_usig_digests_host": {}, "m_usig_messages_host": {}, "t_tags_prehashed_host": {},
           "k_sign_tags_device_w5": {}, "ratio_u_over_t": {}}

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    with Authenticator(0) as a:
        lib, ctx = a.lib, a.ctx
        a.set_private_key(ROLE_REPLICA, d.to_bytes(32, "big"))
        a.usig_init(d.to_bytes(32, "big"), 0x0102030405060708)
        st = torch.cuda.current_stream().cuda_stream
        first = ctypes.c_uint64(0)
        p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        for n in SIZES:
            e = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)
            uis = np.zeros((n, _lib.UI_SLOT), dtype=np.uint8)
            ulen = np.zeros(n, dtype=np.uint8)
            tags = np.zeros((n, _lib.TAG_SLOT), dtype=np.uint8)
            tlen = np.zeros(n, dtype=np.uint8)
            recs = np.zeros(n, dtype=_lib.msg_rec_dtype())
            recs["type"] = _lib.MSG_PREPARE
            recs["client_id"] = 7
            recs["view"] = 3
            recs["seq"] = np.arange(n, dtype=np.uint64)
            recs["op_len"] = 256
            recs["op_off"] = np.arange(n, dtype=np.uint64) * 256
            arena = np.random.default_rng(n + 1).integers(0, 256, size=256 * n, dtype=np.uint8)
            d_e = torch.from_numpy(e).to(dev)
            d_tags = torch.empty((n, _lib.TAG_SLOT), dtype=torch.uint8, device=dev)
            d_lens = torch.empty(n, dtype=torch.uint8, device=dev)

            def check(rc):
                if rc != 0:
                    raise SystemExit(f"call failed: {rc} {a.last_error()}")

            def fu():
                check(lib.mbft_usig_create_uis_digests(ctx, p(e), n, p(uis), p(ulen), ctypes.byref(first)))

            def fm():
                check(lib.mbft_usig_sign_messages_flat(ctx, p(recs), n, p(arena), arena.nbytes, p(uis), p(ulen),
                                                       ctypes.byref(first)))

            def ft():
                check(lib.mbft_generate_tags_prehashed(ctx, ROLE_REPLICA, p(e), n, p(tags), p(tlen)))

            def fk():
                a.generate_tags_prehashed_device(ROLE_REPLICA, d_e.data_ptr(), n, d_tags.data_ptr(),
                                                 d_lens.data_ptr(), st)

            fns = {"u_usig_digests_host": fu, "m_usig_messages_host": fm, "t_tags_prehashed_host": ft,
                   "k_sign_tags_device_w5": fk}
            ts = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    timed(fn, 2)
                    ts[k] += timed(fn, per_round)
            assert int(ulen.min()) >= 24 and int(tlen.min()) >= 8 and int(d_lens.min()) >= 8
            for k in fns:
                res[k][str(n)] = summary(ts[k], n)
            res["ratio_u_over_t"][str(n)] = (statistics.median(ts["u_usig_digests_host"]) /
                                             statistics.median(ts["t_tags_prehashed_host"]))
            print(n, json.dumps({k: res[k][str(n)] for k in fns}), flush=True)
        res["counters_used"] = a.usig_next_counter() - 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
