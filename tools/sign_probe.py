"""Throughput of the batch signer on one MI355X, at n = 4,096,
65,536 and 1,048,576 signatures per call:

  (a) mbft_generate_tags_prehashed_device (k_sign_tags), device to device,
      for the signer windows 4, 5 and 6;
  (b) mbft_sign_messages_flat, host to host, REPLY records with 256-byte
      results (records and arena uploaded, AuthenBytes + SHA-256 + signature +
      DER on the GPU, tags downloaded), at the default window;
  (c) the existing mbft_sign_prehashed_device (k_sign: gather comb over the
      verifier's generator table, home-made nonce, raw r and s) at the same n
      in the same process -- the comparison point, not a bar.

Each figure: warm-up calls first, then `--reps` timed calls (host clock around
a call that ends in a device synchronise), the windows of (a) and (c)
alternating round by round; reported as the median with the minimum and
maximum.  Writes one JSON document.

    python tools/sign_probe.py [--out profiles/sign_probe.json] [--reps 9]
"""
from __future__ import annotations

import argparse
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
WINDOWS = (4, 5, 6)
DEFAULT_WINDOW = 5  # kSignDefaultWindow
N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def summary(ts, n):
    med = statistics.median(ts)
    return {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "reps": len(ts), "msig_per_s": n / med / 1e6}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign_probe.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sign_probe needs a GPU")
    torch.cuda.init()
    from minbft_amd import _lib
    from minbft_amd.authenticator import Authenticator, ROLE_REPLICA

    dev = torch.device("cuda", 0)
    d = int.from_bytes(hashlib.sha256(b"sign-probe").digest(), "big") % (N_ORDER - 1) + 1
    per_round = max(1, args.reps // args.rounds)
    res = {"device": torch.cuda.get_device_name(0), "sizes": list(SIZES), "default_window": DEFAULT_WINDOW, "a_kernel_device": {},
           "b_messages_host": {}, "c_k_sign_device": {}, "ratio_a_over_c": {}}

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
        a.set_private_key(ROLE_REPLICA, d.to_bytes(32, "big"))
        st = torch.cuda.current_stream().cuda_stream
        d_priv = torch.from_numpy(np.frombuffer(d.to_bytes(32, "big"), dtype=np.uint8).copy()).to(dev)
        for n in SIZES:
            g = torch.Generator(device="cpu").manual_seed(n)
            d_e = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).to(dev)
            d_tags = torch.empty((n, _lib.TAG_SLOT), dtype=torch.uint8, device=dev)
            d_lens = torch.empty(n, dtype=torch.uint8, device=dev)
            d_r = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            d_s = torch.empty((n, 32), dtype=torch.uint8, device=dev)

            def new():
                a.generate_tags_prehashed_device(ROLE_REPLICA, d_e.data_ptr(), n, d_tags.data_ptr(),
                                                 d_lens.data_ptr(), st)

            def old():
                a.sign_prehashed_device(d_priv.data_ptr(), 0, d_e.data_ptr(), n, d_r.data_ptr(),
                                        d_s.data_ptr(), st)

            ta = {w: [] for w in WINDOWS}
            tc = []
            for _ in range(args.rounds):
                for w in WINDOWS:
                    a.set_signer_window(w)
                    timed(new, 2)  # warm-up: builds the window's table
                    ta[w] += timed(new, per_round)
                timed(old, 2)
                tc += timed(old, per_round)
            assert int(d_lens.min()) >= 8  # every item signed
            res["a_kernel_device"][str(n)] = {str(w): summary(ta[w], n) for w in WINDOWS}
            res["c_k_sign_device"][str(n)] = summary(tc, n)
            res["ratio_a_over_c"][str(n)] = {
                str(w): statistics.median(ta[w]) / statistics.median(tc) for w in WINDOWS}

            # (b) REPLY records with 256-byte results, host to host, default window
            a.set_signer_window(DEFAULT_WINDOW)
            recs = np.zeros(n, dtype=_lib.msg_rec_dtype())
            recs["type"] = _lib.MSG_REPLY
            recs["client_id"] = 7
            recs["seq"] = np.arange(n, dtype=np.uint64)
            recs["op_len"] = 256
            recs["op_off"] = np.arange(n, dtype=np.uint64) * 256
            arena = np.random.default_rng(n).integers(0, 256, size=256 * n, dtype=np.uint8)
            tb = []
            tags = lens = None
            for k in range(2 + args.reps):
                t0 = time.perf_counter()
                tags, lens = a.sign_messages_flat(recs, arena)
                if k >= 2:
                    tb.append(time.perf_counter() - t0)
            assert int(lens.min()) >= 8
            res["b_messages_host"][str(n)] = summary(tb, n)
            print(n, json.dumps({"a": res["a_kernel_device"][str(n)], "b": res["b_messages_host"][str(n)],
                                 "c": res["c_k_sign_device"][str(n)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
