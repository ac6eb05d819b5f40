"""Measure the P-384 class and write profiles/p384_probe.json.

Medians with min-max over 9 timed calls after 3 of warm-up:
  * mbft_verify_prehashed_p384_keys_device at 4,096, 65,536 and 1,048,576 items;
  * one lone mbft_scheme_verify_p384_flat32 call;
  * yardstick 1: the P-256 inline-key class (mbft_verify_prehashed_keys_device)
    at the same sizes in the same process;
  * yardstick 2: libcrypto's secp384r1 ECDSA_do_verify on one CPU thread.

    python tools/p384_probe.py [--sizes 4096,65536,1048576] [--out profiles/p384_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, TIMED = 3, 9


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def rate(stat, n):
    out = dict(stat)
    out["items"] = n
    out["items_per_s_median"] = n / stat["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p384_probe.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]

    import torch
    torch.cuda.init()
    import p384_ref as o
    from golden_util import prehashed_arrays
    from minbft_amd.authenticator import Authenticator

    with open(os.path.join(ROOT, "tests", "golden", "p384_edges.json")) as f:
        vecs = [v for v in json.load(f) if v["kind"] == "prehashed" and v["status"] == 0]
    rows = lambda k: np.array([list(bytes.fromhex(v[k])) for v in vecs], dtype=np.uint8)  # noqa: E731
    e3, r3, s3 = rows("e"), rows("r"), rows("s")
    xy3 = np.concatenate([rows("x"), rows("y")], axis=1)
    xy2, e2, r2, s2, exp2, _ = prehashed_arrays()
    ok2 = np.nonzero(exp2 == 1)[0]
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "timed": TIMED, "p384_device": [], "p256_inline_device": []}

    with Authenticator(0) as auth:
        for n in sizes:
            idx = np.arange(n) % len(vecs)
            d = [torch.from_numpy(v[idx]).to(dev) for v in (e3, r3, s3, xy3)]
            st = torch.zeros(n, dtype=torch.uint8, device=dev)

            def call384():
                auth.verify_prehashed_p384_keys_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                       n, st.data_ptr(), 0)
                torch.cuda.synchronize()

            res["p384_device"].append(rate(timed(call384), n))
            assert int(st.sum().item()) == 0, "every probe item is a valid signature"
            idx2 = ok2[np.arange(n) % len(ok2)]
            d2 = [torch.from_numpy(v[idx2]).to(dev) for v in (e2, r2, s2, xy2)]
            st2 = torch.zeros(n, dtype=torch.uint8, device=dev)

            def call256():
                auth.verify_prehashed_keys_device(d2[0].data_ptr(), d2[1].data_ptr(), d2[2].data_ptr(), d2[3].data_ptr(),
                                                  n, st2.data_ptr(), 0)
                torch.cuda.synchronize()

            res["p256_inline_device"].append(rate(timed(call256), n))
            assert int(st2.sum().item()) == 0
            print(n, res["p384_device"][-1]["median_s"], res["p256_inline_device"][-1]["median_s"], flush=True)
        # a lone scheme call
        dd = 0x384384
        q = o.pubkey(dd)
        msg = b"REQUEST" + bytes(range(64))
        rr, ss = o.ecdsa_sign(dd, o.hash_to_int(o.scheme_digest(msg)))
        call = (msg, o.der_encode_sig(rr, ss), o.pkix_encode(q)[24:])
        assert auth.scheme_verify_p384([call]).tolist() == [0]
        res["p384_scheme_single_call"] = timed(lambda: auth.scheme_verify_p384([call]))

    # libcrypto, one thread
    from oracle import openssl_xcheck
    lib = openssl_xcheck.load()
    if lib is None:
        res["libcrypto_secp384r1_one_thread"] = None
    else:
        key = lib.EC_KEY_new_by_curve_name(715)
        bn = lambda x: lib.BN_bin2bn(x.to_bytes(48, "big"), 48, None)  # noqa: E731
        assert lib.EC_KEY_set_public_key_affine_coordinates(key, bn(q[0]), bn(q[1])) == 1
        sig = lib.ECDSA_SIG_new()
        lib.ECDSA_SIG_set0(sig, bn(rr), bn(ss))
        md = o.scheme_digest(msg)
        reps = 2000

        def cpu():
            for _ in range(reps):
                rc = lib.ECDSA_do_verify(md, len(md), sig, key)
            assert rc == 1

        res["libcrypto_secp384r1_one_thread"] = rate(timed(cpu), reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
