"""What the verified-call memo costs and saves on one MI355X:
mbft_check_messages_flat over windows of 1,024 and 16,384 messages of a
C3-style stream (a backup's view: REQUEST, PREPARE and the COMMITs of the other
replicas per request), n = 4 and n = 33 replicas, the device route
(mbft_set_small_check 0).  p50 of `--passes` timed passes after 3 of warm-up,
with the minimum and maximum; wall time of the C-ABI call, which ends
synchronized.

  off        the memo off (the same line is the parent commit's when the tool
             is run in a tree that has no memo: it then measures nothing else);
  off_again  the same once more in the same process: the run-to-run spread;
  all_miss   memo on and cleared before every pass: the stage's overhead, the
             read-back route's extra wait included;
  all_hit    memo on, the same window repeated: the ceiling;
  rolling    every window brings new REQUESTs and PREPAREs and the COMMITs that
             embed the PREVIOUS window's PREPAREs: the realistic case, with
             its hit rate from the counters, beside the same windows memo off.

Each (n, window) step runs in a child process under its own time limit; the
run stops at the first step that fails.

    python tools/memo_probe.py [--out profiles/memo_probe.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 3
STEP_LIMIT_S = 420
CLIENT = 7


def summary(ts):
    return {"p50_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "passes": len(ts)}


def seeded(tag):
    from oracle import p256 as o
    d = int.from_bytes(hashlib.sha256(tag.encode()).digest(), "big") % (o.N - 1) + 1
    return d


class Stream:
    """Requests of a C3 stream signed by the library's own batch signers: the
    client's signatures by mbft_generate_tags_flat, the UIs by
    mbft_sign_prehashed under each replica's USIG key."""

    def __init__(self, a, nrep):
        from oracle import p256 as o
        self.o, self.a, self.n = o, a, nrep
        self.usig = [seeded(f"probe usig {nrep} {i}") for i in range(nrep)]
        self.cli = seeded(f"probe client {nrep}")
        self.epoch = [0x1000 + i for i in range(nrep)]
        self.ctr = [0] * nrep
        self.seq = 0
        self.rng = np.random.default_rng(nrep)

    def register(self, a):
        o = self.o
        a.set_key_window(8)
        a.add_role(o.ROLE_USIG)
        a.add_role(o.ROLE_CLIENT)
        for i, d in enumerate(self.usig):
            a.set_public_key(o.ROLE_USIG, i, o.pkix_encode(o.pubkey(d)))
        a.set_public_key(o.ROLE_CLIENT, CLIENT, o.pkix_encode(o.pubkey(self.cli)))
        a.enable_usig(True)
        a.set_small_check(0)

    def requests(self, count):
        from minbft_amd.authenticator import Authenticator
        o = self.o
        out = []
        for _ in range(count):
            self.seq += 1
            out.append(o.Msg(type=o.MSG_REQUEST, stream=1000, client_id=CLIENT, seq=self.seq,
                             op=self.rng.bytes(32)))
        tags, lens = self.a.generate_tags(o.ROLE_CLIENT, [o.msg_authen_bytes(m) for m in out])
        for m, t in zip(out, Authenticator.tag_bytes(tags, lens)):
            m.sig = t
        return out

    def _sign_uis(self, msgs, signer):
        """ui_cert of every message, under replica signer[k]'s USIG key."""
        o = self.o
        e = np.zeros((len(msgs), 32), dtype=np.uint8)
        priv = np.array([list(d.to_bytes(32, "big")) for d in self.usig], dtype=np.uint8)
        for k, (m, rid) in enumerate(zip(msgs, signer)):
            self.ctr[rid] += 1
            m.ui_counter = self.ctr[rid]
            e[k] = np.frombuffer(o.usig_digest(o.msg_authen_bytes(m), self.epoch[rid], m.ui_counter), dtype=np.uint8)
        r, s = self.a.sign_prehashed(priv, e, key_idx=np.array(signer, dtype=np.uint32))
        for k, (m, rid) in enumerate(zip(msgs, signer)):
            sig = o.der_encode_sig(int.from_bytes(bytes(r[k]), "big"), int.from_bytes(bytes(s[k]), "big"))
            m.ui_cert = struct.pack(">Q", self.epoch[rid]) + sig

    def prepares(self, reqs):
        o = self.o
        out = [o.Msg(type=o.MSG_PREPARE, stream=0, replica_id=0, view=0, client_id=CLIENT, seq=rq.seq, op=rq.op,
                     sig=rq.sig) for rq in reqs]
        self._sign_uis(out, [0] * len(out))
        return out

    def commits(self, preps):
        o = self.o
        out, signer = [], []
        for pr in preps:
            for rid in range(1, self.n):
                out.append(o.Msg(type=o.MSG_COMMIT, stream=rid, replica_id=rid, prep_replica_id=0, view=0,
                                 client_id=CLIENT, seq=pr.seq, op=pr.op, sig=pr.sig,
                                 prep_ui_counter=pr.ui_counter, prep_ui_cert=pr.ui_cert))
                signer.append(rid)
        self._sign_uis(out, signer)
        return out


def pack(a, msgs):
    from minbft_amd import _lib
    arr, keep = _lib.make_messages(msgs)
    packed = np.frombuffer(arr, dtype=_lib.message_dtype(), count=len(msgs))
    recs, arena = a.pack_messages(packed, True)
    del keep
    return recs, arena


def one_pass(a, window, nrep, expect_valid=False):
    recs, arena = window
    t0 = time.perf_counter()
    b = a.check_messages_flat(recs, arena, nrep)
    dt = time.perf_counter() - t0
    if expect_valid:  # (outside the timed span)
        out = b.resolve_range(0, recs.shape[0])
        assert not out.any(), np.nonzero(out)[0][:5]
    b.close()
    return dt


def step(nrep, size, passes):
    from minbft_amd.authenticator import Authenticator
    has_memo = hasattr(Authenticator, "set_verified_memo")
    fig = {"has_memo": has_memo}
    with Authenticator(0) as a:
        sm = Stream(a, nrep)
        sm.register(a)
        a.set_private_key(sm.o.ROLE_CLIENT, sm.cli.to_bytes(32, "big"))
        per = size // (nrep + 1)
        pad = size - per * (nrep + 1)
        # the closed window: every request with its PREPARE and COMMITs
        reqs = sm.requests(per + pad)
        preps = sm.prepares(reqs[:per])
        closed = pack(a, reqs + preps + sm.commits(preps))
        assert closed[0].shape[0] == size
        one_pass(a, closed, nrep, expect_valid=True)

        def run(label, before=None):
            ts = []
            for _ in range(WARM + passes):
                if before:
                    before()
                ts.append(one_pass(a, closed, nrep))
            fig[label] = summary(ts[WARM:])

        run("off")
        run("off_again")
        if has_memo:
            memo = 1 << 30
            a.set_verified_memo(memo)
            run("all_miss", before=a.clear_verified_memo)
            st0 = a.verified_memo_stats()
            run("all_hit")
            st1 = a.verified_memo_stats()
            fig["all_hit"]["hit_rate"] = (st1["hits"] - st0["hits"]) / max(1, st1["lookups"] - st0["lookups"])
            a.set_verified_memo(0)
        # the rolling windows: window k = the REQUESTs and PREPAREs of batch k and the COMMITs of batch k - 1
        nwin = WARM + passes
        windows, prev = [], sm.prepares(sm.requests(per))
        for _ in range(nwin):
            rq = sm.requests(per + pad)
            pr = sm.prepares(rq[:per])
            windows.append(pack(a, rq + pr + sm.commits(prev)))
            prev = pr
        assert all(w[0].shape[0] == size for w in windows)
        ts = [one_pass(a, w, nrep) for w in windows]
        fig["rolling_off"] = summary(ts[WARM:])
        if has_memo:
            a.set_verified_memo(1 << 30)
            st0 = a.verified_memo_stats()
            ts = [one_pass(a, w, nrep) for w in windows]
            st1 = a.verified_memo_stats()
            fig["rolling"] = summary(ts[WARM:])
            fig["rolling"]["hit_rate"] = (st1["hits"] - st0["hits"]) / max(1, st1["lookups"] - st0["lookups"])
            fig["rolling"]["dropped"] = st1["dropped"] - st0["dropped"]
    return fig


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memo_probe.json"))
    ap.add_argument("--passes", type=int, default=30)
    ap.add_argument("--step", nargs=2, type=int, metavar=("N", "WINDOW"), help="(internal) run one step")
    args = ap.parse_args(argv)
    if args.step:
        print("STEP " + json.dumps(step(args.step[0], args.step[1], args.passes)), flush=True)
        return 0
    doc = {"passes": args.passes, "warmup": WARM, "figures": {}}
    for nrep in (4, 33):
        for size in (1024, 16384):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--step",
                                str(nrep), str(size)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
            line = [x for x in p.stdout.split("\n") if x.startswith("STEP ")]
            if p.returncode != 0 or not line:
                print(f"n={nrep} window={size}: failed rc={p.returncode}\n{p.stderr[-2000:]}", flush=True)
                return 1
            doc["figures"][f"n={nrep} window={size}"] = json.loads(line[0][5:])
            print(f"n={nrep} window={size}", line[0][5:], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
