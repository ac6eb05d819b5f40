#!/usr/bin/env python3
"""Benchmark: ECDSA-P256 verifies/sec at batch 1M (BASELINE.json `metric`).

Workload (BASELINE.json configs[1]): per GPU, a batch of
1,048,576 single-signer REQUEST authenticators.  Each item is what
Authenticator.VerifyMessageAuthenTag(ClientAuthen, 0, msg, tag) checks for a
256-byte-operation REQUEST (sample/authentication/crypto.go:113-126):
msg = AuthenBytes(REQUEST) = "REQUEST" || seq_be64 || SHA256(op) (47 B,
messages/authen.go:33,54-56), digest = msg || SHA256("") so e = msg[0:32],
tag = DER(r, s) decoded to (r, s).  Operations come from a seeded PCG64;
signatures from the library's GPU signer (deterministic nonces).  Every 97th
item of the batch is then altered (reject_mix: a flipped byte of e, s = N,
r = 0, which reject, or s replaced by N - s, which Go accepts), so the
statuses a step returns hold accepts and rejects at known places.

One step = one pass of the hot path over one batch with inputs resident in
HBM: the batched s^-1 kernels + the verify kernel
(mbft_verify_prehashed_device), signed-digit comb tables at 29-bit windows
for G and the signer key (258 GiB of the GPU's 288 GB; built once, outside
the timed region, `table_build_s`).  Batches alternate between two caller streams so
that batch i+1's s^-1 kernels and verify kernel overlap batch i's (DESIGN.md
§4).  W untimed warmup steps, then exactly K steps bracketed by barrier +
synchronize; time = max over ranks; value = all ranks' verifies / time (weak
scaling: each rank verifies its own batch, no data-path collective).

A plain run does that and no more: tables and inputs, the correctness gates
of the timed path, W + K steps, one JSON line (`value`, `ms_per_step`, ...).
--dump-outputs DIR also writes what the last timed step returned (the batch's
statuses: 0 accept, 1 reject) as DIR/statuses.npy; the inputs are seeded, so
two builds can be compared output for output.

With --full the run goes on to every other line and writes them to the
detail file (--detail-out): `roofline` for k_verify (launch duration from HIP
events in the library, on the stream the kernel runs on, one batch at a time;
plus the steady-state figure on ms_per_step), `sha256_stage` (the GPU SHA-256
stage that builds the REQUEST digests), `cpu_baseline` (the C restatement in
oracle/ over a bounded sample on this host, rank 0 only), p50 latencies,
single calls, adversarial input, C3, the Go wiring and binding configurations.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

class _stdout_to_stderr:
    """Point file descriptor 1 at stderr for the duration (C-level writes
    included), so native libraries cannot interleave text with the JSON
    line on stdout."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def comb_steps(w: int) -> int:
    """Windows (= mixed additions) of a w-bit comb over a 256-bit scalar."""
    return -(-256 // w)


def mixed_adds(g_window: int, q_window: int) -> int:
    """Mixed additions per verify: the first two G windows are one
    affine + affine addition, every further G window and every Q window one
    mixed addition."""
    return comb_steps(g_window) - 2 + comb_steps(q_window)


def work_per_verify(g_window: int, q_window: int):
    """Algorithmic work of k_verify per verify in SURVEY.md
    §8(d)'s unit (one M256 = 64 32x32-bit limb products): the affine first
    addition (2M + 2S + the 2 products of Y3 = 6 M256), one mixed addition
    per further comb window of u1 over G and of u2 over Q -- the Chudnovsky
    madd the kernel runs: 6M + 2S + the 2 products of the merged Y3 = 10 M256
    (ecc.h ec_madd_chud) -- plus u1, u2 (2) and the merged projective x-check
    (one two-product reduction, 2).  Also the executed v_mad_u64_u32 count of
    this implementation (29-bit limbs: fe_mul 81 products + 36 reduction + 8
    carry mads, fe_sqr 45 + 44, fe_mul_add 81 + 36 + 8 (its addend enters as
    the top columns' initial values), fe_mul2 162 + 44, plus 6 carry mads for
    each lazy output (ZZ, ZZZ); 1,146 per mixed addition (the ISA count,
    tools/isa_hist.py), 634 for the first, 162 per mod-N product)."""
    adds = mixed_adds(g_window, q_window)
    m256 = 6 + adds * 10 + 2 + 2
    exec_mads = 634 + adds * 1146 + 2 * 162 + 206
    return m256, m256 * 64, exec_mads


# SURVEY.md §8(d)'s yardstick (joint Straus w=4 with 252 doublings): 3,432 M256.
SURVEY_LIMB_MACS_PER_VERIFY = 219_648


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults long enough for the sustained state: the GPU ramps its clock
    # over the first ~20 ms of load and then runs power-capped;
    # 3 warmup + 20 timed steps read ~10 % low (tools/steps_sweep.sh)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other line (SHA-256 stage, roofline, "
                         "latencies, single calls, adversarial, C3, Go wiring, binding configurations, CPU "
                         "baselines) and write the detail file; the options below --streams shape those lines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (the batch's statuses) as DIR/<name>.npy")
    ap.add_argument("--g-window", type=int, default=29,
                    help="generator comb window in bits (4..29; HBM cost in include/minbft_gpu.h)")
    ap.add_argument("--q-window", type=int, default=29,
                    help="signer-key comb window in bits (4..29)")
    ap.add_argument("--latency-reps", type=int, default=20)
    ap.add_argument("--cpu-sample", type=int, default=262144,
                    help="items for the OpenSSL CPU baseline (the port line uses --cpu-port-sample)")
    ap.add_argument("--cpu-port-sample", type=int, default=65536)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--c3-requests", type=int, default=16384,
                    help="requests in the C3 line (34 messages each at f = 16; 0 = skip)")
    ap.add_argument("--streams", type=int, default=3,
                    help="caller streams the batches rotate over (batches in flight)")
    ap.add_argument("--no-adversarial", action="store_true",
                    help="skip the adversarial throughput lines (crafted exact-path items, C4 share)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialize the RCCL process group even at world size 1 (rehearses the "
                         "multi-GPU launch's stream/queue layout on one GPU)")
    ap.add_argument("--no-extra-lines", action="store_true",
                    help="skip the concurrency, binding-configuration and multi-engine lines")
    ap.add_argument("--no-peak-run", action="store_true",
                    help="use the committed microbenchmark peak instead of running tools/ubench_valu")
    ap.add_argument("--gate-batches", type=int, default=30,
                    help="batches of the sustained correctness gate before the warm-up (every status "
                         "checked on the device)")
    ap.add_argument("--detail-out", default=os.path.join(ROOT, "gpurun_out", "bench_detail.json"),
                    help="side file for every line beyond the compact stdout line")
    return ap.parse_args()


def make_requests(rank: int, n: int, with_ops: bool = False):
    """Synthetic REQUEST authen bytes (47 B) for seq = rank*n + 1 .. ; returns
    the (n, 47) array (and the (n, 256) ops and n seqs if with_ops).
    op = 256 bytes from PCG64(0x4D696E42 + rank)."""
    rng = np.random.Generator(np.random.PCG64(0x4D696E42 + rank))
    ops = rng.integers(0, 256, size=(n, 256), dtype=np.uint8)
    out = np.zeros((n, 47), dtype=np.uint8)
    out[:, :7] = np.frombuffer(b"REQUEST", dtype=np.uint8)
    seq = (np.arange(n, dtype=np.uint64) + np.uint64(rank * n + 1)).astype(">u8")
    out[:, 7:15] = seq.view(np.uint8).reshape(n, 8)
    sha = hashlib.sha256
    digs = b"".join(sha(ops[i].tobytes()).digest() for i in range(n))
    out[:, 15:47] = np.frombuffer(digs, dtype=np.uint8).reshape(n, 32)
    if with_ops:
        return out, ops, np.arange(n, dtype=np.uint64) + np.uint64(rank * n + 1)
    return out


def sha256_stage(auth, torch, dev, st, ops: np.ndarray, seqs: np.ndarray, e_ref, reps: int = 10):
    """The GPU SHA-256 stage that feeds the verifier (north_star item 3):
    e = (AuthenBytes(REQUEST) || SHA256(""))[0:32] from raw (seq, op) fields
    in HBM (mbft_request_digests_device).  Checked bit-exact against the
    host-built digests, then timed with HIP events on the stream the kernel
    runs on.  Bytes moved per item: op + seq in, e out."""
    n, op_len = ops.shape
    d_ops = torch.from_numpy(np.ascontiguousarray(ops)).to(dev)
    d_seq = torch.from_numpy(seqs.astype(np.int64)).to(dev)
    d_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    auth.request_digests_device(d_seq.data_ptr(), d_ops.data_ptr(), op_len, n, d_out.data_ptr(),
                                st.cuda_stream)
    torch.cuda.synchronize()
    if not torch.equal(d_out, e_ref):
        raise SystemExit("bench gate failed: GPU REQUEST digests differ from host AuthenBytes")
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        auth.request_digests_device(d_seq.data_ptr(), d_ops.data_ptr(), op_len, n,
                                    d_out.data_ptr(), st.cuda_stream)
    b.record(st)
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    nbytes = n * (op_len + 8 + 32)
    comp = n * ((op_len + 9 + 63) // 64)
    del d_ops, d_seq, d_out
    return {"kernel": "k_request_e_tiled", "items": n, "op_bytes": op_len, "ms": ms,
            "GB_per_s": nbytes / (ms * 1e-3) / 1e9, "hbm_frac": nbytes / (ms * 1e-3) / 8e12,
            "compressions_per_s": comp / (ms * 1e-3), "items_per_s": n / (ms * 1e-3),
            "bound": "valu (64 SHA-256 rounds per 64-B block; 288 B of HBM per item)"}


N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


def reject_mix(torch, dev, d_e, d_r, d_s, B: int):
    """Copies of (e, r, s) with every 97th item altered (kind cycling 0..3):
    0 flips a byte of e, 1 sets s = N, 2 sets r = 0 (all must reject), 3
    replaces s by N - s (high s: Go has no low-s rule, must accept); every
    other item must accept.  Returns (e2, r2, s2, want, counts): want = the
    status of every item by construction."""
    idx = torch.arange(0, B, 97, device=dev)
    kind = (idx // 97) % 4
    e2, r2, s2 = d_e.clone(), d_r.clone(), d_s.clone()
    i0, i1, i2, i3 = (idx[kind == k] for k in range(4))
    e2[i0, 11] ^= 0x40
    s2[i1] = torch.tensor(list(N_ORDER.to_bytes(32, "big")), dtype=torch.uint8, device=dev)
    r2[i2] = 0
    hs = s2[i3].cpu().numpy()
    for k in range(hs.shape[0]):
        hs[k] = np.frombuffer((N_ORDER - int.from_bytes(hs[k].tobytes(), "big")).to_bytes(32, "big"),
                              dtype=np.uint8)
    s2[i3] = torch.from_numpy(hs).to(dev)
    want = torch.zeros((B,), dtype=torch.uint8, device=dev)
    want[torch.cat([i0, i1, i2])] = 1
    return e2, r2, s2, want, {"altered": int(idx.numel()), "rejects": int(i0.numel() + i1.numel() + i2.numel()),
                              "high_s_accepts": int(i3.numel())}


def reject_gate(auth, torch, dev, d_e, d_r, d_s, d_slot, B: int, st):
    """Every 97th item altered (kind cycling 0..3): 0 flips a byte of e, 1
    sets s = N, 2 sets r = 0 (all must reject), 3 replaces s by N - s (high
    s: Go has no low-s rule, must accept); every other item must accept."""
    idx = torch.arange(0, B, 97, device=dev)
    kind = (idx // 97) % 4
    e2, r2, s2 = d_e.clone(), d_r.clone(), d_s.clone()
    i0, i1, i2, i3 = (idx[kind == k] for k in range(4))
    e2[i0, 11] ^= 0x40
    s2[i1] = torch.tensor(list(N_ORDER.to_bytes(32, "big")), dtype=torch.uint8, device=dev)
    r2[i2] = 0
    hs = s2[i3].cpu().numpy()
    for k in range(hs.shape[0]):
        hs[k] = np.frombuffer((N_ORDER - int.from_bytes(hs[k].tobytes(), "big")).to_bytes(32, "big"),
                              dtype=np.uint8)
    s2[i3] = torch.from_numpy(hs).to(dev)
    out = torch.empty((B,), dtype=torch.uint8, device=dev)
    auth.verify_prehashed_device(e2.data_ptr(), r2.data_ptr(), s2.data_ptr(), d_slot.data_ptr(), B,
                                 out.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    want = torch.zeros((B,), dtype=torch.uint8, device=dev)
    want[torch.cat([i0, i1, i2])] = 1
    bad = int((out != want).sum().item())
    if bad:
        raise SystemExit(f"bench reject gate failed: {bad} statuses differ from the construction")
    return {"items": B, "altered": int(idx.numel()), "rejects": int(i0.numel() + i1.numel() + i2.numel()),
            "high_s_accepts": int(i3.numel()), "ok": True}


def _le_rows(vals):
    """Python ints -> (n, 32) big-endian uint8 rows."""
    return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=np.uint8).reshape(-1, 32)


def _ints(rows: np.ndarray):
    return [int.from_bytes(rows[i].tobytes(), "big") for i in range(rows.shape[0])]


def craft_exact_path(auth, torch, dev, d: int, n: int, seed: int):
    """n valid signatures of the signer d whose u2 = r s^-1 has a zero low
    29-bit comb window, so k_verify must hand every one to the exact path:
    pick a nonce k and u2 = v 2^29, get r = x(kG) from the GPU signer, then
    s = r / u2 and e = r (k / u2 - d) (so u1 = e / s = k - d u2 and
    u1 G + u2 Q = kG).  The u2 inverses by one batched inversion."""
    import random
    rng = random.Random(seed)
    N = N_ORDER
    ks = [rng.randrange(1, N) for _ in range(n)]
    u2 = [rng.randrange(1, N >> 29) << 29 for _ in range(n)]
    d_k = torch.from_numpy(_le_rows(ks)).to(dev)
    d_z = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    d_r = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    d_s = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    d_priv = torch.from_numpy(np.frombuffer(d.to_bytes(32, "big"), dtype=np.uint8).copy()).to(dev)
    auth.sign_nonce_device(d_priv.data_ptr(), 0, d_z.data_ptr(), d_k.data_ptr(), n, d_r.data_ptr(),
                           d_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rs = _ints(d_r.cpu().numpy())
    pre = [1] * (n + 1)
    for i in range(n):
        pre[i + 1] = pre[i] * u2[i] % N
    inv = pow(pre[n], -1, N)
    iu2 = [0] * n
    for i in range(n - 1, -1, -1):
        iu2[i] = inv * pre[i] % N
        inv = inv * u2[i] % N
    s_ = [rs[i] * iu2[i] % N for i in range(n)]
    e_ = [rs[i] * ((ks[i] * iu2[i] - d) % N) % N for i in range(n)]
    return (torch.from_numpy(_le_rows(e_)).to(dev), d_r, torch.from_numpy(_le_rows(s_)).to(dev))


def time_batches(auth, torch, streams, batches, reps: int):
    """Median wall time of running every (e, r, s, slot, out, n) batch once,
    batches rotating over the caller streams, synchronized on both sides."""
    ts = []
    for k in range(reps + 1):
        torch.cuda.synchronize()
        a = time.perf_counter()
        for j, (e, r, s, sl, out, n) in enumerate(batches):
            auth.verify_prehashed_device(e.data_ptr(), r.data_ptr(), s.data_ptr(), sl.data_ptr(), n,
                                         out.data_ptr(), streams[j % len(streams)].cuda_stream)
        torch.cuda.synchronize()
        if k:
            ts.append(time.perf_counter() - a)
    return float(np.median(ts))


def adversarial(auth, torch, dev, streams, B: int, d: int, d_e, d_r, d_s, d_slot, base_s: float,
                q_window: int = 29, dist=None, msgs=None):
    """Throughput under adversarial input:
      zero_window_all: every item crafted so that its u2 has a zero comb
                       window (anyone can force this by picking s): resolved
                       in k_verify's rare branch, no exact path;
      exact_path_all:  every item crafted (with the key's discrete log) so
                       that a key-phase mixed addition is degenerate:
                       k_verify queues it, k_verify_slow recomputes it with
                       complete additions (256 distinct crafted items
                       tiled over the batch);
      exact_path_1_per_wave: one degenerate item per 64 (the pattern that
                       made every wave pay the exact path before the queue);
      c4_share:        one GPU's share of C4 at the prehashed entry
                       (8,388,608 items, 8 signer keys at W = 24, an 8 %
                       mix: 2 % tampered e, 2 % wrong key, 2 % r / s out of
                       range, 1 % off-curve key slot, 1 % high s, which
                       accept), every status checked;
      c4_authenticator_level: the same share as VerifyMessageAuthenTag
                       calls with SURVEY §8(d)'s full 10 % mix (c4_calls
                       below), through mbft_verify_batch_flat.
    Values are verifies/s over the whole set (median of 3, synchronized)."""
    out = {}
    t = time.perf_counter()
    ce, cr, cs = craft_exact_path(auth, torch, dev, d, B, 0xAD)
    craft_s = time.perf_counter() - t
    st = torch.empty((B,), dtype=torch.uint8, device=dev)
    dt = time_batches(auth, torch, streams, [(ce, cr, cs, d_slot, st, B)], 3)
    if int((st == 0).sum().item()) != B:
        raise SystemExit("adversarial gate: crafted zero-window items not all accepted")
    out["zero_window_all"] = {"value": B / dt, "items": B, "ms": dt * 1e3,
                              "vs_valid_batch": (B / dt) / (B / base_s), "craft_s": craft_s,
                              "path": "fast (k_verify rare branch)"}
    del ce, cr, cs
    t = time.perf_counter()
    rows = craft_degenerate(d, q_window, 256, 0xDE)
    craft_s = time.perf_counter() - t
    reps = (B + len(rows) - 1) // len(rows)
    ce = torch.from_numpy(np.tile(_le_rows([x[0] for x in rows]), (reps, 1))[:B]).to(dev)
    cr = torch.from_numpy(np.tile(_le_rows([x[1] for x in rows]), (reps, 1))[:B]).to(dev)
    cs = torch.from_numpy(np.tile(_le_rows([x[2] for x in rows]), (reps, 1))[:B]).to(dev)
    dt = time_batches(auth, torch, streams, [(ce, cr, cs, d_slot, st, B)], 3)
    if int((st == 0).sum().item()) != B:
        raise SystemExit("adversarial gate: crafted degenerate items not all accepted")
    out["exact_path_all"] = {"value": B / dt, "items": B, "ms": dt * 1e3,
                             "vs_valid_batch": (B / dt) / (B / base_s), "craft_s": craft_s,
                             "distinct_items": len(rows),
                             "path": "exact (k_verify_slow: degenerate key-phase addition)"}
    me, mr, ms = d_e.clone(), d_r.clone(), d_s.clone()
    me[::64], mr[::64], ms[::64] = ce[::64], cr[::64], cs[::64]
    dt = time_batches(auth, torch, streams, [(me, mr, ms, d_slot, st, B)], 3)
    if int((st == 0).sum().item()) != B:
        raise SystemExit("adversarial gate: 1-per-wave batch not all accepted")
    out["exact_path_1_per_wave"] = {"value": B / dt, "items": B, "ms": dt * 1e3,
                                    "vs_valid_batch": (B / dt) / (B / base_s)}
    del ce, cr, cs, me, mr, ms
    # C4 share: 8 keys at W = 24 (the W = 29 signer key is dropped first)
    n4 = 8 * B
    auth.clear_keys()
    auth.set_key_window(24)
    ds = [int.from_bytes(hashlib.sha256(b"minbft-amd c4 key %d" % i).digest(), "big") % (N_ORDER - 1) + 1
          for i in range(8)]
    xy = np.frombuffer(b"".join(pubkey_bytes(k) for k in ds) + b"\x01" * 64,
                       dtype=np.uint8).reshape(9, 64)  # + one off-curve point
    slots, valid = auth.register_points(xy)
    assert valid[:8].all() and not valid[8]
    rng = np.random.Generator(np.random.PCG64(0xC4))
    kidx = rng.integers(0, 8, size=n4).astype(np.int32)
    e4 = torch.from_numpy(rng.integers(0, 256, size=(n4, 32), dtype=np.uint8)).to(dev)
    d_priv = torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "big") for k in ds),
                                            dtype=np.uint8).copy()).to(dev)
    d_kidx = torch.from_numpy(kidx).to(dev)
    r4 = torch.empty((n4, 32), dtype=torch.uint8, device=dev)
    s4 = torch.empty((n4, 32), dtype=torch.uint8, device=dev)
    auth.sign_prehashed_device(d_priv.data_ptr(), d_kidx.data_ptr(), e4.data_ptr(), n4, r4.data_ptr(),
                               s4.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sl_t = torch.from_numpy(slots.astype(np.int32)).to(dev)
    slot4 = sl_t[d_kidx.long()].clone()
    kind = torch.from_numpy(rng.integers(0, 100, size=n4)).to(dev)
    e4[kind < 2, 7] ^= 0x20                                                # tampered e
    m = (kind >= 2) & (kind < 4)
    slot4[m] = sl_t[((d_kidx[m] + 1) % 8).long()]                          # wrong key
    r4[(kind >= 4) & (kind < 5)] = 0                                       # r = 0
    s4[(kind >= 5) & (kind < 6)] = 0xFF                                    # s = 2^256 - 1
    slot4[(kind >= 6) & (kind < 7)] = int(slots[8])                        # off-curve key slot
    hs = (kind >= 7) & (kind < 8)                                          # high s: accept
    hsn = s4[hs].cpu().numpy()
    s4[hs] = torch.from_numpy(_le_rows([N_ORDER - v for v in _ints(hsn)])).to(dev)
    st4 = torch.empty((n4,), dtype=torch.uint8, device=dev)
    batches = [(e4[j * B:(j + 1) * B], r4[j * B:(j + 1) * B], s4[j * B:(j + 1) * B],
                slot4[j * B:(j + 1) * B], st4[j * B:(j + 1) * B], B) for j in range(8)]
    # all ranks start together (barrier) and the time is the MAX over ranks
    # of each rank's median: C4 (BASELINE.json configs[3]) is N such shares
    from minbft_amd import dist as mdist
    sync = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
    world = dist.get_world_size() if sync else 1
    if sync:
        torch.cuda.synchronize()
        dist.barrier()
    dt_rank = time_batches(auth, torch, streams, batches, 3)
    want = torch.zeros((n4,), dtype=torch.uint8, device=dev)
    want[kind < 6] = 1
    want[(kind >= 6) & (kind < 7)] = 5
    bad = int((st4 != want).sum().item())
    dt = dt_rank
    if sync:
        dt = mdist.max_over_ranks(dist, dt_rank, dev)
        tb = torch.tensor([bad], dtype=torch.int64, device=dev)
        dist.all_reduce(tb)
        bad = int(tb.item())
    if bad:
        raise SystemExit(f"adversarial gate: {bad} C4 statuses differ from the construction")
    mix = ("8 % mix at the prehashed entry (no DER, no digest work): 2% tampered e, 2% wrong key, "
           "2% r/s out of range (r = 0 or s = 2^256-1), 1% off-curve key slot (BAD_KEY), 1% high s (accept); "
           "the full 10 % mix runs at the authenticator level (c4_authenticator_level)")
    out["c4_share"] = {"value": n4 / dt_rank, "items": n4, "ms": dt_rank * 1e3, "keys": 8, "key_window": 24,
                       "mix": mix, "statuses_checked": n4}
    out["c4"] = {"value": world * n4 / dt, "unit": "verifies/s", "n_gpus": world, "items": world * n4,
                 "items_per_gpu": n4, "ms": dt * 1e3, "scaling": "weak",
                 "timing": "ranks start at a barrier; median of 3 passes per rank, MAX over ranks",
                 "mix": mix, "statuses_checked": world * n4, "entry": "mbft_verify_prehashed_device",
                 "config": "BASELINE.json configs[3] (64M = 8 x 8,388,608 at N = 8), prehashed items"}
    del e4, r4, s4, st4, slot4, kind, want, batches
    torch.cuda.empty_cache()
    out["c4_authenticator_level"] = c4_calls(auth, torch, dev, msgs, ds, dist)
    return out


def c4_calls(auth, torch, dev, msgs: np.ndarray, ds, dist=None, n4: int = 8 << 20):
    """C4 (BASELINE.json configs[3]) at the authenticator level:
    one GPU's share of the 64M adversarial batch as VerifyMessageAuthenTag
    (ClientAuthen, id, AuthenBytes(REQUEST), DER tag) calls, through
    mbft_verify_batch_flat over library page-locked buffers (the Go binding's
    path: DER decode, Sum(m) digest and key lookup on the GPU, k_prepare).
    A pool of 1,048,576 distinct REQUESTs signed by 8 clients (W = 24 key
    tables) is tiled to n4 calls, then SURVEY §8(d)'s 10 % mix is applied:
      2 % tampered op (a byte of SHA256(op) inside e)         -> REJECT_SIG
      2 % wrong signer (the next client's id)                  -> REJECT_SIG
      2 % r / s out of range: r = 0, r = N, s = N, s = 2^256-1 -> REJECT_SIG
      1 % "off-curve key": an id with no key -- the reference rejects an
          off-curve key at load (x509, keymanager.go:352-366), so at this
          boundary it is a signer without a key                -> UNKNOWN_KEY
      1 % malformed DER (wrong outer tag)                      -> MALFORMED_DER (Go panics)
      1 % high s (N - s)                                       -> ACCEPT (no low-s rule)
      1 % quirk-mode tamper past byte 32 of the AuthenBytes   -> ACCEPT (crypto.go:121)
    Every status is checked against the construction, and a 4,096-call sample
    against the C oracle.  Median of 3 timed passes after a warm-up."""
    from minbft_amd import dist as mdist
    from minbft_amd.authenticator import ROLE_CLIENT, der_encode_rows, host_array
    from oracle import c_oracle
    nk = len(ds)
    auth.clear_keys()
    auth.set_key_window(24)
    auth.add_role(ROLE_CLIENT)
    qxy = b"".join(pubkey_bytes(k) for k in ds)
    for i in range(nk):
        auth.set_public_key(ROLE_CLIENT, i, qxy[64 * i:64 * i + 64])
    P = msgs.shape[0]
    rng = np.random.Generator(np.random.PCG64(0xC4A))
    kpool = rng.integers(0, nk, size=P).astype(np.uint32)
    d_priv = torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "big") for k in ds),
                                            dtype=np.uint8).copy()).to(dev)
    d_k = torch.from_numpy(kpool.astype(np.int32)).to(dev)
    d_e = torch.from_numpy(np.ascontiguousarray(msgs[:, :32])).to(dev)
    d_r = torch.empty((P, 32), dtype=torch.uint8, device=dev)
    d_s = torch.empty((P, 32), dtype=torch.uint8, device=dev)
    auth.sign_prehashed_device(d_priv.data_ptr(), d_k.data_ptr(), d_e.data_ptr(), P, d_r.data_ptr(),
                               d_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pr, ps = d_r.cpu().numpy(), d_s.cpu().numpy()
    del d_priv, d_k, d_e, d_r, d_s
    pool = np.arange(n4) % P
    kind = rng.integers(0, 100, size=n4)
    r = pr[pool]
    s_ = ps[pool]
    Nb = np.frombuffer(N_ORDER.to_bytes(32, "big"), dtype=np.uint8)
    rs = np.nonzero((kind >= 4) & (kind < 6))[0]
    q = rng.integers(0, 4, size=rs.size)
    r[rs[q == 0]] = 0
    r[rs[q == 1]] = Nb
    s_[rs[q == 2]] = Nb
    s_[rs[q == 3]] = 0xFF
    hs = np.nonzero(kind == 8)[0]
    s_[hs] = _le_rows([N_ORDER - v for v in _ints(s_[hs])])
    tags, tlen = der_encode_rows(r, s_)
    del r, s_
    tags[kind == 7, 0] = 0x31
    m = msgs[pool]
    m[kind < 2, 20] ^= 0x01
    m[kind == 9, 40] ^= 0xFF
    ids = kpool[pool].copy()
    w = (kind >= 2) & (kind < 4)
    ids[w] = (ids[w] + 1) % nk
    ids[kind == 6] = nk + ids[kind == 6]
    want = np.zeros(n4, dtype=np.uint8)
    want[kind < 6] = 1
    want[kind == 6] = 4
    want[kind == 7] = 2
    # flat buffers in library page-locked memory, as go/gpuauth marshals
    # them: the compact form (u8 roles, u32 offsets, each REQUEST as its
    # 32-byte e prefix (msg || SHA256(""))[0:32] = msg[0:32] -- the byte-40
    # tamper is outside it and accepted either way), then the wide form
    # (u32 roles, u64 offsets, the 47-byte AuthenBytes) for comparison
    sync = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
    world = dist.get_world_size() if sync else 1
    tmask = np.arange(tags.shape[1])[None, :] < tlen[:, None]

    def form(compact):
        ml, odt = (32, np.uint32) if compact else (47, np.uint64)
        roles = host_array(n4, np.uint8 if compact else np.uint32)
        roles[:] = ROLE_CLIENT
        ids_h = host_array(n4, np.uint32)
        ids_h[:] = ids
        mo, to = host_array(n4 + 1, odt), host_array(n4 + 1, odt)
        mo[:] = np.arange(n4 + 1, dtype=odt) * ml
        to[0] = 0
        to[1:] = np.cumsum(tlen.astype(odt))
        mb = host_array(ml * n4)
        mb[:] = np.ascontiguousarray(m[:, :ml]).reshape(-1)
        tb = host_array(int(to[n4]))
        tb[:] = tags[tmask]
        return roles, ids_h, mb, mo, tb, to

    def timed(run, arrays, out):
        run(*arrays, out=out)  # warm-up
        if sync:
            torch.cuda.synchronize()
            dist.barrier()
        ts = []
        for _ in range(3):
            a = time.perf_counter()
            run(*arrays, out=out)
            ts.append(time.perf_counter() - a)
        return float(np.median(ts))

    out = host_array(n4)
    wide = form(False)
    dt_wide = timed(auth.verify_flat_arrays, wide, out)
    bad_wide = int((np.array(out) != want).sum())
    wide_bytes = int(sum(a.nbytes for a in wide) + out.nbytes)
    del wide
    comp = form(True)
    dt_rank = timed(auth.verify_flat32_arrays, comp, out)
    host_bytes = int(sum(a.nbytes for a in comp) + out.nbytes)
    del comp
    got = np.array(out)
    bad = int((got != want).sum()) + bad_wide
    # a C-oracle sample (the calls with a key: the oracle takes key slots)
    idx = rng.choice(np.nonzero(kind != 6)[0], size=4096, replace=False)
    ost = c_oracle.verify_ecdsa_role_batch(
        np.frombuffer(qxy, dtype=np.uint8), ids[idx],
        [m[i].tobytes() for i in idx], [tags[i, :tlen[i]].tobytes() for i in idx])
    obad = int((ost != got[idx]).sum())
    dt = dt_rank
    if sync:
        dt = mdist.max_over_ranks(dist, dt_rank, dev)
        tb_ = torch.tensor([bad + obad], dtype=torch.int64, device=dev)
        dist.all_reduce(tb_)
        bad = int(tb_.item())
        obad = 0
    if bad or obad:
        raise SystemExit(f"C4 authenticator gate: {bad} statuses differ from the construction, "
                         f"{obad} from the C oracle sample")
    counts = {name: int(c) for name, c in zip(
        ("accept", "reject_sig", "malformed_der", "unknown_key"),
        ((got == 0).sum(), (got == 1).sum(), (got == 2).sum(), (got == 4).sum()))}
    return {"value": world * n4 / dt, "unit": "verifies/s (authenticator calls, host in / host out)",
            "n_gpus": world, "calls": world * n4, "calls_per_gpu": n4, "ms": dt * 1e3,
            "per_gpu_value": n4 / dt_rank, "scaling": "weak",
            "timing": "median of 3 passes per rank after a warm-up; ranks start at a barrier, MAX over ranks",
            "entry": "mbft_verify_batch_flat32 (compact: u8 roles, u32 offsets, 32-B e prefixes; library "
                     "page-locked flat buffers, GPU decode: k_prepare)",
            "wide_form": {"entry": "mbft_verify_batch_flat (u32 roles, u64 offsets, 47-B AuthenBytes)",
                          "per_gpu_value": n4 / dt_wide, "ms": dt_wide * 1e3, "host_buffer_bytes": wide_bytes,
                          "statuses_checked": n4},
            "pool": f"{P} distinct REQUESTs signed by {nk} clients (key window 24), tiled",
            "mix": "SURVEY 8(d) 10 %: 2% tampered op, 2% wrong signer, 2% r/s in {0, N, N (s), 2^256-1}, "
                   "1% signer without a key (the reference's stand-in for an off-curve key, rejected at "
                   "load), 1% malformed DER, 1% high s (accept), 1% tamper past byte 32 (accept)",
            "status_counts_rank0": counts, "statuses_checked": world * n4, "c_oracle_sample": 4096,
            "host_buffer_bytes": host_bytes}


def flat_pinned_level(auth, msgs, tags, tlen, B: int, reps: int, msg_len: int = 47,
                      compact: bool = False):
    """mbft_verify_batch_flat over the C2 calls in library page-locked flat
    buffers (host_array), p50 host submit -> statuses over `reps` batches
    after 3 warm-ups, with the host stage times.  compact: the Go binding's
    form, mbft_verify_batch_flat32 (u8 roles, u32 offsets) with each message
    as its 32-byte e prefix (msg_len 32: a REQUEST's AuthenBytes are 47 B, so
    e = msg[0:32])."""
    from minbft_amd.authenticator import ROLE_CLIENT, host_array
    if compact:
        msg_len = 32
    roles, ids = host_array(B, np.uint8 if compact else np.uint32), host_array(B, np.uint32)
    roles[:] = ROLE_CLIENT
    ids[:] = 0
    odt = np.uint32 if compact else np.uint64
    mo, to = host_array(B + 1, odt), host_array(B + 1, odt)
    mo[:] = np.arange(B + 1, dtype=odt) * msg_len
    to[0] = 0
    to[1:] = np.cumsum(tlen.astype(odt))
    mb = host_array(B * msg_len)
    mb[:] = np.ascontiguousarray(msgs[:, :msg_len]).reshape(-1)
    tb = host_array(int(to[B]))
    tb[:] = tags[np.arange(tags.shape[1])[None, :] < tlen[:, None]]
    out = host_array(B)
    lat = []
    auth.stage_profile()  # reset
    run = auth.verify_flat32_arrays if compact else auth.verify_flat_arrays
    for k in range(3 + reps):
        a = time.perf_counter()
        run(roles, ids, mb, mo, tb, to, out=out)
        b = time.perf_counter() - a
        if k == 2:
            auth.stage_profile()  # drop the warm-ups
        if k >= 3:
            lat.append(b)
    return lat, auth.stage_profile(), np.array(out)


def single_calls(auth, msgs, tags, tlen, n_seq: int = 200, threads: int = 16, per_thread: int = 400):
    """VerifyMessageAuthenTag one call at a time: p50
    latency of a lone call (one GPU round trip), then `threads` callers at
    once with mbft_set_coalescing on (no added wait): calls that arrive while
    a batch is on the GPU share the next one.  C2 calls, all must accept."""
    import threading

    from minbft_amd.authenticator import ROLE_CLIENT
    calls = [(bytes(msgs[i]), bytes(tags[i, :tlen[i]])) for i in range(threads * per_thread)]
    lat = []
    for k in range(n_seq + 5):
        m, t = calls[k]
        a = time.perf_counter()
        st = auth.verify_status(ROLE_CLIENT, 0, m, t)
        if k >= 5:
            lat.append(time.perf_counter() - a)
        if st != 0:
            raise SystemExit(f"single-call gate: status {st}")
    # the same lone calls through the resident verifier (mbft_set_resident)
    auth.set_resident(1)
    lat_res = []
    for k in range(n_seq + 5):
        m, t = calls[k]
        a = time.perf_counter()
        st = auth.verify_status(ROLE_CLIENT, 0, m, t)
        if k >= 5:
            lat_res.append(time.perf_counter() - a)
        if st != 0:
            raise SystemExit(f"resident single-call gate: status {st}")
    auth.set_resident(0)
    auth.set_coalescing(True, 0, 0)
    auth.stage_profile()  # reset
    bad = [0]
    barrier = threading.Barrier(threads + 1)

    def run(t):
        barrier.wait()
        for m, g in calls[t * per_thread:(t + 1) * per_thread]:
            if auth.verify_status(ROLE_CLIENT, 0, m, g) != 0:
                bad[0] += 1

    th = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
    for x in th:
        x.start()
    barrier.wait()
    a = time.perf_counter()
    for x in th:
        x.join()
    dt = time.perf_counter() - a
    auth.set_coalescing(False, 0, 0)
    st = auth.stage_profile()
    if bad[0]:
        raise SystemExit(f"coalesced-call gate: {bad[0]} calls not accepted")
    n = threads * per_thread
    out = {"entry": "mbft_verify_message_authen_tag", "p50_latency_us": float(np.median(lat)) * 1e6,
           "p50_latency_resident_us": float(np.median(lat_res)) * 1e6,
           "concurrent": {"threads": threads, "calls": n, "calls_per_s": n / dt,
                          "gpu_batches": st["batches"], "mean_calls_per_batch": n / max(st["batches"], 1),
                          "coalescing": "mbft_set_coalescing(enabled, max_wait_us=0)",
                          "driver": "Python threads (ctypes, the interpreter lock between calls)"}}
    native = native_concurrent_calls(auth, calls, threads, per_thread)
    if native:
        out["concurrent_native"] = native
    return out


def native_concurrent_calls(auth, calls, threads: int, per_thread: int,
                            configs=((16, 1), (64, 1), (64, 4)),
                            resident_configs=((1, 1), (16, 16), (64, 64))):
    """The same concurrent calls from OS threads (tools/conc_calls.cpp: one
    mbft_verify_message_authen_tag per call, no interpreter in between -- how
    a Go replica's goroutines reach the C-ABI through cgo), coalescing on, at
    (threads, slots) configs on the Go binding's 4 lanes (mbft_set_concurrency
    4): mbft_set_coalescing_slots lets up to `slots` coalesced batches run at
    once (default 1); the calls are the same threads x per_thread, split over
    the threads.  Every call must accept."""
    import ctypes

    from __graft_entry__ import build_conc_calls
    try:
        drv = ctypes.CDLL(build_conc_calls())
    except (OSError, subprocess.CalledProcessError) as e:  # bench helper only
        return {"error": str(e)}
    drv.conc_calls_run.restype = ctypes.c_double
    drv.conc_calls_run.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7
    drv.conc_calls_cpu_s.restype = ctypes.c_double
    n = threads * per_thread
    from minbft_amd.authenticator import ROLE_CLIENT
    role = np.full(n, ROLE_CLIENT, dtype=np.uint32)
    ids = np.zeros(n, dtype=np.uint32)
    mb = b"".join(m for m, _ in calls[:n])
    tb = b"".join(t for _, t in calls[:n])
    moff = np.concatenate([[0], np.cumsum([len(m) for m, _ in calls[:n]])]).astype(np.uint64)
    toff = np.concatenate([[0], np.cumsum([len(t) for _, t in calls[:n]])]).astype(np.uint64)
    mbuf = np.frombuffer(mb, dtype=np.uint8).copy()
    tbuf = np.frombuffer(tb, dtype=np.uint8).copy()
    fn = ctypes.cast(auth.lib.mbft_verify_message_authen_tag, ctypes.c_void_p).value
    res = {"calls": n, "driver": "tools/conc_calls.cpp (OS threads)"}
    prev = auth.concurrency()
    try:
        auth.set_concurrency(4)
        for nth, slots in configs:
            if n % nth:
                continue
            auth.set_coalescing_slots(slots)
            auth.set_coalescing(True, 0, 0)
            rc = np.full(n, -99, dtype=np.int32)
            best = None
            for _ in range(2):  # the first run warms the lanes' staging
                auth.stage_profile()  # reset
                dt = drv.conc_calls_run(fn, auth.ctx, nth, n // nth, role.ctypes.data,
                                        ids.ctypes.data, mbuf.ctypes.data, moff.ctypes.data,
                                        tbuf.ctypes.data, toff.ctypes.data, rc.ctypes.data)
                cpu_s = drv.conc_calls_cpu_s()
                st = auth.stage_profile()
                if (rc != 0).any():
                    raise SystemExit(f"native coalesced-call gate: {int((rc != 0).sum())} calls not accepted")
                if best is None or dt < best[0]:
                    best = (dt, st["batches"], cpu_s)
            auth.set_coalescing(False, 0, 0)
            res[f"threads_{nth}_slots_{slots}"] = {"calls_per_s": n / best[0], "gpu_batches": best[1],
                                        "mean_calls_per_batch": n / max(best[1], 1),
                                        "cpu_us_per_call": best[2] / n * 1e6}
        # the resident verifier (mbft_set_resident): a kernel kept on the GPU,
        # one mailbox slot per caller, no launch per call; coalescing stays on
        # for calls that find every slot taken
        for nth, slots in resident_configs:
            if n % nth:
                continue
            auth.set_coalescing(True, 0, 0)
            auth.set_resident(slots)
            rc = np.full(n, -99, dtype=np.int32)
            best = None
            for _ in range(2):
                dt = drv.conc_calls_run(fn, auth.ctx, nth, n // nth, role.ctypes.data,
                                        ids.ctypes.data, mbuf.ctypes.data, moff.ctypes.data,
                                        tbuf.ctypes.data, toff.ctypes.data, rc.ctypes.data)
                cpu_s = drv.conc_calls_cpu_s()
                if (rc != 0).any():
                    raise SystemExit(f"resident-call gate: {int((rc != 0).sum())} calls not accepted")
                if best is None or dt < best[0]:
                    best = (dt, cpu_s)
            best, cpu_s = best
            rs = auth.resident_stats()
            ws = auth.resident_wait_stats()
            auth.set_resident(0)
            auth.set_coalescing(False, 0, 0)
            res[f"resident_threads_{nth}_slots_{slots}"] = {
                "calls_per_s": n / best, "mean_call_us": best / (n // nth) * 1e6,
                "cpu_us_per_call": cpu_s / n * 1e6,
                "resident_calls": rs["calls"], "coalescer_fallbacks": rs["fallbacks"],
                "kernel_launches": rs["launches"], "own_hw_queue": rs["own_queue"], "wait": ws}
        # what a Go replica gets by default (gpuauth.Config.ResidentSlots = 32,
        # coalescing on): the resident verifier, one slot per caller; the
        # threads_*_slots_* lines above are the launch path (coalescer only)
        r16 = res.get("resident_threads_16_slots_16")
        if r16 is not None:
            res["threads_16_go_default"] = {
                "calls_per_s": r16["calls_per_s"], "cpu_us_per_call": r16["cpu_us_per_call"],
                "path": "resident verifier (mbft_set_resident)",
                "same_as": "resident_threads_16_slots_16"}
    finally:
        auth.set_resident(0)
        auth.set_coalescing(False, 0, 0)
        auth.set_coalescing_slots(1)
        auth.set_concurrency(prev)
    return res


def resident_interference(auth, torch, step, nsteps: int, msgs, tags, tlen, B: int, reps: int,
                          slots: int = 32, period_us: int = 200):
    """What the resident verifier costs batch work: C2's
    ms_per_step (the headline loop, 3 batches in flight) and the 1M
    authenticator-level p50 (mbft_verify_batch_flat32, the Go binding's
    form), with the Go binding's default resident kernel (32 slots) kept
    alive by a trickle of single calls -- one VerifyMessageAuthenTag every
    period_us from an OS thread (tools/conc_calls.cpp trickle_start), as a
    replica's client streams keep calling while its peer streams verify
    batches (core/message-handling.go:204-246) -- against resident off.
    Off / live alternate three times (drift on the box spreads over both);
    the minimum of each is reported, and the trickle's own call latencies."""
    import ctypes

    from __graft_entry__ import build_conc_calls
    from minbft_amd.authenticator import ROLE_CLIENT
    drv = ctypes.CDLL(build_conc_calls())
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    drv.trickle_start.restype = ctypes.c_int
    drv.trickle_start.argtypes = [vp, vp, u32, u32, vp, sz, vp, sz, ctypes.c_int]
    drv.trickle_stop.restype = ctypes.c_long
    drv.trickle_stop.argtypes = [vp, ctypes.c_long, vp]
    fn = ctypes.cast(auth.lib.mbft_verify_message_authen_tag, ctypes.c_void_p).value
    m = np.ascontiguousarray(msgs[0]).copy()
    t = np.ascontiguousarray(tags[0, :tlen[0]]).copy()

    def c2():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        a = time.perf_counter()
        for _ in range(nsteps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - a) / nsteps * 1e3

    def auth_p50():
        lat, _, st = flat_pinned_level(auth, msgs, tags, tlen, B, reps, compact=True)
        if int((np.asarray(st) == 0).sum()) != B:
            raise SystemExit("resident_interference: authenticator-level gate failed")
        return float(np.median(lat)) * 1e3

    c2ms = {"resident_off": [], "resident_live": []}
    aums = {"resident_off": [], "resident_live": []}
    tl = []
    calls = bad_total = 0
    waits = None
    try:
        for _ in range(3):
            for mode in ("resident_off", "resident_live"):
                live = mode == "resident_live"
                if live:
                    auth.set_resident(slots)
                    if drv.trickle_start(fn, auth.ctx, ROLE_CLIENT, 0, m.ctypes.data, m.nbytes, t.ctypes.data,
                                         t.nbytes, period_us) != 0:
                        raise SystemExit("resident_interference: trickle did not start")
                    time.sleep(0.005)
                c2ms[mode].append(c2())
                aums[mode].append(auth_p50())
                if live:
                    buf = np.zeros(1 << 16, dtype=np.float64)
                    bad = ctypes.c_long(0)
                    n = drv.trickle_stop(buf.ctypes.data, buf.shape[0], ctypes.byref(bad))
                    tl.append(buf[:min(n, buf.shape[0])].copy())
                    calls += n
                    bad_total += bad.value
                    rs = auth.resident_stats()
                    waits = auth.resident_wait_stats()
                    auth.set_resident(0)
                    if rs["calls"] == 0:
                        raise SystemExit("resident_interference: the trickle never reached the resident kernel")
    finally:
        drv.trickle_stop(None, 0, None)
        auth.set_resident(0)
    if bad_total:
        raise SystemExit(f"resident_interference: {bad_total} trickle calls not accepted")
    lat = np.concatenate(tl) if tl else np.zeros(1)
    c2b = {k: min(v) for k, v in c2ms.items()}
    aub = {k: min(v) for k, v in aums.items()}
    return {"slots": slots, "trickle_period_us": period_us, "c2_steps": nsteps,
            "c2_ms_per_step": c2b, "c2_ratio": c2b["resident_live"] / c2b["resident_off"],
            "c2_ms_per_step_runs": c2ms,
            "auth_level_p50_ms": aub, "auth_level_ratio": aub["resident_live"] / aub["resident_off"],
            "trickle": {"calls": int(calls), "p50_us": float(np.percentile(lat, 50)),
                        "p99_us": float(np.percentile(lat, 99)), "during": "C2 steps and 1M flat batches"},
            "resident_wait": waits}


def c3_messages(auth, nreq: int, f: int = 16, op_len: int = 64, q_window: int = 23, seed: int = 0xC3):
    """The C3 workload (c3_line): keys registered on `auth`, and the message
    structs (mbft_message, pointing into arrays kept alive by the returned
    tuple).  Returns (msgs, n, tables_s, keep)."""
    from minbft_amd import _lib
    from minbft_amd.authenticator import ROLE_CLIENT, ROLE_USIG, der_encode_rows, host_array
    n = 2 * f + 1
    R = nreq
    rng = np.random.Generator(np.random.PCG64(seed))
    dus = [int.from_bytes(hashlib.sha256(b"minbft-amd c3 usig %d" % j).digest(), "big") % (N_ORDER - 1) + 1
           for j in range(n)]
    dcl = int.from_bytes(hashlib.sha256(b"minbft-amd c3 client").digest(), "big") % (N_ORDER - 1) + 1
    auth.clear_keys()
    auth.set_key_window(q_window)
    pts = [pubkey_bytes(d) for d in dus + [dcl]]
    t = time.perf_counter()
    auth.register_points(np.frombuffer(b"".join(pts), dtype=np.uint8).reshape(-1, 64))
    for role in (ROLE_USIG, ROLE_CLIENT):
        auth.add_role(role)
    for j in range(n):
        auth.set_public_key(ROLE_USIG, j, pts[j])
    auth.set_public_key(ROLE_CLIENT, 7, pts[n])
    auth.enable_usig(True)
    tables_s = time.perf_counter() - t
    epochs = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    seq = np.arange(1, R + 1, dtype=np.uint64)
    ctr = seq.copy()                                          # counter k + 1 for request k
    ops = rng.integers(0, 256, size=(R, op_len), dtype=np.uint8)
    dt = _lib.message_dtype()

    def base(m, typ):
        a = np.zeros(m, dtype=dt)
        a["type"] = typ
        a["client_id"] = 7
        return a

    def fill_req(a, k):                                       # k: request index per row
        a["seq"] = seq[k]
        a["op"] = ops.ctypes.data + k.astype(np.uint64) * np.uint64(op_len)
        a["op_len"] = op_len

    def sign(e, keyidx, priv):
        r, s_ = auth.sign_prehashed(priv, e, keyidx)
        return der_encode_rows(r, s_)

    def certs(epoch_rows, tags, tl):
        c = np.zeros((tags.shape[0], 80), dtype=np.uint8)
        c[:, :8] = epoch_rows.astype(">u8").view(np.uint8).reshape(-1, 8)
        c[:, 8:] = tags
        return c, (tl + 8).astype(np.uint64)

    kk = np.arange(R)
    privs = np.frombuffer(b"".join(d.to_bytes(32, "big") for d in dus + [dcl]), dtype=np.uint8).reshape(-1, 32)
    # REQUEST signatures (client), PREPARE UIs (replica 0), COMMIT UIs (replicas 1..n-1)
    rq = base(R, _lib.MSG_REQUEST)
    fill_req(rq, kk)
    sigs, sl = sign(auth.authen_digests_packed(rq, 0), np.full(R, n, dtype=np.uint32), privs)
    pp = base(R, _lib.MSG_PREPARE)
    fill_req(pp, kk)
    pcert, pcl = certs(np.full(R, epochs[0], dtype=np.uint64),
                       *sign(auth.authen_digests_packed(pp, 2, np.full(R, epochs[0], dtype=np.uint64), ctr),
                             np.zeros(R, dtype=np.uint32), privs))
    cj = np.repeat(np.arange(1, n, dtype=np.uint32), R)        # replica of each COMMIT row
    ck = np.tile(kk, n - 1)                                   # its request
    cm = base((n - 1) * R, _lib.MSG_COMMIT)
    fill_req(cm, ck)
    cm["replica_id"] = cj
    cm["prep_ui_counter"] = ctr[ck]
    ccert, ccl = certs(epochs[cj], *sign(auth.authen_digests_packed(cm, 3, epochs[cj], ctr[ck]), cj, privs))
    # the stream: per request REQUEST, PREPARE, then the COMMITs in a shuffled order
    per = n + 1
    msgs = np.zeros(R * per, dtype=dt)
    sig_ptr = sigs.ctypes.data + kk.astype(np.uint64) * np.uint64(72)
    pc_ptr = pcert.ctypes.data + kk.astype(np.uint64) * np.uint64(80)
    rows = np.arange(R) * per
    msgs[rows] = rq
    msgs["stream"][rows] = 1000
    msgs["sig"][rows] = sig_ptr
    msgs["sig_len"][rows] = sl
    msgs[rows + 1] = pp
    msgs["sig"][rows + 1] = sig_ptr
    msgs["sig_len"][rows + 1] = sl
    msgs["ui_counter"][rows + 1] = ctr
    msgs["ui_cert"][rows + 1] = pc_ptr
    msgs["ui_cert_len"][rows + 1] = pcl
    order = np.argsort(rng.random((R, n - 1)), axis=1)       # COMMIT order per request
    for b in range(n - 1):
        j = order[:, b]                                       # replica index - 1, per request
        src = j * R + kk                                      # row in cm / ccert
        dst = rows + 2 + b
        msgs[dst] = cm[src]
        msgs["stream"][dst] = j + 1
        msgs["sig"][dst] = sig_ptr
        msgs["sig_len"][dst] = sl
        msgs["prep_ui_cert"][dst] = pc_ptr
        msgs["prep_ui_cert_len"][dst] = pcl
        msgs["ui_counter"][dst] = ctr
        msgs["ui_cert"][dst] = ccert.ctypes.data + src.astype(np.uint64) * np.uint64(80)
        msgs["ui_cert_len"][dst] = ccl[src]
    keep = (ops, sigs, pcert, ccert)
    return msgs, n, tables_s, keep


def c3_line(auth, torch, dev, nreq: int, f: int = 16, op_len: int = 64, q_window: int = 23,
            seed: int = 0xC3):
    """C3 (BASELINE.json configs[2]): a backup's view of nreq
    requests in a MinBFT group of n = 2f + 1 = 33 replicas -- per request the
    REQUEST (client 7), the primary's PREPARE and the COMMITs of the 32
    backups (streams 0..32, mixed signers per request), sequential USIG
    counters per replica from 1 and a random epoch per replica -- validated
    by mbft_validate_messages (the core's validators with stream semantics,
    identical calls verified once: 34 distinct verifies per request, all
    AuthenBytes and digests on the GPU in the same round trip).  33 USIG keys
    + 1 client key at window q_window beside the W = 29 generator table.
    Inputs are signed on the GPU through the library's own digest stage
    (mbft_authen_digests) and signer.  Returns messages/s and verifies/s
    (median of 3 calls, host buffers in, results out)."""
    from minbft_amd.authenticator import host_array
    msgs, n, tables_s, keep = c3_messages(auth, nreq, f, op_len, q_window, seed)
    R = nreq
    per = n + 1
    out = np.zeros(msgs.shape[0], dtype=np.int32)
    ts = []
    for k in range(4):
        # passes after the first find every replica's epoch already captured
        # (the same epochs): identical results, same work
        a = time.perf_counter()
        auth.validate_messages_packed(msgs, n, 0, out)
        if k:
            ts.append(time.perf_counter() - a)
    bad = int((out != 0).sum())
    if bad:
        raise SystemExit(f"C3 gate: {bad} of {out.size} messages rejected")
    dt_ = float(np.median(ts))
    # The device message layer: the same messages as a flat batch (records +
    # one byte arena, every message with its own copy of its bytes, as a Go
    # replica would marshal what it received) in library page-locked memory,
    # validated by mbft_validate_messages_flat on the GPU end to end; the host
    # only replays the outcomes in order.  Packing is the caller's marshal
    # (timed apart: mbft_pack_messages from the structs).
    a = time.perf_counter()
    recs, arena = auth.pack_messages(msgs, pinned=True)
    pack_s = time.perf_counter() - a
    out_f = host_array(msgs.shape[0], np.int32)
    tf = []
    for k in range(6):
        a = time.perf_counter()
        auth.validate_messages_flat(recs, arena, n, 0, out_f)
        if k:
            tf.append(time.perf_counter() - a)
    if int((out_f != 0).sum()) or not np.array_equal(np.asarray(out_f), out):
        raise SystemExit("C3 gate: the device message layer disagrees with the host layer")
    df = float(np.median(tf))
    # one more pass with HIP events on the copy stream (mbft_profile_msg_layer):
    # the upload time of records + arena, and the device span, per call
    auth.profile(True)
    auth.msg_layer_profile()  # reset
    auth.validate_messages_flat(recs, arena, n, 0, out_f)
    mprof = auth.msg_layer_profile()
    auth.profile_read()
    auth.profile(False)
    # the Go drop-in's own sequence over the same stream (go/core/
    # message-handling-batch.go + go/gpuauth/messages.go)
    go = go_wiring_line(auth, msgs, n, out)
    go["coalesced"] = {f"lanes_{ln}": go_wiring_line(auth, msgs, n, out, lanes=ln, coalesce=True)
                       for ln in (1, 2, 4)}
    del keep  # (the message structs point into these arrays)
    return {"messages": int(msgs.shape[0]), "requests": R, "n_replicas": n, "verifies": R * per,
            "messages_per_s": msgs.shape[0] / df, "verifies_per_s": R * per / df, "ms": df * 1e3,
            "key_window": q_window, "op_bytes": op_len, "tables_s": tables_s,
            "entry": "mbft_validate_messages_flat over library page-locked records + byte arena "
                     "(the message layer on the GPU, in-order replay on the host)",
            "flat_batch_bytes": int(recs.nbytes + arena.nbytes),
            "hip_events": {"h2d_ms": mprof["h2d_ms"], "device_ms": mprof["device_ms"],
                           "h2d_GBps": mprof["bytes"] / max(mprof["h2d_ms"], 1e-9) / 1e6,
                           "basis": "mbft_profile_msg_layer: HIP events on the library's copy stream around "
                                    "the records' and arena's uploads, and from the first upload to the end "
                                    "of the last kernel / download (one profiled pass)"},
            "msg_kernels": msg_kernel_roofline(),
            "go_wiring": go,
            "pack_ms": pack_s * 1e3,
            "pack_entry": "mbft_pack_messages (mbft_message structs -> records + arena, one host thread)",
            "host_layer": {"entry": "mbft_validate_messages (host-built calls, one GPU round trip)",
                           "messages_per_s": msgs.shape[0] / dt_, "ms": dt_ * 1e3}}


def msg_kernel_roofline():
    """The message-layer kernels' algorithmic bytes/s against the 8 TB/s
    HBM roofline, from the newest committed C3 kernel-trace analysis
    (tools/msg_kernel_roofline.py over a rocprofv3 trace of tools/c3_probe.py:
    per-kernel durations need the trace; HIP events here would time the
    chunk pipeline, not a kernel)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_msg_kernels_roofline_*.json")))
    if not files:
        return None
    with open(files[-1]) as f:
        d = json.load(f)
    return {"basis": "profiles/" + os.path.basename(files[-1]), "peak_GBps": d["peak_GBps"],
            "kernels": {k: {"GBps": round(v["GBps"], 1), "frac_of_hbm": round(v["frac_of_hbm"], 4),
                            "ms_per_pass": round(v["ms_per_pass"], 4)} for k, v in d["kernels"].items()},
            "note": d["note"]}


def go_wiring_line(auth, msgs: np.ndarray, n: int, want: np.ndarray, batch: int = 4096, threads: int = 8,
                   lanes: int = 4, coalesce: bool = False):
    """The C-ABI sequence of the Go drop-in's batched core loop over a C3
    stream (go/core/message-handling-batch.go, go/gpuauth/messages.go): each
    peer / client stream separately, in batches of at most maxBatch = 4,096
    messages in stream order, each batch's records + arena in library
    page-locked memory (gpuauth's arena), mbft_check_messages_flat, then
    every message resolved in order (mbft_resolve_message; timed here as
    mbft_resolve_messages over the batch -- the same work without one Python
    ctypes call per message, which would cost more than the resolve itself;
    Go's cgo call per message, ~0.1-0.2 us, is not included).  Streams run on
    `threads` worker threads at once (the Go loops are goroutines) over
    `lanes` concurrency lanes (gpuauth's Config.Concurrency default 4).  The
    Go-side marshal (raw field copies, no hashing) is done beforehand and not
    timed.  Median of 3 timed passes after a warm-up; every result checked.
    coalesce: mbft_set_check_coalescing on (what go/gpuauth enables), with
    threads = one per stream (the core's goroutine per connection): the
    streams' concurrent checks merge into device passes."""
    import queue
    import threading
    sids = np.unique(msgs["stream"])
    chunks, wants = [], []
    for sid in sids:
        idx = np.nonzero(msgs["stream"] == sid)[0]
        lst = []
        for k in range(0, idx.size, batch):
            sub = np.ascontiguousarray(msgs[idx[k:k + batch]])
            recs, arena = auth.pack_messages(sub, pinned=True)
            recs["stream"] = 0
            lst.append((recs, arena, sub.shape[0]))
        chunks.append(lst)
        wants.append(want[idx])
    if coalesce:
        threads = len(chunks)
    prev = auth.concurrency()
    auth.set_concurrency(lanes)
    auth.set_check_coalescing(coalesce)
    auth.check_coalescing_stats()
    bad = [0]
    tres = [0.0]

    def run_stream(j):
        outs = []
        for recs, arena, m in chunks[j]:
            b = auth.check_messages_flat(recs, arena, n)
            a = time.perf_counter()
            outs.append(b.resolve_range(0, m))
            tres[0] += time.perf_counter() - a
            b.close()
        if not np.array_equal(np.concatenate(outs), wants[j]):
            bad[0] += 1

    def one_pass():
        q = queue.Queue()
        for j in range(len(chunks)):
            q.put(j)

        def worker():
            while True:
                try:
                    j = q.get_nowait()
                except queue.Empty:
                    return
                run_stream(j)
        th = [threading.Thread(target=worker) for _ in range(threads)]
        a = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        return time.perf_counter() - a

    try:
        one_pass()
        tres[0] = 0.0
        auth.check_coalescing_stats()
        ts = [one_pass() for _ in range(3)]
        cst = auth.check_coalescing_stats()
    finally:
        auth.set_concurrency(prev)
        auth.set_check_coalescing(False)
    if bad[0]:
        raise SystemExit(f"go_wiring gate: {bad[0]} streams differ from the one-call validation")
    dt = float(np.median(ts))
    nb = sum(len(c) for c in chunks)
    extra = {}
    if coalesce:
        extra = {"coalescing": "mbft_set_check_coalescing(enabled, max_wait_us=0)",
                 "device_passes_per_run": cst["passes"] / 3,
                 "mean_messages_per_pass": cst["messages"] / max(cst["passes"], 1)}
    return {**extra, "messages_per_s": msgs.shape[0] / dt, "ms": dt * 1e3, "messages": int(msgs.shape[0]),
            "streams": int(len(sids)), "check_calls": int(nb), "max_batch": batch,
            "threads": threads, "lanes": lanes,
            "resolve_ns_per_message": tres[0] / 3 / msgs.shape[0] * 1e9,
            "sequence": "per stream batch of <= 4096 messages: mbft_check_messages_flat (library page-locked "
                        "records + arena), then mbft_resolve_message per message in order (timed as "
                        "mbft_resolve_messages); Go marshal and per-message cgo calls not included",
            "gate": "every result equal to the one-call validation (all valid)"}


def _window_batches(auth, msgs: np.ndarray, windows):
    """Each window (row indices into the mbft_message array msgs) packed as
    its own flat batch -- records + arena, the records' offsets relative to
    the window's arena -- all in ONE library page-locked allocation each (the
    Go binding marshals what it received into mbft_host_alloc arenas).
    Returns (recs uint8 view, rec_off, arena, byte_off, keep)."""
    from minbft_amd.authenticator import host_array
    parts = [auth.pack_messages(np.ascontiguousarray(msgs[np.asarray(w)]), pinned=False) for w in windows]
    rec_off = np.zeros(len(parts) + 1, dtype=np.uint64)
    byte_off = np.zeros(len(parts) + 1, dtype=np.uint64)
    for k, (r, b) in enumerate(parts):
        rec_off[k + 1] = rec_off[k] + r.shape[0]
        byte_off[k + 1] = byte_off[k] + ((b.nbytes + 7) & ~7)
    recs = host_array(int(rec_off[-1]), parts[0][0].dtype)
    arena = host_array(max(int(byte_off[-1]), 1))
    for k, (r, b) in enumerate(parts):
        recs[int(rec_off[k]):int(rec_off[k + 1])] = r
        arena[int(byte_off[k]):int(byte_off[k]) + b.nbytes] = b
    return recs, rec_off, arena, byte_off


def _run_windows(auth, drv, n_replicas: int, batch, threads_first=None):
    """msg_latency_run over packed windows: per-window latency (us) and the
    per-message results; threads_first: [first window of thread t] + [end]."""
    import ctypes
    recs, rec_off, arena, byte_off = batch
    K = rec_off.shape[0] - 1
    first = np.asarray(threads_first if threads_first is not None else [0, K], dtype=np.int32)
    res = np.full(int(rec_off[-1]), -99, dtype=np.int32)
    lat = np.zeros(K, dtype=np.float64)
    fn = lambda name: ctypes.cast(getattr(auth.lib, name), ctypes.c_void_p).value  # noqa: E731
    dt = drv.msg_latency_run(fn("mbft_check_messages_flat"), fn("mbft_resolve_message"),
                             fn("mbft_msg_batch_free"), auth.ctx, n_replicas, first.shape[0] - 1,
                             first.ctypes.data, recs.ctypes.data, rec_off.ctypes.data, arena.ctypes.data,
                             byte_off.ctypes.data, res.ctypes.data, lat.ctypes.data)
    if dt < 0:
        w = int(-1 - dt)
        raise SystemExit(f"latency driver: check of window {w} failed ({int(res[int(rec_off[w])])}): "
                         f"{auth.last_error()}")
    return lat, res, dt


def _pct(lat):
    return {"p50_us": float(np.percentile(lat, 50)), "p90_us": float(np.percentile(lat, 90)),
            "p99_us": float(np.percentile(lat, 99)), "samples": int(len(lat))}


SMALL_CHECK_DEFAULT = 512  # mbft_set_small_check's default (msgdev.cpp / host_internal.h)


def go_wiring_latency(auth, nreq: int = 128, f: int = 1, q_window: int = 26, op_len: int = 256,
                      seed: int = 0xC5, sizes=(2, 8, 16, 64, 256, 512), small_max: int = SMALL_CHECK_DEFAULT,
                      configs=(("go_default", 4, True, 32), ("go_default_launch", 4, True, 0),
                               ("plain", 1, False, 0)), c5: bool = True, routes=None):
    """The Go core loop's low-load regime: a client's
    REQUEST stream is strictly sequential (the handler blocks on the reply,
    core/message-handling.go:399), and peer streams at low load deliver one
    message at a time, so every check is a batch of one.  Workload: the
    C3 messages of an n = 2f + 1 = 3 replica group (c3_messages: REQUEST with a
    256-byte op, the primary's PREPARE, the backups' COMMITs; USIG keys and the
    client key at W = q_window beside the W = 29 generator table), each window
    packed as its own flat batch in library page-locked memory.  Timed from
    an OS thread (tools/msg_latency.cpp): mbft_check_messages_flat, then
    mbft_resolve_message per message, then mbft_msg_batch_free -- exactly the
    sequence go/gpuauth/messages.go makes per batch (the Go-side marshal and
    the cgo call overhead, ~0.1-0.2 us a call, not included).  Every result
    checked (all valid).  Windows of 1 message per kind (a lone REQUEST,
    PREPARE, COMMIT), then 2, 8, 16, 64, 256 and 512 consecutive messages of the stream; in
    the Go binding's default configuration (4 lanes, check coalescing on, the
    resident verifier with 32 slots: a small check's calls go to the kernel
    kept on the GPU, no launch), the same with a launch per check, and plain
    (1 lane, no coalescing), with the small route (the default for <= 512
    messages) and with the device message layer forced (small route off)."""
    import ctypes

    from __graft_entry__ import build_msg_latency
    drv = ctypes.CDLL(build_msg_latency())
    drv.msg_latency_run.restype = ctypes.c_double
    drv.msg_latency_run.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_int] + \
        [ctypes.c_void_p] * 7
    drv.msg_latency_cpu_s.restype = ctypes.c_double
    msgs, n, tables_s, keep = c3_messages(auth, nreq, f, op_len, q_window, seed)
    per = n + 1
    rows = np.arange(nreq) * per
    M = msgs.shape[0]
    out = {"workload": f"C3 stream of an n = {n} group (f = {f}): {nreq} requests x (REQUEST, PREPARE, "
                       f"{n - 1} COMMITs) = {M} messages, {op_len}-byte ops, USIG + client keys at W = "
                       f"{q_window}, generator W = 29",
           "sequence": "per window: mbft_check_messages_flat (library page-locked records + arena), "
                       "mbft_resolve_message per message, mbft_msg_batch_free; one OS thread "
                       "(tools/msg_latency.cpp), windows one after another",
           "tables_s": tables_s}
    prev = auth.concurrency()
    whole = _window_batches(auth, msgs, [list(range(k, min(k + 64, M))) for k in range(0, M, 64)])
    kinds = {"REQUEST": rows, "PREPARE": rows + 1, "COMMIT": rows + 2}
    singles = {k: _window_batches(auth, msgs, [[int(i)] for i in idx]) for k, idx in kinds.items()}
    sized = {w: _window_batches(auth, msgs, [list(range(k, k + w)) for k in range(0, M - w + 1, w)])
             for w in sizes}
    out["small_check_max"] = small_max
    try:
        for cfg, lanes, co, resident in configs:
            auth.set_concurrency(lanes)
            auth.set_check_coalescing(co)
            auth.set_resident(resident)
            res_cfg = {"lanes": lanes, "check_coalescing": co, "resident_slots": resident}
            for route, small in routes or (("small_route", small_max), ("device_layer", 0)):
                auth.set_small_check(small)
                # the whole stream once in order (captures every replica's
                # epoch, warms the lanes' staging and the kernels)
                _, r, _ = _run_windows(auth, drv, n, whole)
                if (r != 0).any():
                    raise SystemExit(f"go_wiring_latency gate: {int((r != 0).sum())} messages rejected")
                d = {}
                for kind, b in singles.items():
                    lat, r, _ = _run_windows(auth, drv, n, b)
                    if (r != 0).any():
                        raise SystemExit(f"go_wiring_latency gate ({kind}): rejects")
                    d[f"1_{kind}"] = _pct(lat)
                    # process CPU (every thread) per window: the CPU bill
                    # beside the latency
                    d[f"1_{kind}"]["cpu_us_per_window"] = drv.msg_latency_cpu_s() / len(lat) * 1e6
                for w, b in sized.items():
                    # untimed passes first (at least 8 windows: every lane's
                    # staging grown to this window size -- a lane's first
                    # window of a new size allocates), then passes until at
                    # least 32 timed windows (the 512-message stream holds
                    # only 2 windows of 256)
                    nwin = b[1].shape[0] - 1  # (recs, rec_off, arena, byte_off)
                    for _ in range(max(1, -(-8 // nwin))):
                        _run_windows(auth, drv, n, b)
                    lats = []
                    cpu = 0.0
                    for _ in range(max(1, -(-32 // nwin))):
                        lat, r, _ = _run_windows(auth, drv, n, b)
                        cpu += drv.msg_latency_cpu_s()
                        if (r != 0).any():
                            raise SystemExit(f"go_wiring_latency gate (window {w}): rejects")
                        lats.append(lat)
                    lat = np.concatenate(lats)
                    d[f"{w}_messages"] = _pct(lat)
                    d[f"{w}_messages"]["cpu_us_per_window"] = cpu / len(lat) * 1e6
                res_cfg[route] = d
            out[cfg] = res_cfg
        if c5:
            out["c5_proxy"] = c5_proxy(auth, drv, msgs, n, nreq)
    finally:
        auth.set_resident(0)
        auth.set_small_check(SMALL_CHECK_DEFAULT)
        auth.set_check_coalescing(False)
        auth.set_concurrency(prev)
    del keep
    return out


def c5_proxy(auth, drv, msgs: np.ndarray, n: int, nreq: int):
    """NOT C5 (no consensus runs): the verification part of a 3-replica
    MinBFT commit (core/integration_test.go:146-226 runs the
    real thing) as the C-ABI sequence the three replicas' Go core loops make,
    one message at a time, in causal order -- per request: the REQUEST checked
    at the primary and at both backups (the client sends it to all), the
    PREPARE at both backups, backup 1's COMMIT at the primary and backup 2,
    backup 2's COMMIT at the primary and backup 1.  One context stands in for
    the three replicas' authenticators (the tables are shared; every message
    is valid, so the merged USIG epoch state changes no result).  Go binding
    defaults: 4 lanes, check coalescing on, small route, the resident
    verifier (32 slots).  Reported per
    committed request: the primary's commit path (REQUEST at the primary ->
    PREPARE at a backup -> a COMMIT at the primary: 1 + 2 + 3 = 6 signature
    checks in sequence) and every check's latency."""
    per = n + 1
    order, role = [], []
    for k in range(nreq):
        r = k * per
        # the COMMITs of the stream are shuffled per request: find each backup's
        cm = {int(msgs["replica_id"][r + 2 + b]): r + 2 + b for b in range(n - 1)}
        seq = [(r, "REQUEST@primary"), (r, "REQUEST@backup"), (r, "REQUEST@backup"),
               (r + 1, "PREPARE@backup"), (r + 1, "PREPARE@backup"),
               (cm[1], "COMMIT@primary"), (cm[1], "COMMIT@backup"),
               (cm[2], "COMMIT@primary"), (cm[2], "COMMIT@backup")]
        for i, rl in seq:
            order.append([i])
            role.append(rl)
    auth.set_concurrency(4)
    auth.set_check_coalescing(True)
    auth.set_small_check(SMALL_CHECK_DEFAULT)
    auth.set_resident(32)
    b = _window_batches(auth, msgs, order)
    _run_windows(auth, drv, n, b)  # warm
    lat, r, dt = _run_windows(auth, drv, n, b)
    if (r != 0).any():
        raise SystemExit("c5_proxy gate: rejects")
    role = np.array(role)
    L = lat.reshape(nreq, 9)
    commit_path = L[:, 0] + L[:, 3] + L[:, 5]
    return {"label": "not C5: the verification critical path of a 3-replica commit through the C-ABI, "
                     "one message at a time (no consensus, one context for three replicas)",
            "per_check": {rl: _pct(lat[role == rl]) for rl in ("REQUEST@primary", "REQUEST@backup",
                                                              "PREPARE@backup", "COMMIT@primary",
                                                              "COMMIT@backup")},
            "primary_commit_path_us": _pct(commit_path),
            "checks_per_request": 9, "signature_checks_on_commit_path": 6,
            "requests": nreq, "wall_ms": dt * 1e3}


def key_series(n: int, seed: bytes):
    """n distinct signer keys d_i = d_0 + i and their public keys Q_i = Q_0 +
    i G (one affine addition each; synthetic load, outside timed regions)."""
    d0 = int.from_bytes(hashlib.sha256(seed).digest(), "big") % (N_ORDER - n - 1) + 1
    q = pt_mul(d0, G_POINT)
    ds, xy = [], []
    for i in range(n):
        ds.append(d0 + i)
        xy.append(q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big"))
        q = pt_add(q, G_POINT)
    return ds, np.frombuffer(b"".join(xy), dtype=np.uint8).reshape(n, 64)


def c2_config_line(auth, torch, dev, streams, B: int, d_e, g_window: int, q_window: int, nkeys: int,
                   steps: int, warmup: int, label: str):
    """C2 throughput (inputs in HBM, same step loop as the headline) at other
    comb windows and signer populations: nkeys client keys at q_window beside
    a g_window generator table, item i signed by key i mod nkeys."""
    from minbft_amd.authenticator import ROLE_CLIENT
    t = time.perf_counter()
    auth.clear_keys()
    auth.set_generator_window(g_window)
    auth.set_key_window(q_window)
    ds, xy = key_series(nkeys, b"minbft-amd bench clients " + label.encode())
    slots, valid = auth.register_points(xy)
    assert valid.all()
    auth.add_role(ROLE_CLIENT)
    auth.set_public_key(ROLE_CLIENT, 0, xy[0].tobytes())
    tables_s = time.perf_counter() - t
    kidx = (np.arange(B) % nkeys).astype(np.int32)
    d_priv = torch.from_numpy(np.frombuffer(b"".join(k.to_bytes(32, "big") for k in ds),
                                            dtype=np.uint8).copy()).to(dev)
    d_kidx = torch.from_numpy(kidx).to(dev)
    r = torch.empty((B, 32), dtype=torch.uint8, device=dev)
    s_ = torch.empty((B, 32), dtype=torch.uint8, device=dev)
    auth.sign_prehashed_device(d_priv.data_ptr(), d_kidx.data_ptr(), d_e.data_ptr(), B, r.data_ptr(),
                               s_.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d_slot = torch.from_numpy(slots.astype(np.int32)[kidx]).to(dev)
    sts = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in streams]
    k = [0]

    def step():
        j = k[0] % len(streams)
        k[0] += 1
        auth.verify_prehashed_device(d_e.data_ptr(), r.data_ptr(), s_.data_ptr(), d_slot.data_ptr(), B,
                                     sts[j].data_ptr(), streams[j].cuda_stream)

    for _ in streams:
        step()
    torch.cuda.synchronize()
    acc = min(int((x == 0).sum().item()) for x in sts)
    if acc != B:
        raise SystemExit(f"{label} gate: {acc}/{B} accepted")
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - a
    return {"value": B * steps / dt, "unit": "verifies/s", "ms_per_step": dt / steps * 1e3,
            "comb_windows": {"G": g_window, "Q": q_window}, "signer_keys": nkeys, "items": B,
            "steps": steps, "tables_s": tables_s, "gate": "all accepted",
            "adds_per_verify": mixed_adds(g_window, q_window) + 1}


def binding_lines(auth, torch, dev, streams, B: int, d_e, steps: int, warmup: int):
    """C2 at the configurations the Go binding ships:
    round 2's fixed defaults (generator 26, clients 16), 1,024 distinct
    clients at W = 16, and what mbft_plan_windows (the binding's default now)
    picks for 1 and for 1,024 client keys on this device's free HBM."""
    from minbft_amd.authenticator import plan_windows
    out = {"round2_defaults_1_client": c2_config_line(auth, torch, dev, streams, B, d_e, 26, 16, 1,
                                                     steps, warmup, "r2d1"),
           "round2_defaults_1024_clients": c2_config_line(auth, torch, dev, streams, B, d_e, 26, 16, 1024,
                                                         steps, warmup, "r2d1024")}
    auth.clear_keys()
    auth.set_generator_window(16)  # release the generator table: plan on the free HBM
    torch.cuda.empty_cache()
    p1 = plan_windows(dev.index or 0, 0, 0, 1)
    p1024 = plan_windows(dev.index or 0, 0, 0, 1024)
    out["planned_1_client"] = {"plan": p1, "note": "the headline line runs at this plan"
                               if (p1["generator"], p1["client"]) == (29, 29) else "differs from the headline"}
    out["planned_1024_clients"] = c2_config_line(auth, torch, dev, streams, B, d_e, p1024["generator"],
                                                 p1024["client"], 1024, steps, warmup, "plan1024")
    out["planned_1024_clients"]["plan"] = p1024
    return out


def concurrency_line(auth, msgs, tags, tlen, threads: int = 8, batches: int = 24, n: int = 4096):
    """Concurrent Prefetch-sized batches (the Go core's peer stream loops,
    api/api.go:132): `threads` callers each verify `batches` flat batches of
    n C2 calls in library page-locked memory, with mbft_set_concurrency 1
    (every call serialized on the context, round 2) and 4 (lanes: the
    batches' copies and kernels overlap).  All must accept."""
    import threading

    from minbft_amd.authenticator import ROLE_CLIENT, host_array
    out = {}
    arrays = []
    for t in range(threads):
        lo = (t * n) % max(msgs.shape[0] - n, 1)
        roles, ids = host_array(n, np.uint32), host_array(n, np.uint32)
        roles[:] = ROLE_CLIENT
        ids[:] = 0
        mo, to = host_array(n + 1, np.uint64), host_array(n + 1, np.uint64)
        mo[:] = np.arange(n + 1, dtype=np.uint64) * 47
        tl = tlen[lo:lo + n]
        to[0] = 0
        to[1:] = np.cumsum(tl.astype(np.uint64))
        mb = host_array(n * 47)
        mb[:] = np.ascontiguousarray(msgs[lo:lo + n, :47]).reshape(-1)
        tb = host_array(int(to[n]))
        tg = tags[lo:lo + n]
        tb[:] = tg[np.arange(tg.shape[1])[None, :] < tl[:, None]]
        arrays.append((roles, ids, mb, mo, tb, to, host_array(n)))
    for lanes in (1, 4):
        auth.set_concurrency(lanes)
        bad = [0]
        barrier = threading.Barrier(threads + 1)

        def run(t):
            a = arrays[t]
            barrier.wait()
            for _ in range(batches):
                auth.verify_flat_arrays(*a[:6], out=a[6])
                bad[0] += int((np.asarray(a[6]) != 0).sum())

        for a in arrays:  # warm every lane's buffers
            auth.verify_flat_arrays(*a[:6], out=a[6])
        th = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
        for x in th:
            x.start()
        barrier.wait()
        t0 = time.perf_counter()
        for x in th:
            x.join()
        dt = time.perf_counter() - t0
        if bad[0]:
            raise SystemExit(f"concurrency gate: {bad[0]} calls not accepted")
        out[f"lanes_{lanes}"] = {"calls_per_s": threads * batches * n / dt, "wall_ms": dt * 1e3}
    auth.set_concurrency(1)
    out.update({"threads": threads, "batches_per_thread": batches, "calls_per_batch": n,
                "entry": "mbft_verify_batch_flat (page-locked arenas, GPU decode), one arena per thread",
                "speedup": out["lanes_4"]["calls_per_s"] / out["lanes_1"]["calls_per_s"]})
    return out


def multi_engine_line(world: int, B: int, msgs, tags, tlen, qxy: bytes, g_window: int, q_window: int,
                      reps: int):
    """The in-process multi-GPU model a Go replica uses (mbft_ctx_add_device):
    ONE context over all `world` devices, tables replicated on each, and
    world x B C2 calls per mbft_verify_batch_flat (library page-locked
    buffers, GPU decode) split into contiguous shards, one host thread and
    stream per device, statuses back in index order.  p50 host submit ->
    statuses over `reps` batches after 2 warm-ups.  Runs on rank 0 after
    every rank has released its own tables."""
    from minbft_amd.authenticator import ROLE_CLIENT, Authenticator, host_array
    t = time.perf_counter()
    a = Authenticator(0, devices=range(1, world))
    try:
        a.set_generator_window(g_window)
        a.set_key_window(q_window)
        a.add_role(ROLE_CLIENT)
        a.set_public_key(ROLE_CLIENT, 0, qxy)
        tables_s = time.perf_counter() - t
        n = world * B
        roles, ids = host_array(n, np.uint32), host_array(n, np.uint32)
        roles[:] = ROLE_CLIENT
        ids[:] = 0
        mo, to = host_array(n + 1, np.uint64), host_array(n + 1, np.uint64)
        mo[:] = np.arange(n + 1, dtype=np.uint64) * 47
        tl = np.tile(tlen, world)
        to[0] = 0
        to[1:] = np.cumsum(tl.astype(np.uint64))
        mb = host_array(n * 47)
        mb[:] = np.tile(np.ascontiguousarray(msgs[:, :47]).reshape(-1), world)
        tb = host_array(int(to[n]))
        one = tags[np.arange(tags.shape[1])[None, :] < tlen[:, None]]
        tb[:] = np.tile(one, world)
        out = host_array(n)
        lat = []
        for k in range(2 + reps):
            t0 = time.perf_counter()
            a.verify_flat_arrays(roles, ids, mb, mo, tb, to, out=out)
            if k >= 2:
                lat.append(time.perf_counter() - t0)
        acc = int((np.asarray(out) == 0).sum())
        if acc != n:
            raise SystemExit(f"multi-engine gate: {acc}/{n} accepted")
        p50 = float(np.median(lat))
        return {"value": n / p50, "unit": "verifies/s (p50 batch, host in / host out)", "devices": world,
                "items": n, "p50_ms": p50 * 1e3, "tables_s": tables_s,
                "comb_windows": {"G": g_window, "Q": q_window},
                "entry": "one mbft_ctx over all devices (mbft_ctx_add_device), mbft_verify_batch_flat",
                "gate": "all accepted"}
    finally:
        a.close()



def measure_peak_mad_rate(run: bool = True):
    """v_mad_u64_u32 issue rate (lane-ops/s) from tools/ubench_valu, else the
    committed measurement profiles/round1_ubench_valu.json.  Must run before
    this process touches the GPU (the child is a separate program)."""
    exe = os.path.join(ROOT, "tools", "ubench_valu")
    try:
        if run and os.path.exists(exe):
            p = subprocess.run([exe, "0", "mad"], capture_output=True, text=True, timeout=60)
            for line in p.stdout.splitlines():
                d = json.loads(line)
                if d.get("op") == "v_mad_u64_u32":
                    return d["lane_ops_per_s"], "measured live (tools/ubench_valu)"
    except Exception:
        pass
    with open(os.path.join(ROOT, "profiles", "round1_ubench_valu.json")) as f:
        for line in f:
            d = json.loads(line)
            if d.get("op") == "v_mad_u64_u32":
                return d["lane_ops_per_s"], "profiles/round1_ubench_valu.json"
    return 256 * 64 * 2.4e9 / 4, "spec fallback"


def read_traffic(g_window: int, q_window: int):
    """HBM bytes per k_verify launch for these comb windows from the committed
    PMC passes (tools/pmc_round.sh -> tools/pmc_summarize.py: FETCH_SIZE x2
    per the gfx950 correction + WRITE_SIZE), newest round first, or None if
    that window pair was not profiled.  The x2 holds for this access pattern
    too: every random 64-B comb-entry gather is one 128-B fabric request
    (TCC_EA0_RDREQ_128B, tools/pmc_rdreq.sh, profiles/round2_pmc_rdreq.json)."""
    for name in ("round6_pmc_w29_29.json", "round4_pmc_w29_29.json", "round3_pmc_w29_29.json", "round2_pmc_w29_29.json",
                 "round1_pmc_windows.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                return json.load(f)[f"w{g_window}_{q_window}"]["hbm_bytes_per_launch"], "profiles/" + name
        except Exception:
            continue
    return None, None


def effective_cpus():
    """CPUs this process can actually use: its affinity set, capped by the
    cgroup CPU quota (cgroup v2 cpu.max, else v1 cfs_quota_us / period).  On
    the GPU box os.cpu_count() shows the whole machine (256) while the job
    gets a 16-CPU share."""
    try:
        aff = len(os.sched_getaffinity(0))
    except Exception:
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = int(q) / int(per)
    except Exception:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    eff = aff if quota is None else max(1, min(aff, int(-(-quota // 1))))
    return {"effective": eff, "affinity": aff, "cgroup_quota_cpus": quota}


def cpu_info():
    """nproc (CPUs this process may run on), os.cpu_count() and the lscpu
    model name of this host."""
    model = None
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                model = line.split(":", 1)[1].strip()
    except Exception:
        pass
    try:
        nproc = len(os.sched_getaffinity(0))
    except Exception:
        nproc = os.cpu_count()
    return {"nproc": nproc, "os_cpu_count": os.cpu_count(), "lscpu_model": model,
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}


def cpu_baseline(msgs: np.ndarray, tags: np.ndarray, tlen: np.ndarray, qxy: bytes,
                 ossl_sample: int, port_sample: int):
    """All-core CPU baselines of the same per-call work as
    VerifyMessageAuthenTag(ClientAuthen, ...) (crypto.go:79-89,120-126: DER
    decode, digest = msg || SHA256(""), ecdsa.Verify), on bounded prefixes
    of the C2 workload, one thread per CPU (os.cpu_count()).  NOT Go: no Go
    toolchain exists on this image or the GPU box.
      openssl: OpenSSL 3 d2i_ECDSA_SIG + ECDSA_do_verify
               (oracle/c/openssl_baseline.c) -- the stronger line, `value`;
      port:    the oracle's C restatement (oracle/c/p256_oracle.c)."""
    from oracle import c_oracle
    c_oracle.build()
    cpus = effective_cpus()
    threads = cpus["effective"]
    qarr = np.frombuffer(qxy, dtype=np.uint8)
    lines = []
    for kind, n, fn in (("openssl", ossl_sample, c_oracle.ossl_verify_ecdsa_role_batch),
                        ("port", port_sample, c_oracle.verify_ecdsa_role_batch)):
        n = min(n, msgs.shape[0])
        ms = [msgs[i].tobytes() for i in range(n)]
        ts = [tags[i, :tlen[i]].tobytes() for i in range(n)]
        slot = np.zeros(n, dtype=np.uint32)
        t = time.perf_counter()
        st = fn(qarr, slot, ms, ts, nthreads=threads)
        dt = time.perf_counter() - t
        ok = int((st == 0).sum())
        if ok != n:
            raise SystemExit(f"cpu baseline ({kind}) accepted {ok}/{n}")
        lines.append({"impl": kind, "value": n / dt, "unit": "verifies/s", "threads": threads,
                      "per_cpu": n / dt / threads, "items": n, "wall_s": dt})
    best = max(lines, key=lambda ln: ln["value"])
    info = cpu_info()
    # kind: the implementation that won -- "port" is this repo's C
    # restatement of the reference's path (oracle/c/p256_oracle.c),
    # "openssl" an independent P-256 (OpenSSL 3); neither is the reference's
    # Go, which cannot run here (no Go toolchain)
    # kind "port": both implementations restate the reference's per-call
    # steps (crypto.go:79-89,120-126) -- the openssl line with OpenSSL 3's
    # P-256 for the arithmetic -- and neither is the reference itself
    return {"value": best["value"], "unit": "verifies/s", "cores": threads, "kind": "port",
            "impl": best["impl"], "per_cpu": best["value"] / threads,
            "cpu_us_per_verify": threads / best["value"] * 1e6,
            "label": f"not Go (no Go toolchain on the box): {best['impl']} on the {threads} CPUs this "
                     "process can use (affinity capped by the cgroup quota)",
            "sample": f"first {best['items']} C2 REQUEST authenticator calls: DER decode + Sum(m) digest "
                      f"+ P-256 verify, {threads} threads, {best['wall_s']:.2f} s wall, all accepted",
            "cpus": cpus, "lines": lines, **info}


# The driver parses the final stdout line from a bounded tail of the output:
# the line must stay well under this size (round 5's 23 KB line was not
# parsed).  Everything else goes to the detail file the line names.
LINE_LIMIT = 8000


def _get(d, *path):
    """d[path[0]][path[1]]... or None where any level is missing."""
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def _r(x, nd=4):
    """Round floats for the compact line (None passes through)."""
    if isinstance(x, float):
        return float(f"{x:.{nd}g}")
    return x


def highlights(full: dict) -> dict:
    """The secondary figures worth a glance, one number each, picked from
    the detail objects (every one is in the detail file in full)."""
    h = {
        "auth_level_p50_ms_1M": _get(full, "p50_batch_latency_ms"),
        "auth_level_verifies_per_s": _get(full, "authenticator_level", "value"),
        "device_batch_p50_ms_1M": _get(full, "p50_batch_latency_device_ms"),
        "lone_call_resident_us": _get(full, "single_calls", "p50_latency_resident_us"),
        "lone_call_launch_us": _get(full, "single_calls", "p50_latency_us"),
        "callers16_calls_per_s": _get(full, "single_calls", "concurrent_native",
                                      "threads_16_go_default", "calls_per_s"),
        "callers16_cpu_us_per_call": _get(full, "single_calls", "concurrent_native",
                                          "resident_threads_16_slots_16", "cpu_us_per_call"),
        "lone_call_resident_cpu_us": _get(full, "single_calls", "concurrent_native",
                                          "resident_threads_1_slots_1", "cpu_us_per_call"),
        "callers64_calls_per_s": _get(full, "single_calls", "concurrent_native",
                                      "resident_threads_64_slots_64", "calls_per_s"),
        "callers64_cpu_us_per_call": _get(full, "single_calls", "concurrent_native",
                                          "resident_threads_64_slots_64", "cpu_us_per_call"),
        "go_loop_lone_request_us": _get(full, "go_wiring_latency", "go_default", "small_route",
                                        "1_REQUEST", "p50_us"),
        "go_loop_lone_request_cpu_us": _get(full, "go_wiring_latency", "go_default", "small_route",
                                            "1_REQUEST", "cpu_us_per_window"),
        "go_loop_lone_commit_us": _get(full, "go_wiring_latency", "go_default", "small_route",
                                       "1_COMMIT", "p50_us"),
        "go_loop_512_msgs_us": _get(full, "go_wiring_latency", "go_default", "small_route",
                                    "512_messages", "p50_us"),
        "go_loop_device_1024_msgs_us": _get(full, "go_wiring_latency", "mid_size", "1024_messages", "p50_us"),
        "go_loop_device_4096_msgs_us": _get(full, "go_wiring_latency", "mid_size", "4096_messages", "p50_us"),
        "c3_messages_per_s": _get(full, "c3_usig_streams", "messages_per_s"),
        "c4_auth_level_verifies_per_s": _get(full, "adversarial", "c4_authenticator_level", "value"),
        "c2_with_resident_live_ms_per_step": _get(full, "resident_interference", "c2_ms_per_step",
                                                  "resident_live"),
        "c2_resident_off_ms_per_step": _get(full, "resident_interference", "c2_ms_per_step",
                                            "resident_off"),
    }
    return {k: _r(v) for k, v in h.items() if v is not None}


def compact_line(full: dict, detail_file) -> dict:
    """The one JSON line bench.py prints: the contract's keys, the headline's
    latency / kernel / roofline / SHA stage / CPU baseline, one-number
    highlights, and the path of the detail file holding every other line."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "p50_batch_latency_ms",
            "p50_batch_latency_device_ms", "kernel_ms", "sha256_stage")
    line = {k: full[k] for k in keep if k in full}
    if "p50_batch_latency_ms" in line:
        line["p50_batch_latency_definition"] = ("host submit -> statuses back, 1M VerifyMessageAuthenTag calls "
                                                "through mbft_verify_batch_flat32 (the Go binding's form), median "
                                                "of latency_reps after 3 warm-ups")
    roof = full.get("roofline")
    if roof:
        line["roofline"] = {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic",
                                                     "launch_ms", "steady_state", "executed_mad_frac",
                                                     "peak_source")}
        line["roofline"]["per_unit"] = "10880 limb-MACs/verify x batch verifies per launch (DESIGN.md §4)"
        line["roofline"]["traffic_basis"] = "PMC FETCH_SIZE x2 + WRITE_SIZE per launch (DESIGN.md §2)"
        if isinstance(line["roofline"].get("steady_state"), dict):
            line["roofline"]["steady_state"] = {k: v for k, v in line["roofline"]["steady_state"].items()
                                                if k != "basis"}
    cpu = full.get("cpu_baseline")
    if cpu:
        line["cpu_baseline"] = {k: cpu.get(k) for k in ("value", "unit", "cores", "kind", "impl", "per_cpu",
                                                        "sample", "cpu_us_per_verify", "lscpu_model")
                                if cpu.get(k) is not None}
        line["cpu_baseline"]["lines"] = [{"impl": ln.get("impl"), "value": _r(ln.get("value"))}
                                         for ln in cpu.get("lines", [])]
    else:
        line["cpu_baseline"] = None
    line["highlights"] = highlights(full)
    line["detail_file"] = detail_file
    # hard bound: drop the optional parts, largest first, until it fits
    for k in ("highlights", "sha256_stage", "p50_batch_latency_definition"):
        if len(json.dumps(line)) <= LINE_LIMIT:
            break
        line.pop(k, None)
    return line


def write_detail(full: dict, path: str):
    """The full result (every line) as a side file; returns the path written,
    or None if it could not be written (the compact line still prints)."""
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1, default=float)
        return os.path.relpath(path, ROOT) if path.startswith(ROOT) else path
    except OSError as e:
        print(f"bench: detail file not written: {e}", file=sys.stderr)
        return None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, rank: int, arrays: dict):
    """--dump-outputs: each array as out_dir/<name>.npy in float32 (ranks
    past 0 add _rank<r> to the name).  The arrays share DUMP_LIMIT_BYTES
    evenly; a larger one is cut to a sorted sample of its first axis drawn
    from a fixed seed, so two runs keep the same rows."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.asarray(a)
        row_bytes = 4 * max(int(np.prod(a.shape[1:])), 1)
        if a.shape[0] * row_bytes > share:
            keep = np.random.Generator(np.random.PCG64(0xD0)).choice(a.shape[0], size=share // row_bytes,
                                                                    replace=False)
            a = a[np.sort(keep)]
        suffix = f"_rank{rank}" if rank else ""
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a.astype(np.float32))


def main():
    args = parse()
    from minbft_amd import dist as mdist
    # --gpus N is authoritative: under torch.distributed.run WORLD_SIZE must
    # equal N; without a launcher, N > 1 restarts this script as N ranks of a
    # child torch.distributed.run (nothing has touched a GPU yet) and relays
    # rank 0's JSON line
    if mdist.launch_mode(args.gpus) == "relaunch":
        sys.exit(mdist.relaunch(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    import torch
    import torch.distributed as dist

    world, rank, local = mdist.env_ranks()
    # the microbenchmark runs as a child program BEFORE this process
    # initializes the GPU
    peak = measure_peak_mad_rate(run=not args.no_peak_run) if rank == 0 and args.full else None
    use_dist = world > 1 or args.force_dist
    if use_dist:
        # RCCL prints a version banner on stdout at communicator creation;
        # keep stdout for the one JSON line (banner -> stderr)
        with _stdout_to_stderr():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            dist.barrier()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    from minbft_amd import build
    build.build()
    from minbft_amd.authenticator import Authenticator, ROLE_CLIENT, der_encode_rows

    B = args.batch
    auth = Authenticator(local)
    # Caller streams the batches rotate over (--streams, default 3).  A
    # batch's s^-1 chain waits for the work already on its stream (the
    # inputs' stream order), i.e. for the verify kernel of the batch that
    # stream ran before; with three streams two other batches' verify
    # kernels keep the GPU busy meanwhile (pipelining).
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(args.streams, 1))]
    try:
        # table_build_s: the two comb-table builds alone (generator, key);
        # the synthetic inputs (1M ops hashed with hashlib, the SHA stage,
        # 1M GPU signatures) are timed apart as inputs_s
        t_tab = time.perf_counter()
        if args.g_window != 16:
            auth.set_generator_window(args.g_window)
        t_tab = time.perf_counter() - t_tab
        t_inp = time.perf_counter()
        # single signer (client 0)
        d = int.from_bytes(hashlib.sha256(b"minbft-amd bench client 0").digest(), "big")
        d = d % (0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551 - 1) + 1
        priv = np.frombuffer(d.to_bytes(32, "big"), dtype=np.uint8).copy()
        msgs, ops, seqs = make_requests(rank, B, with_ops=True)
        e = np.ascontiguousarray(msgs[:, :32])  # quirk: e = (msg || SHA256(""))[0:32]
        d_priv = torch.from_numpy(priv).to(dev)
        d_e = torch.from_numpy(e).to(dev)
        sha = sha256_stage(auth, torch, dev, streams[0], ops, seqs, d_e) if args.full else None
        del ops
        d_r = torch.empty((B, 32), dtype=torch.uint8, device=dev)
        d_s = torch.empty((B, 32), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        auth.sign_prehashed_device(d_priv.data_ptr(), 0, d_e.data_ptr(), B, d_r.data_ptr(),
                                   d_s.data_ptr(), stream)
        torch.cuda.synchronize()
        # the signer's public key Q = d*G, computed once with Python big
        # integers (synthetic input, outside every timed region)
        qxy = pubkey_bytes(d)
        t_inp = time.perf_counter() - t_inp
        t_key = time.perf_counter()
        auth.set_key_window(args.q_window)
        auth.add_role(ROLE_CLIENT)
        auth.set_public_key(ROLE_CLIENT, 0, qxy)
        slot = auth.key_slot(ROLE_CLIENT, 0)
        t_key = time.perf_counter() - t_key
        t_tab += t_key
        d_slot = torch.full((B,), slot, dtype=torch.int32, device=dev)
        # Two caller streams, alternated per batch: the library runs batch
        # i+1's s^-1 kernels on its internal stream as soon as the batch is
        # issued, overlapping batch i's verify kernel.
        d_sts = [torch.empty((B,), dtype=torch.uint8, device=dev) for _ in streams]
        d_st = d_sts[0]
        nstep = [0]
        # The timed batch: the valid batch with the reject mix in it (about
        # 1 item in 100 altered), so that the statuses a step returns say
        # something: t_want holds every item's status by construction.
        t_e, t_r, t_s, t_want, _ = reject_mix(torch, dev, d_e, d_r, d_s, B)

        def step():
            k = nstep[0] % len(streams)
            nstep[0] += 1
            auth.verify_prehashed_device(t_e.data_ptr(), t_r.data_ptr(), t_s.data_ptr(),
                                         d_slot.data_ptr(), B, d_sts[k].data_ptr(),
                                         streams[k].cuda_stream)

        # correctness gate at the benchmarked windows: the timed batch (the
        # valid batch with the reject mix -- every 97th item: flipped e byte,
        # s = N, r = 0, or high s, which Go accepts) comes back exactly as
        # constructed on every stream, and so does the mix built and run once
        # more on its own (reject_gate)
        for _ in streams:
            step()
        torch.cuda.synchronize()
        n_diff = max(int((d != t_want).sum().item()) for d in d_sts)
        if n_diff:
            raise SystemExit(f"bench correctness gate failed: {n_diff}/{B} statuses differ from the construction")
        gate = reject_gate(auth, torch, dev, d_e, d_r, d_s, d_slot, B, streams[0])
        # The sustained gate: --gate-batches more batches back to back over
        # the streams, every status vector checked on the device (a count of
        # statuses that differ from the construction, per stream, enqueued
        # behind each batch on its stream:
        # no host synchronize between batches).  It ends right before the W
        # warm-up steps, so they and the K timed steps start from the clock
        # of sustained load: from an idle GPU the first ~20 ms of batches run
        # ~13 % slow (tools/ramp_probe.py, profiles/round6_ramp_probe.jsonl),
        # which a 5-step warm-up does not cover.
        bads = [torch.zeros((), dtype=torch.int64, device=dev) for _ in streams]
        for _ in range(args.gate_batches):
            k = nstep[0] % len(streams)
            step()
            with torch.cuda.stream(streams[k]):
                bads[k] += (d_sts[k] != t_want).sum()
        torch.cuda.synchronize()
        n_bad = sum(int(b.item()) for b in bads)
        if n_bad:
            raise SystemExit(f"bench sustained gate failed: {n_bad} statuses differ from the construction")
        gate["sustained_batches_checked"] = args.gate_batches

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        auth.profile(True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        t1 = time.perf_counter()
        prof = auth.profile_read()
        auth.profile(False)
        dt = t1 - t0
        dt = mdist.max_over_ranks(dist, dt, dev)  # MAX over ranks (no-op at N=1)
        if args.dump_outputs:
            # what the caller of the last timed step got back: that batch's
            # statuses (the stream it ran on is the last one used)
            last = (nstep[0] - 1) % len(streams)
            dump_outputs(args.dump_outputs, rank, {"statuses": d_sts[last].cpu().numpy()})
        head = {
            "metric": "ECDSA-P256 verifies/sec at batch 1M (1/2/4/8 GPU); p50 batch latency",
            "value": world * B * args.steps / dt,
            "unit": "verifies/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32 (29-bit-limb mod-p/mod-N integer arithmetic)",
            "data": "synthetic: seeded 256-byte REQUEST ops, GPU-signed (deterministic nonce)",
            "config": {"workload": "C2: 1M single-signer REQUEST ECDSA-P256 verify batch per GPU "
                                   "(Authenticator ClientAuthen, Sum(m) digest), inputs resident in HBM",
                       "batch_per_gpu": B, "parallelism": f"independent shards x{world}",
                       "comb_windows": {"G": args.g_window, "Q": args.q_window},
                       "batches_in_flight": len(streams),
                       "reject_mix": "every 97th item altered (flipped e byte, s = N, r = 0: reject; "
                                     "N - s: accept), so a step's statuses are not all zero"},
            "table_build_s": t_tab,
            "table_build_basis": f"generator (W = {args.g_window}) + key (W = {args.q_window}) comb tables "
                                 f"only: {t_tab - t_key:.2f} s + {t_key:.2f} s",
            "inputs_s": t_inp,
        }
        if not args.full:
            # the plain run ends here: the headline alone (every other line
            # is behind --full)
            result = None
            if rank == 0:
                nb = max(prof["batches"], 1)
                result = {**head, "gate": gate,
                          "kernel_ms": {"k_verify_in_timed_loop_overlapped": prof["verify_ms"] / nb,
                                        "batched_inverse_span_overlapped": prof["inverse_ms"] / nb}}
                print(json.dumps(compact_line(result, None)), flush=True)
            if use_dist:
                dist.barrier()
                dist.destroy_process_group()
            return result

        # per-step device latency (synchronized), p50
        # one batch at a time (synchronized): p50 batch latency, and the
        # k_verify launch duration without a neighbouring batch's kernels on
        # the GPU (HIP events on the kernel's stream)
        # (two loops: the library splits an idle batch into two overlapped
        # parts -- host.cpp verify_device -- except while profiling, which
        # times whole 1M-item kernels for the roofline)
        lat_dev = []
        for _ in range(args.latency_reps):
            torch.cuda.synchronize()
            a = time.perf_counter()
            step()
            torch.cuda.synchronize()
            lat_dev.append(time.perf_counter() - a)
        auth.profile(True)
        lat_dev_unsplit = []
        for _ in range(args.latency_reps):
            torch.cuda.synchronize()
            a = time.perf_counter()
            step()
            torch.cuda.synchronize()
            lat_dev_unsplit.append(time.perf_counter() - a)
        prof_iso = auth.profile_read()
        auth.profile(False)
        # host submit -> status back (PCIe-inclusive), p50 over 20 after 3 warm
        r_h = d_r.cpu().numpy()
        s_h = d_s.cpu().numpy()
        slots_h = np.full(B, slot, dtype=np.uint32)
        lat_pre = []
        for k in range(3 + args.latency_reps):
            a = time.perf_counter()
            st = auth.verify_prehashed(e, r_h, s_h, slots_h)
            b = time.perf_counter() - a
            if k >= 3:
                lat_pre.append(b)
        assert int((st == 0).sum()) == B
        # The authenticator level (BASELINE.md §2 GPU row): mbft_verify_batch
        # over the C2 calls VerifyMessageAuthenTag(ClientAuthen, 0, msg, tag)
        # with host buffers in and statuses out -- DER decode, Sum(m) digest,
        # H2D, s^-1 + verify kernels, D2H, in-order resolution.  p50 over
        # latency_reps batches after 3 warm-ups = the metric's p50 batch latency.
        tags, tlen = der_encode_rows(r_h, s_h)
        items = Authenticator.pack_items(ROLE_CLIENT, 0, msgs, 47, tags, tlen)
        st_b = np.zeros(B, dtype=np.uint8)
        lat_auth = []
        auth.stage_profile()  # reset
        for k in range(3 + args.latency_reps):
            a = time.perf_counter()
            auth.verify_batch_items(items, st_b)
            b = time.perf_counter() - a
            if k == 2:
                auth.stage_profile()  # drop the warm-ups
            if k >= 3:
                lat_auth.append(b)
        stages = auth.stage_profile()
        if int((st_b == 0).sum()) != B:
            raise SystemExit(f"authenticator-level gate failed: {int((st_b == 0).sum())}/{B} accepted")
        # The same calls as the Go binding passes them: mbft_verify_batch_flat
        # over flat buffers in library page-locked memory (go/gpuauth marshals
        # into mbft_host_alloc arenas), so the calls are decoded on the GPU
        # (k_prepare) and the host reads none of their bytes.
        lat_wide, stages_wide, st_f = flat_pinned_level(auth, msgs, tags, tlen, B, args.latency_reps)
        if int((st_f == 0).sum()) != B:
            raise SystemExit(f"flat device-decode gate failed: {int((st_f == 0).sum())}/{B} accepted")
        # the Go binding's form (go/gpuauth: mbft_verify_batch_flat32, ECDSA
        # messages as their 32-byte e prefix) -- the headline p50
        lat_flat, stages_flat, st_f = flat_pinned_level(auth, msgs, tags, tlen, B, args.latency_reps,
                                                        compact=True)
        if int((st_f == 0).sum()) != B:
            raise SystemExit(f"compact flat gate failed: {int((st_f == 0).sum())}/{B} accepted")
        single = single_calls(auth, msgs, tags, tlen)
        interf = None
        if not args.no_extra_lines:
            interf = resident_interference(auth, torch, step, max(args.steps, 200), msgs, tags, tlen, B,
                                           max(args.latency_reps, 10))
        # (before the adversarial / C3 lines, which replace the key store)
        conc = None if args.no_extra_lines else concurrency_line(auth, msgs, tags, tlen)
        adv = None
        if not args.no_adversarial:
            adv = adversarial(auth, torch, dev, streams, B, d, d_e, d_r, d_s, d_slot,
                              float(np.median(lat_dev)), args.q_window, dist if use_dist else None, msgs)
        c3 = None
        if args.c3_requests:
            c3 = c3_line(auth, torch, dev, args.c3_requests)
        lowload = None
        if not args.no_extra_lines:
            lowload = go_wiring_latency(auth)
            # mid-size passes: windows of 1,024 - 4,096
            # messages, past the small route, through the device message
            # layer (a 1,024-request stream)
            lowload["mid_size"] = go_wiring_latency(auth, nreq=1024, sizes=(1024, 2048, 4096),
                                                    configs=(("go_default", 4, True, 32),), c5=False,
                                                    routes=(("device_layer", 0),))["go_default"]["device_layer"]
        binding = None
        if not args.no_extra_lines:
            binding = binding_lines(auth, torch, dev, streams, B, d_e, min(args.steps, 100),
                                    min(args.warmup, 10))
        multi = None
        if use_dist:
            dist.barrier()
        if use_dist and world > 1 and not args.no_extra_lines:
            # one context over all devices needs every device's memory: the
            # ranks drop their tables first
            auth.close()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            dist.barrier()
            if rank == 0:
                multi = multi_engine_line(world, B, msgs, tags, tlen, qxy, args.g_window, args.q_window,
                                          args.latency_reps)
            dist.barrier()

        result = None
        if rank == 0:
            # k_verify launches in the timed loop overlap the next batch's
            # launch (two caller streams): their event-bracketed duration is
            # longer than the kernel's own.  The roofline uses the isolated
            # launches; the steady-state figure uses the time per step.
            verify_ms_overlapped = prof["verify_ms"] / max(prof["batches"], 1)
            verify_ms = (prof_iso["verify_ms"] / max(prof_iso["batches"], 1)
                         if prof_iso["batches"] else verify_ms_overlapped)
            inv_ms = prof["inverse_ms"] / max(prof["batches"], 1)
            peak, peak_src = peak
            m256, limb_macs, exec_mads = work_per_verify(args.g_window, args.q_window)
            traffic, traffic_src = read_traffic(args.g_window, args.q_window)
            achieved = B * limb_macs / (verify_ms * 1e-3)
            executed = B * exec_mads / (verify_ms * 1e-3)
            survey = B * SURVEY_LIMB_MACS_PER_VERIFY / (verify_ms * 1e-3)
            cpu = None
            if not args.no_cpu_baseline:
                cpu = cpu_baseline(msgs, tags, tlen, qxy, args.cpu_sample, args.cpu_port_sample)
            if cpu and lowload and cpu.get("value"):
                # Go verifies a message's signatures one after another on one
                # goroutine: the primary's commit path is 6 verifies in a row
                per_verify_us = cpu["cores"] / cpu["value"] * 1e6
                lowload["c5_proxy"]["cpu_reference"] = {
                    "per_verify_us": per_verify_us, "commit_path_us": 6 * per_verify_us,
                    "basis": "cpu_baseline (OpenSSL, not Go): one CPU's time per verify x the 6 "
                             "signature checks of the primary's commit path"}
            p50_items = float(np.median(lat_auth))
            p50_auth = float(np.median(lat_flat))
            result = {
                **head,
                "p50_batch_latency_ms": p50_auth * 1e3,
                "p50_batch_latency_definition": "host submit -> statuses back for 1M VerifyMessageAuthenTag "
                                                "calls through mbft_verify_batch_flat32 as the Go binding calls "
                                                "it (compact flat buffers in library page-locked memory, each "
                                                "REQUEST's message as its 32-byte e prefix: PCIe, GPU decode "
                                                "of DER + digest + key, kernels, statuses), "
                                                f"median of {args.latency_reps} batches after 3 warm-ups",
                "p50_batch_latency_device_ms": float(np.median(lat_dev) * 1e3),
                "p50_batch_latency_device_unsplit_ms": float(np.median(lat_dev_unsplit) * 1e3),
                "p50_batch_latency_prehashed_host_ms": float(np.median(lat_pre) * 1e3),
                "authenticator_level": {
                    "entry": "mbft_verify_batch_flat32 (compact, library page-locked buffers, GPU decode)",
                    "items": B, "value": B / p50_auth, "unit": "verifies/s (p50 batch, host in / host out)",
                    "bytes_per_call": 1 + 4 + 4 + 4 + 32 + float(tlen.mean()) + 1,
                    "stages_ms_per_batch": stages_flat, "gate": "all accepted",
                    "wide_form": {"entry": "mbft_verify_batch_flat (u32 roles, u64 offsets, 47-byte messages)",
                                  "p50_ms": float(np.median(lat_wide)) * 1e3,
                                  "value": B / float(np.median(lat_wide)),
                                  "bytes_per_call": 4 + 4 + 8 + 8 + 47 + float(tlen.mean()) + 1,
                                  "stages_ms_per_batch": stages_wide},
                    "host_decode": {
                        "entry": "mbft_verify_batch (mbft_item array: host DER + digest on the worker pool)",
                        "p50_ms": p50_items * 1e3, "value": B / p50_items,
                        "stages_ms_per_batch": stages, "gate": "all accepted"}},
                "single_calls": single,
                "resident_interference": interf,
                "gate": gate,
                "adversarial": adv,
                "c3_usig_streams": c3,
                "go_wiring_latency": lowload,
                "concurrent_batches": conc,
                "binding_configs": binding,
                "multi_engine_authenticator_level": multi,
                "kernel_ms": {"k_verify": verify_ms,
                              "k_verify_in_timed_loop_overlapped": verify_ms_overlapped,
                              "batched_inverse_span_overlapped": inv_ms},
                "roofline": {
                    "bound": "valu",
                    "achieved": achieved / 1e12,
                    "peak": peak / 1e12,
                    "unit": "TOP/s (limb-MAC = one 32x32->64 v_mad_u64_u32)",
                    "frac": achieved / peak,
                    "traffic": traffic,
                    "traffic_basis": f"PMC per launch ({traffic_src}: FETCH_SIZE x2 gfx950 correction + "
                                     "WRITE_SIZE): 128-B fabric read requests = 18 comb entries + ~1.2 input "
                                     "lines per verify; a random 64-B entry always costs a 128-B line "
                                     "(profiles/round2_pmc_rdreq.json), so 2x the 1.31 GB algorithmic bytes is "
                                     "the floor for this access pattern",
                    "per_unit": f"{limb_macs} limb-MACs/verify ({m256} M256 = 6 (affine first add) + "
                                f"{mixed_adds(args.g_window, args.q_window)} Chudnovsky mixed adds x 10 + "
                                f"2 (u1, u2) + 2 (x-check), DESIGN.md §4) x {B} verifies per launch",
                    "peak_source": peak_src,
                    "launch_ms": verify_ms,
                    "steady_state": {"achieved": B * limb_macs / (dt / args.steps) / 1e12,
                                     "frac": B * limb_macs / (dt / args.steps) / peak,
                                     "basis": "ms_per_step (overlapped batches)"},
                    "executed_mad_frac": executed / peak,
                    "survey_yardstick_frac": survey / peak,
                },
                "sha256_stage": sha,
                "cpu_baseline": cpu,
            }
            detail = write_detail(result, args.detail_out)
            print(json.dumps(compact_line(result, detail)), flush=True)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return result
    finally:
        auth.close()


# Synthetic-input point arithmetic (Python bigint, affine; None = infinity):
# key generation and crafted adversarial signatures, outside timed regions.
P_FIELD = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
G_POINT = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
           0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)


def pt_add(p, q):
    P = P_FIELD
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = (3 * p[0] * p[0] + P - 3) * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return (x, (lam * (p[0] - x) - p[1]) % P)


def pt_mul(k: int, pt):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = pt_add(acc, acc)
        if bit == "1":
            acc = pt_add(acc, pt)
    return acc


def pubkey_bytes(d: int) -> bytes:
    """Q = d*G (affine, 64 B) -- host-side key generation for the synthetic
    signer, outside the timed region."""
    acc = pt_mul(d, G_POINT)
    return acc[0].to_bytes(32, "big") + acc[1].to_bytes(32, "big")


def signed_digits(u: int, W: int):
    """The comb's signed-digit recoding of u (k_verify comb_digit), low
    window first."""
    S = (256 + W - 1) // W
    out, carry = [], 0
    for i in range(S):
        x = ((u >> (W * i)) & ((1 << W) - 1)) + carry
        neg = i + 1 < S and x > (1 << (W - 1))
        out.append(x - (1 << W) if neg else x)
        carry = 1 if neg else 0
    return out


def craft_degenerate(d: int, W: int, m: int, seed: int):
    """m valid signatures of signer d (key window W) whose verification hits
    a DEGENERATE mixed addition in the key phase: the accumulator u1 G +
    P_j Q equals +-(the next entry d_j 2^(Wj) Q).  That needs the key's
    discrete log (u1 = d (+-d_j 2^(Wj) - P_j)), so only a key owner can make
    it; k_verify sends such lanes (ZZ == 0) to the exact path (k_verify_slow)."""
    import random
    rng = random.Random(seed)
    N = N_ORDER
    q = pt_mul(d, G_POINT)
    rows = []
    while len(rows) < m:
        u2 = rng.randrange(1, N)
        dig = signed_digits(u2, W)
        j = rng.randrange(0, len(dig))
        if dig[j] == 0:
            continue
        pj = sum(dig[i] << (W * i) for i in range(j))
        sign = 1 if rng.random() < 0.5 else -1
        u1 = d * (sign * (dig[j] << (W * j)) - pj) % N
        R = pt_add(pt_mul(u1, G_POINT), pt_mul(u2, q))
        if R is None or R[0] % N == 0:
            continue
        r = R[0] % N
        s_ = r * pow(u2, -1, N) % N
        rows.append((u1 * s_ % N, r, s_))
    return rows


if __name__ == "__main__":
    main()
