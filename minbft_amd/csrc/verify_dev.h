// Device code the verifier's kernel units share (verify_large.hip,
// verify_pairs.hip, verify_quads.hip, verify_split.hip, verify_server.hip): the
// comb over the tables (comb_entry, the LDS gathers, comb_step, comb_run,
// comb_verify_fast, comb_complete), an item's scalars and its accept test
// (load_scalars, verify_finish), the exact and table-free paths (verify_exact,
// verify_ladder_item), the admission rule (admit), the compacted queues
// (queue_push) and the joins of the lane-group forms (comb_start_affine,
// chud_shfl_xor, verify_dead, verify_join).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecc.h"
#include "kernels.h"
#include "ladder_dev.h"
#include "modinv.h"
#include "scalar_dev.h"
#include "teeth_dev.h"
#include "verify_args.h"
#include "words_dev.h"

// The table-free items' queue (k_verify -> k_verify_ladder) inside the
// `slowq` buffer (verify_plan.h): its length right after the exact-path
// queue's, its n entries from ladder_queue_offset.  Derived from slowq /
// slown, so the kernels' argument block is what it was.
static_assert(kSpillPlanes == 4 * NL, "Spill: X, Y, ZZ, ZZZ of NL limbs");
MBFT_DEV uint32_t* ladder_count(const VerifyArgs& A) { return A.slown + 1; }
MBFT_DEV uint32_t* ladder_queue(const VerifyArgs& A) { return A.slowq + ladder_queue_offset(A.n); }

MBFT_DEV const uint4* comb_entry(const uint32_t* tab, int W, int step, uint32_t idx) {
  return reinterpret_cast<const uint4*>(tab + ((((size_t)step) << (W - 1)) + idx) * 16u);
}

// y -> -y (p - y) where `neg`; y canonical < p
MBFT_DEV void fe_cneg(fe& y, bool neg) {
  fe t;
  fe_neg(t, y);
  fe_select(y, neg, t, y);
}

// Table gathers of the verifier fast path go straight into LDS (gfx950
// global_load_lds_dwordx4: lane l's 16 B land at base + 16 l), so the entry
// prefetched one step ahead holds no VGPRs across the mixed addition; the
// lane reads its 64 B back when the step starts.  Per wave a 4 KB buffer:
// 4 slots of 64 x 16 B.
//
// COOP (cooperative gather): every step each lane needs one random 64-B
// entry.  Loaded lane by lane, each of the 4 load instructions touches 64
// unrelated table pages: 256 address translations and cache-line requests
// per wave per step, which at 258 GiB of tables miss the per-CU TLB 86 % of
// the time (PMC TCP_UTCL1_TRANSLATION_MISS).  Cooperatively,
// load k fetches 16-B chunk (lane & 3) of the entries of lanes 16k .. 16k+15
// (their addresses come in by ds_bpermute): 16 entries per instruction, 64
// translations and requests per step.  Needs all 64 lanes of the wave in
// the loop with valid addresses (verify_one).  Without COOP, load k fetches
// chunk k of the lane's own entry.
#ifndef MBFT_GATHER_CPOL
#define MBFT_GATHER_CPOL 2  // table gathers non-temporal (nt): +1 % same-box, A/B builds
#endif
constexpr unsigned kWaitVm0 = 0x0F70;    // s_waitcnt vmcnt(0)
constexpr unsigned kWaitLgkm0 = 0xC07F;  // s_waitcnt lgkmcnt(0)

template <bool COOP>
MBFT_DEV void gather_issue(const uint4* mine, uint4* buf) {
  const int lane = __lane_id();
  __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // the previous reads of buf are done
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint4* src;
    if (COOP) {
      const uint64_t a = reinterpret_cast<uint64_t>(mine);
      const int from = (16 * k + (lane >> 2)) << 2;
      const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)a);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)(a >> 32));
      src = reinterpret_cast<const uint4*>(((uint64_t)hi << 32) | lo) + (lane & 3);
    } else {
      src = mine + k;
    }
    __builtin_amdgcn_global_load_lds(src, buf + 64 * k, 16, 0, MBFT_GATHER_CPOL);
  }
}

// This lane's entry from the buffer (waits for the gathers).  COOP: slot
// 64k + l holds chunk (l & 3) of the entry of lane 16k + (l >> 2), so the
// lane's 4 chunks are slots 4 lane .. 4 lane + 3.
template <bool COOP>
MBFT_DEV void gather_read(fe& px, fe& py, const uint4* buf) {
  const int lane = __lane_id();
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  uint4 c[4];
#pragma unroll
  for (int k = 0; k < 4; k++) c[k] = COOP ? buf[4 * lane + k] : buf[64 * k + lane];
  uint32_t wx[8] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w};
  uint32_t wy[8] = {c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w};
  fe_from_words(px, wx);
  fe_from_words(py, wy);
}

#ifdef MBFT_STEP_TIMING
// Comb-step stamps of a timing build (-DMBFT_STEP_TIMING): a wave's cycles over
// its comb steps, summed by comb_step and added to g_step_clk by verify_one
// (verify_large.hip, where the phases are listed).
struct StepClock {
  unsigned long long s[4] = {0, 0, 0, 0};
  unsigned long long steps = 0;
};
#else
struct StepClock {};
#endif

// Rare comb steps (a zero digit, or an accumulator still at infinity) are
// resolved around the unconditional in-place mixed addition without holding
// any extra registers across it: before it, a zero-digit lane spills its
// accumulator and an infinity lane its entry to per-thread scratch
// (coalesced planes, A.scr); after it, the zero-digit lane reloads the
// accumulator (the addition is skipped, its Y sign unflipped) and the
// infinity lane becomes the entry (Z = 1).  Both are wave-uniform branches
// that honest inputs take with probability ~2^-(W-1) per window.
// Addresses are 32-bit word offsets from the (uniform) scratch base, made
// opaque where they are used: otherwise the compiler hoists the 36 per-lane
// 64-bit addresses out of the comb loop and spills them.
struct Spill {
  uint32_t* base;   // A.scr (wave-uniform)
  uint32_t tid;     // this thread's column
  uint32_t stride;  // words per plane
  MBFT_DEV void put(int k, const fe& a) const {
    uint32_t t = tid;
    asm volatile("" : "+v"(t));
#pragma unroll
    for (int j = 0; j < NL; j++) base[t + (uint32_t)(k * NL + j) * stride] = a.v[j];
  }
  MBFT_DEV void get(int k, fe& a) const {
    uint32_t t = tid;
    asm volatile("" : "+v"(t));
#pragma unroll
    for (int j = 0; j < NL; j++) a.v[j] = base[t + (uint32_t)(k * NL + j) * stride];
  }
};

// One comb step (the body of comb_run's loop, below; LAST: the peeled final
// step of a LAST_XZ run, whose addition skips ZZZ and Y).
template <bool COOP, bool LAST>
MBFT_DEV void comb_step(chud& acc, bool& inf, bool& yneg, bool& neg, bool& zero, uint32_t (&U)[8],
                        const uint32_t* tab, int W, int S, int step, uint32_t& carry, uint4* buf,
                        const Spill& sp, bool live, StepClock& sc) {
  fe px, py;
#ifdef MBFT_STEP_TIMING
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#endif
  gather_read<COOP>(px, py, buf);
#ifdef MBFT_STEP_TIMING
  __builtin_amdgcn_s_waitcnt(kWaitLgkm0);
  const unsigned long long t2 = __builtin_amdgcn_s_memtime();
#endif
  shr_words(U, W);
  bool nneg, nzero;
  const uint32_t in = comb_digit(U[0], carry, W, step + 2 >= S, nneg, nzero);
  gather_issue<COOP>(comb_entry(tab, W, step + 1 < S ? step + 1 : step, in), buf);
#ifdef MBFT_STEP_TIMING
  const unsigned long long t3 = __builtin_amdgcn_s_memtime();
#endif
  // dead lanes (zero scalars, results discarded) never count as rare
  const bool rare = __ballot(live && (zero || inf)) != 0;
  if (rare && live) {
    if (zero) {
      sp.put(0, acc.X);
      sp.put(1, acc.Y);
      sp.put(2, acc.ZZ);
      sp.put(3, acc.ZZZ);
    } else if (inf) {
      sp.put(0, px);
      sp.put(1, py);
    }
  }
  ec_madd_chud<true, LAST>(acc, acc, px, py, yneg != neg);  // Y takes the digit's sign (ecc.h)
  const bool yold = yneg;
  yneg = neg;
  if (rare && live) {
    if (zero) {  // d = 0: nothing added
      sp.get(0, acc.X);
      sp.get(1, acc.Y);
      sp.get(2, acc.ZZ);
      sp.get(3, acc.ZZZ);
      yneg = yold;
    } else if (inf) {  // infinity + entry = entry (Z = 1); acc.Y holds t y2
      sp.get(0, acc.X);
      sp.get(1, acc.Y);
      fe_one_mont(acc.ZZ);
      fe_one_mont(acc.ZZZ);
      yneg = neg;
      inf = false;
    }
  }
  neg = nneg;
  zero = nzero;
#ifdef MBFT_STEP_TIMING
  const unsigned long long t4 = __builtin_amdgcn_s_memtime();
  sc.s[0] += t1 - t0;
  sc.s[1] += t2 - t1;
  sc.s[2] += t3 - t2;
  sc.s[3] += t4 - t3;
  sc.steps += 1;
#else
  (void)sc;
#endif
}

// Verifier fast path: acc (a Chudnovsky point, or `inf`) += the signed-digit
// entries of windows step0 .. S-1 of U (`carry` = the recoding carry into
// window step0).  Every step is the in-place mixed addition, so the common
// loop carries no control-flow merge and no register copies; the next entry
// is in flight one step ahead.  Zero digits and infinity are exact (the rare
// branches above: an attacker who picks s controls u1 or u2 and can force
// them, so they are not sent to the slow path).  `yneg`: acc.Y holds -Y
// (ec_madd_chud: after an addition, the sign of the digit it added); a
// negative digit's -y is folded into the same per-lane select.  A degenerate
// addition (acc == +-entry) leaves ZZ == 0 for good, which the caller
// detects.  COOP: cooperative gathers (W and the loop wave-uniform); else
// per lane.  acc.ZZ and acc.ZZZ are kept lazy (ecc.h ec_madd_chud<true>):
// the caller normalizes them (fe_norm_lazy) before any other use.  LAST_XZ
// (with COOP: S is wave-uniform): this run ends the
// chain and only X, ZZ are read afterwards (the x-check): the final step is
// peeled and its addition skips ZZZ and Y.
// (end_ >= 0: stop before window end_ -- a range's low part, k_verify_quads;
// the entry gathered ahead for window end_ goes unused)
template <bool COOP, bool LAST_XZ = false>
MBFT_DEV void comb_run(chud& acc, bool& inf, bool& yneg, uint32_t (&U)[8], const uint32_t* tab,
                       int W, int step0, uint32_t carry, uint4* buf, const Spill& sp, bool live,
                       StepClock& sc, int end_ = -1) {
  static_assert(COOP || !LAST_XZ, "the peeled last step needs a wave-uniform window");
  const int S = (256 + W - 1) / W;
  bool neg, zero;
  const uint32_t idx = comb_digit(U[0], carry, W, step0 + 1 >= S, neg, zero);
  gather_issue<COOP>(comb_entry(tab, W, step0, idx), buf);
  const int end = end_ >= 0 ? end_ : (LAST_XZ ? S - 1 : S);
#pragma unroll 1
  for (int step = step0; step < end; step++)
    comb_step<COOP, false>(acc, inf, yneg, neg, zero, U, tab, W, S, step, carry, buf, sp, live, sc);
  if (LAST_XZ && S - 1 >= step0)
    comb_step<COOP, true>(acc, inf, yneg, neg, zero, U, tab, W, S, S - 1, carry, buf, sp, live, sc);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);  // the last (unused) gather is done with buf
}

// acc = u1 G + u2 Q over the comb tables, fast path: the first two G windows
// are one affine + affine addition, all later windows are mixed additions.
// Returns true if the sum is the point at infinity (Go's Verify: (0, 0),
// reject).  A degenerate addition (only constructible with the key's
// discrete log) leaves ZZ == 0: the caller sends that lane to the exact path.
// The G phase (one table, one window) always gathers cooperatively; the Q
// phase when QCOOP (the wave's key windows agree).
template <bool QCOOP>
MBFT_DEV bool comb_verify_fast(chud& acc, uint32_t (&U1)[8], uint32_t (&U2)[8],
                               const uint32_t* tabG, int wg, const uint32_t* tabQ, int wq,
                               uint4* buf, const Spill& sp, bool live, StepClock& sc) {
  uint32_t carry = 0;
  bool neg0, zero0, neg1, zero1;
  const uint32_t i0 = comb_digit(U1[0], carry, wg, false, neg0, zero0);
  shr_words(U1, wg);
  const uint32_t i1 = comb_digit(U1[0], carry, wg, false, neg1, zero1);
  shr_words(U1, wg);
  {
    // the first two G windows: affine + affine.  acc.Y holds +-Y (only X and
    // Z are read afterwards): a negative first digit just starts the lane
    // with Y negated.
    fe x0, y0, x1, y1;
    gather_issue<true>(comb_entry(tabG, wg, 0, i0), buf);
    gather_read<true>(x0, y0, buf);
    gather_issue<true>(comb_entry(tabG, wg, 1, i1), buf);
    gather_read<true>(x1, y1, buf);
    ec_add_affine_chud(acc, x0, y0, x1, y1, neg0 != neg1);
  }
  bool yneg = !neg0, inf = false;
  if (__ballot(live && (zero0 || zero1)) != 0) {
    // a zero digit among the first two: the sum is the other entry (Z = 1,
    // reloaded per lane), or infinity if both are zero
    if (zero0 && zero1) {
      inf = true;
    } else if (zero0 || zero1) {
      load_point(acc.X, acc.Y, comb_entry(tabG, wg, zero0 ? 1 : 0, zero0 ? i1 : i0));
      fe_one_mont(acc.ZZ);
      fe_one_mont(acc.ZZZ);
      yneg = zero0 ? neg1 : neg0;
    }
  }
  // never degenerate in the G phase: |partial sum| < |next addend| as
  // integers, and partial + addend == u1 != 0 at the top
  comb_run<true>(acc, inf, yneg, U1, tabG, wg, 2, carry, buf, sp, live, sc);
  comb_run<QCOOP, QCOOP>(acc, inf, yneg, U2, tabQ, wq, 0, 0u, buf, sp, live, sc);
  fe_norm_lazy(acc.ZZ);
  return inf;
}

// Same sum with exact handling of doubling / opposite points / infinity.
MBFT_DEV void comb_complete(jac& acc, bool& inf, uint32_t (&U)[8], const uint32_t* tab, int W) {
  const int S = (256 + W - 1) / W;
  uint32_t carry = 0;
#pragma unroll 1
  for (int step = 0; step < S; step++) {
    bool neg, zero;
    const uint32_t idx = comb_digit(U[0], carry, W, step + 1 >= S, neg, zero);
    shr_words(U, W);
    if (zero) continue;
    fe px, py;
    load_point(px, py, comb_entry(tab, W, step, idx));
    fe_cneg(py, neg);
    ec_madd_complete(acc, inf, px, py);
  }
}

// Load e, r, s^-1 of item i and compute u1, u2 words.  LANE_INV: s^-1 by
// this lane (small batches, k_verify_pairs, A.winv null); else from the
// batched planes.  A template, so the large-batch kernel carries no
// inversion code (it would cost registers there).
template <bool LANE_INV>
MBFT_DEV void load_scalars(const VerifyArgs& A, long i, uint32_t (&U1)[8], uint32_t (&U2)[8],
                          const fe* wpre = nullptr) {
  uint32_t ew[8], rw[8];
  load_be256(ew, A.e + 32 * i);
  load_be256(rw, A.r + 32 * i);
  fe w, e, r;
  if (!LANE_INV) {
    plane_load(w, A.winv, A.n, i);
  } else if (wpre) {
    w = *wpre;  // inverted by the whole wave (verify_pair: one item in the wave)
  } else {
    // small batches (verify_device): this lane's own s^-1 by variable-time
    // divsteps (modinv.h; s is public and in [1, N) for a live lane), VALU
    // code (per-lane data), ~38 us for a wave -- instead of the batched
    // chain's five launches and ~100 us of dependent latency
    uint32_t sw[8], iw[8];
    load_be256(sw, A.s + 32 * i);
    if (!modinv_n_var(iw, sw)) {
#pragma unroll
      for (int k = 0; k < 8; k++) iw[k] = 0;  // not reachable: 0 < s < N
    }
    fe_from_words(w, iw);
    fn_to_mont(w, w);  // s^-1 R
  }
  fe_from_words(e, ew);
  fe_from_words(r, rw);
  scalars(U1, U2, e, r, w);
}

// The accept test of item i (x_matches_r, scalar_dev.h) on the accumulator's
// X and ZZ; r from the batch, or from the caller's words.
MBFT_DEV void verify_finish(const VerifyArgs& A, long i, const fe& X, const fe& ZZ,
                           const uint32_t* rw_in = nullptr) {
  uint32_t rw[8];
  if (rw_in) {
#pragma unroll
    for (int k = 0; k < 8; k++) rw[k] = rw_in[k];
  } else {
    load_be256(rw, A.r + 32 * i);
  }
  A.status[i] = x_matches_r(X, ZZ, rw) ? ST_ACCEPT : ST_REJECT;
}

// The ending of the paths that sum with complete additions (verify_exact,
// verify_ladder_item): a final infinity rejects, as Go's (0, 0) does, else the
// accept test on X and ZZ = Z^2.
MBFT_DEV void verify_finish_jac(const VerifyArgs& A, long i, const jac& j, bool inf) {
  if (inf) {
    A.status[i] = ST_REJECT;  // (x, y) = (0, 0) -> false
    return;
  }
  fe ZZ;
  fe_sqr(ZZ, j.Z);
  verify_finish(A, i, j.X, ZZ);
}

// The exact path for item i: both phases recomputed with complete additions
// (doubling, infinity).
MBFT_DEV void verify_exact(const VerifyArgs& A, long i) {
  KeyDesc kd = A.keys[A.slot[i]];
  uint32_t U1[8], U2[8];
  if (A.winv)
    load_scalars<false>(A, i, U1, U2);
  else
    load_scalars<true>(A, i, U1, U2);
  bool inf = true;
  jac j;
  comb_complete(j, inf, U1, A.tabG, A.wg);
  comb_complete(j, inf, U2, kd.tab, (int)kd.wbits);
  verify_finish_jac(A, i, j, inf);
}

// Item i under a table-free key (KeyDesc.wbits == 0: `tab` is the point
// itself, one comb entry) or a compact key (wbits kTeethFlag | t: `tab` is
// its 2^t entries): u2 Q by the ladder (ladder_dev.h) or by the doubling comb
// (teeth_dev.h), then u1 G's
// comb entries added to it one by one with complete additions -- every join
// case (u1 G == +-u2 Q, the keys Q == +-G, u1 == 0) is exact, and the G side
// is ~4 % of the item's work.  r, s in range and the key valid (the caller
// checked).
template <bool LANE_INV>
MBFT_DEV void verify_ladder_item(const VerifyArgs& A, long i) {
  const KeyDesc kd = A.keys[A.slot[i]];
  uint32_t U1[8], U2[8];
  load_scalars<LANE_INV>(A, i, U1, U2);
  bool inf = true;
  jac j;
  // by the key's class: a compact key's doubling comb over its own small
  // table (teeth_dev.h; signed or not, one body), else the ladder over the
  // point.  A wave that holds both classes runs both bodies in turn
  // (DESIGN.md §4.8).
  if (kd.wbits >= kTeethFlag) {
    teeth_mul(j, inf, U2, kd.tab, (int)(kd.wbits & 0xFFu), (kd.wbits & kSignedTeethFlag) != 0u);
  } else {
    fe qx, qy;
    load_point(qx, qy, reinterpret_cast<const uint4*>(kd.tab));
    ladder_mul(j, inf, U2, qx, qy);
  }
  comb_complete(j, inf, U1, A.tabG, A.wg);
  verify_finish_jac(A, i, j, inf);
}

// (the small-batch forms: s^-1 from the planes where the batch has them)
MBFT_DEV void verify_ladder_inline(const VerifyArgs& A, long i) {
  if (A.winv)
    verify_ladder_item<false>(A, i);
  else
    verify_ladder_item<true>(A, i);
}

// What every form settles about an item before any curve arithmetic.
// crypto/ecdsa.Verify rejects r <= 0 || s <= 0 || r >= N || s >= N.  An
// unknown slot or a key that failed validation is BAD_KEY, except that slots
// >= kHostSlot carry a status the host decided (batch pipeline), written as
// is, so the statuses the host reads back are final.  A key of a class the
// comb does not serve (key_class_queued) is `tfree`: never live; the form runs
// the ladder for it (verify_ladder_inline) or, in k_verify, queues it.
// An item that is not `live` is dead: past the end of the batch (in_batch
// false: the caller passes item 0), bad key, bad range or tfree.  Dead lanes
// still run their form's comb -- the cooperative gather needs all 64 lanes,
// the lane pairs and quads their shuffles -- on zero scalars over a valid
// table (kd defaults to the generator's) and write only dead_status: k_verify
// BEFORE the comb, so that nothing of a dead lane stays live across it.
struct Admission {
  uint32_t rw[8], sw[8];
  uint32_t slot;
  KeyDesc kd;
  bool range_ok, key_ok, tfree, live;
  uint8_t dead_status;
};

MBFT_DEV void admit(Admission& a, const VerifyArgs& A, long ii, bool in_batch) {
  load_be256(a.rw, A.r + 32 * ii);
  load_be256(a.sw, A.s + 32 * ii);
  a.slot = A.slot[ii];
  a.range_ok = !words_is_zero(a.rw) && words_lt(a.rw, kNw) &&
               !words_is_zero(a.sw) && words_lt(a.sw, kNw);
  a.kd = KeyDesc{A.tabG, (uint32_t)A.wg, 0u};
  if (a.slot < A.nslots) a.kd = A.keys[a.slot];
  a.key_ok = a.slot < A.nslots && a.kd.valid;
  a.dead_status = a.key_ok ? ST_REJECT
                           : ((A.host_status & kArgHostStatus) && a.slot >= kHostSlot ? (uint8_t)a.slot : ST_BAD_KEY);
  a.tfree = a.key_ok && key_class_queued(a.kd.wbits);
  a.live = in_batch && a.key_ok && a.range_ok && !a.tfree;
}

// Item index i appended to a compacted queue by every lane that calls this
// together: one atomic per wave.
MBFT_DEV void queue_push(uint32_t* count, uint32_t* queue, long i) {
  const uint64_t qm = __ballot(true);
  const int nq = __popcll(qm);
  const int rank = __popcll(qm & ((1ull << __lane_id()) - 1ull));
  const int leader = __ffsll((unsigned long long)qm) - 1;
  uint32_t base = 0;
  if (__lane_id() == leader) base = atomicAdd(count, (uint32_t)nq);
  base = __shfl(base, leader);
  queue[base + rank] = (uint32_t)i;
}

// One item per thread.  Every lane of the wave runs the comb loop (the
// cooperative gather needs all 64): lanes past the end of the batch, with an
// unknown / invalid key, or with r or s out of range are "dead" -- they run
// the loop on zero scalars over a valid table and write only their status.
// (admit's rules, open-coded: through the helper k_verify's register
// allocation moved and the large batches measured 0.7 % slower)

// G's first two windows on ONE lane (per-lane loads; comb_verify_fast gathers
// its own cooperatively): affine + affine, zero digits exact.  Leaves U and
// carry at window 2.
MBFT_DEV void comb_start_affine(chud& acc, bool& inf, bool& yneg, uint32_t (&U)[8], uint32_t& carry,
                                const uint32_t* tab, int W) {
  bool neg0, zero0, neg1, zero1;
  const uint32_t i0 = comb_digit(U[0], carry, W, false, neg0, zero0);
  shr_words(U, W);
  const uint32_t i1 = comb_digit(U[0], carry, W, false, neg1, zero1);
  shr_words(U, W);
  fe x0, y0, x1, y1;
  load_point(x0, y0, comb_entry(tab, W, 0, i0));
  load_point(x1, y1, comb_entry(tab, W, 1, i1));
  ec_add_affine_chud(acc, x0, y0, x1, y1, neg0 != neg1);
  yneg = !neg0;
  inf = zero0 && zero1;
  if (zero0 != zero1) {
    acc.X = zero0 ? x1 : x0;
    acc.Y = zero0 ? y1 : y0;
    fe_one_mont(acc.ZZ);
    fe_one_mont(acc.ZZZ);
    yneg = zero0 ? neg1 : neg0;
  }
}

// o = the sum held by the lane at distance `mask` (lane id xor mask)
MBFT_DEV void chud_shfl_xor(chud& o, const chud& a, int mask) {
#pragma unroll
  for (int k = 0; k < NL; k++) {
    o.X.v[k] = __shfl_xor(a.X.v[k], mask);
    o.Y.v[k] = __shfl_xor(a.Y.v[k], mask);
    o.ZZ.v[k] = __shfl_xor(a.ZZ.v[k], mask);
    o.ZZZ.v[k] = __shfl_xor(a.ZZZ.v[k], mask);
  }
}

// The ending of a dead item on its first lane, after the comb: a tfree key's
// item by the ladder, else the status admit chose.
MBFT_DEV void verify_dead(const VerifyArgs& A, long i, bool in_batch, const Admission& ad) {
  if (in_batch && ad.tfree && ad.range_ok)
    verify_ladder_inline(A, i);
  else if (in_batch)
    A.status[i] = ad.dead_status;
}

// The ending of a live item: u1 G (acc, inf) and u2 Q (o, oinf) joined by the
// x-only addition, then the accept test.  same_sign: ecc.h's Y convention
// agrees between the two.  u1 G == +-u2 Q (the join fails, or leaves ZZ == 0)
// takes the exact path.
MBFT_DEV void verify_join(const VerifyArgs& A, long i, const chud& acc, bool inf, const chud& o, bool oinf,
                          bool same_sign) {
  fe X, ZZ;
  if (inf && oinf) {
    A.status[i] = ST_REJECT;  // infinity: (x, y) = (0, 0) -> false
    return;
  }
  if (inf || oinf) {
    X = inf ? o.X : acc.X;
    ZZ = inf ? o.ZZ : acc.ZZ;
  } else if (!ec_add_chud_x(X, ZZ, acc, o, same_sign)) {
    verify_exact(A, i);
    return;
  }
  fe zc = ZZ;
  fe_canon(zc);
  if (fe_is_zero_canon(zc)) {
    verify_exact(A, i);
    return;
  }
  verify_finish(A, i, X, ZZ);
}
