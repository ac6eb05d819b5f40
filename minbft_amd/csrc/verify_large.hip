// The verifier's large-batch form and what serves its queues: k_verify (one
// item per lane, cooperative gathers; verify_one), k_verify_slow (the exact
// path's queue, as lane pairs), k_verify_ladder (the table-free and compact
// keys' queue) and k_verify_keys (keys given with the call).  Also the
// dispatch of every form, mbft_launch::verify: it launches the kernels of this
// unit and calls the other units' launchers (verify_launch.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"
#include "pair_dev.h"
#include "verify_dev.h"
#include "verify_launch.h"

using namespace mbft;

#ifdef MBFT_STEP_TIMING
// Comb-step stamps (timing builds only: tools/step_timing.py, built with
// -DMBFT_STEP_TIMING): per wave, shader-clock cycles (s_memtime) summed over
// its cooperative comb steps in k_verify: [0] waiting for the entry
// prefetched one step earlier (vmcnt), [1] reading it from LDS, [2] issuing
// the next gather (address exchange by ds_bpermute, 4 LDS-DMA loads), [3]
// the mixed addition (its VALU issue, dependency stalls, and the cycles the
// SIMD gives the other waves); [4] steps, [5] waves; [6] / [7] the comb's
// span in shader cycles / in 100 MHz wall-clock ticks (their ratio: the
// in-kernel clock), [8] the whole verify_one in shader cycles, [9] its part
// before the comb.  The stamps themselves cost cycles (each waits for the
// LDS / SMEM queue); compare the timing build's step with the normal one.
__device__ unsigned long long g_step_clk[12];
extern "C" int mbft_debug_step_timing(unsigned long long out[12], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_clk), sizeof(g_step_clk)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_step_clk), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// One item per thread.  Every lane of the wave runs the comb loop (the
// cooperative gather needs all 64): lanes past the end of the batch, with an
// unknown / invalid key, or with r or s out of range are "dead" -- they run
// the loop on zero scalars over a valid table and write only their status.
// (admit's rules, open-coded: through the helper k_verify's register
// allocation moved and the large batches measured 0.7 % slower)
MBFT_DEV void verify_one(const VerifyArgs& A, long i, bool in_batch, uint4* buf) {
#ifdef MBFT_STEP_TIMING
  const unsigned long long tv0 = __builtin_amdgcn_s_memtime();
#endif
  const long ii = in_batch ? i : 0;  // lanes past the end read item 0
  uint32_t rw[8], sw[8];
  load_be256(rw, A.r + 32 * ii);
  load_be256(sw, A.s + 32 * ii);
  const uint32_t slot = A.slot[ii];

  // crypto/ecdsa.Verify: r <= 0 || s <= 0 || r >= N || s >= N -> false
  const bool range_ok = !words_is_zero(rw) && words_lt(rw, kNw) &&
                        !words_is_zero(sw) && words_lt(sw, kNw);
  KeyDesc kd{A.tabG, (uint32_t)A.wg, 0u};
  if (slot < A.nslots) kd = A.keys[slot];
  const bool key_ok = slot < A.nslots && kd.valid;
  // slots >= kHostSlot carry a status the host decided (batch pipeline):
  // written as is, so the statuses the host reads back are final
  // a table-free key (window 0): not live for the comb; its index goes to the
  // second compacted queue, which k_verify_ladder serves (one atomic per
  // wave) and whose status is that kernel's to write (kNoStatus here)
  constexpr uint8_t kNoStatus = 0xFF;
  const bool tfree = key_ok && key_class_queued(kd.wbits);
  const bool queued = tfree && in_batch && range_ok && (A.host_status & kArgTableFree);
  const uint8_t dead_status =
      queued ? kNoStatus
             : key_ok ? ST_REJECT : ((A.host_status & kArgHostStatus) && slot >= kHostSlot ? (uint8_t)slot : ST_BAD_KEY);
  const bool live = in_batch && key_ok && range_ok && !tfree;
  if (queued) {
    queue_push(ladder_count(A), ladder_queue(A), i);
  }

  // w = s^-1 (Montgomery form), u1 = e w, u2 = r w (plain, canonical < N).
  // e, r, w are not kept live across the comb (register pressure): the rare
  // slow path and the final check reload them.
  uint32_t U1[8], U2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) U1[j] = U2[j] = 0u;
  if (live) load_scalars<false>(A, ii, U1, U2);
  const uint32_t* tq = kd.tab;
  int wq = (int)kd.wbits;

  // Dead lanes adopt the first live lane's key table; the Q phase gathers
  // cooperatively when every lane then has the same key window.
  // (a dead lane's status is written here, before the comb, so that nothing
  // of it stays live across the comb)
  if (!live && in_batch && dead_status != kNoStatus) A.status[i] = dead_status;
  const uint64_t lm = __ballot(live);
  if (lm == 0) return;
  const int first = __ffsll((unsigned long long)lm) - 1;
  const uint64_t tq64 = reinterpret_cast<uint64_t>(tq);
  const uint32_t tlo = __builtin_amdgcn_readlane((uint32_t)tq64, first);
  const uint32_t thi = __builtin_amdgcn_readlane((uint32_t)(tq64 >> 32), first);
  const int wq_u = __builtin_amdgcn_readlane(wq, first);
  if (!live) {
    tq = reinterpret_cast<const uint32_t*>(((uint64_t)thi << 32) | tlo);
    wq = wq_u;
  }
  const bool quni = __ballot(wq != wq_u) == 0;

  chud acc;
  const Spill sp{A.scr, blockIdx.x * blockDim.x + threadIdx.x, A.sstride};
  StepClock sc;
#ifdef MBFT_STEP_TIMING
  const unsigned long long tc0 = __builtin_amdgcn_s_memtime(), rc0 = __builtin_amdgcn_s_memrealtime();
#endif
  const bool inf = !quni ? comb_verify_fast<false>(acc, U1, U2, A.tabG, A.wg, tq, wq, buf, sp, live, sc)
                         : comb_verify_fast<true>(acc, U1, U2, A.tabG, A.wg, tq, wq, buf, sp, live, sc);
#ifdef MBFT_STEP_TIMING
  const unsigned long long tc1 = __builtin_amdgcn_s_memtime(), rc1 = __builtin_amdgcn_s_memrealtime();
  if (__lane_id() == 0) {
    for (int k = 0; k < 4; k++) atomicAdd(&g_step_clk[k], sc.s[k]);
    atomicAdd(&g_step_clk[4], sc.steps);
    atomicAdd(&g_step_clk[5], 1ull);
    atomicAdd(&g_step_clk[6], tc1 - tc0);
    atomicAdd(&g_step_clk[7], rc1 - rc0);
    atomicAdd(&g_step_clk[9], tc0 - tv0);
  }
  struct End {
    unsigned long long t0;
    __device__ ~End() {
      if (__lane_id() == 0) atomicAdd(&g_step_clk[8], __builtin_amdgcn_s_memtime() - t0);
    }
  } end_stamp{tv0};
#endif
  if (!live) return;
  if (inf) {
    A.status[i] = ST_REJECT;  // u1 G + u2 Q = infinity: (x, y) = (0, 0) -> false
    return;
  }

  fe zc = acc.ZZ;
  fe_canon(zc);
  if (fe_is_zero_canon(zc)) {
    // The exact path (a degenerate addition: acc == +-entry in the Q phase,
    // constructible only with the key's discrete log) is deferred to
    // k_verify_slow over a compacted queue, so that a crafted item costs its
    // own exact recomputation only -- not a stall of the 63 other lanes of
    // its wave.  One atomic per wave.
    queue_push(A.slown, A.slowq, i);
    return;
  }
  verify_finish(A, i, acc.X, acc.ZZ);
}

// The exact path for the items k_verify queued: both phases recomputed with
// complete additions (doubling, infinity), one item per thread, grid-stride
// over the queue (its length is known only on the device).  A final
// infinity rejects, as Go's (0, 0) does.
//
// The queued items run as G / Q lane pairs (verify_pair): a degenerate
// addition can only happen where the two single-scalar sums meet, so the
// fast mixed addition serves both halves and only a degenerate join takes
// the complete formulas (verify_exact).  s^-1 from the batched planes.
__global__ void __launch_bounds__(256, 2) k_verify_slow(VerifyArgs A) {
  __shared__ uint4 coop[4][256];  // per wave: 64 lanes x 64 B (per-lane gathers)
  uint4* buf = coop[threadIdx.x >> 6];
  const Spill sp{A.scr, blockIdx.x * blockDim.x + threadIdx.x, A.sstride};
  const long nq = (long)*A.slown;
  const long stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < 2 * nq; base += stride) {
    const long t = base + threadIdx.x, q = t >> 1;
    const bool in = q < nq;
    verify_pair<false>(A, in ? (long)A.slowq[q] : 0, (int)(t & 1), in, buf, sp);
  }
}

// The items k_verify queued for their table-free keys (window 0): one item
// per lane, grid-stride over the second compacted queue (its length is known
// only on the device; an empty queue ends the kernel at once).  u2 Q by the
// double-and-add ladder, s^-1 from the batch's planes, u1 G added with
// complete additions (verify_ladder_item).  Not served as G / Q lane pairs:
// the G half is a few percent of an item's work, and the pair would idle
// half the lanes.
__global__ void __launch_bounds__(256, 2) k_verify_ladder(VerifyArgs A) {
  long nq = (long)*ladder_count(A);
  if (nq > A.n) nq = A.n;  // (the queue holds n entries)
  const long stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride)
    verify_ladder_item<false>(A, (long)ladder_queue(A)[q]);
}

// The inline-key class (mbft_verify_prehashed_keys*): the key
// arrives beside the signature, no slot, no KeyDesc, nothing of the key store.
// Its own argument block -- VerifyArgs stays what it is.
struct KeysArgs {
  const uint8_t* e;        // n x 32 B big-endian
  const uint8_t* r;
  const uint8_t* s;
  const uint8_t* xy;       // n x 64 B big-endian X || Y (crypto/ecdsa.Verify's pub, per item)
  const uint32_t* winv;    // s^-1 R mod N, 9 planes of n (LANE_INV false), else null
  const uint32_t* tabG;    // generator comb table (window wg)
  int wg;
  long n;
  uint8_t* status;
};

// One item per lane, grid-stride, no LDS, no queue.  Per item: r, s in
// [1, N); X, Y < p and Y^2 == X^3 - 3 X + b (k_check_points' field
// operations, on the batch's own bytes); a dead item's status at once, a bad
// key before a bad range (admit's precedence); else u2 Q by the ladder over
// the validated point and u1 G's comb entries added with complete additions,
// exactly verify_ladder_item's sum.  Lanes past n touch nothing.
template <bool LANE_INV>
__global__ void __launch_bounds__(256, 2) k_verify_keys(KeysArgs K) {
  // what load_scalars and verify_finish_jac read of a batch
  VerifyArgs A{};
  A.e = K.e;
  A.r = K.r;
  A.s = K.s;
  A.winv = K.winv;
  A.n = K.n;
  A.status = K.status;
  const long stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < K.n; i += stride) {
    fe qx, qy;
    bool key_ok, range_ok;
    {
      uint32_t rw[8], sw[8], wx[8], wy[8];
      load_be256(rw, K.r + 32 * i);
      load_be256(sw, K.s + 32 * i);
      load_be256(wx, K.xy + 64 * i);
      load_be256(wy, K.xy + 64 * i + 32);
      range_ok = !words_is_zero(rw) && words_lt(rw, kNw) && !words_is_zero(sw) && words_lt(sw, kNw);
      const bool in_range = words_lt(wx, kPw) && words_lt(wy, kPw);
      fe b, t, lhs, rhs;
      fe_from_words(qx, wx);
      fe_from_words(qy, wy);
      fe_from_words(b, kBw);
      fe_to_mont(qx, qx);
      fe_to_mont(qy, qy);
      fe_to_mont(b, b);
      fe_sqr(lhs, qy);
      fe_sqr(t, qx);
      fe_mul(t, t, qx);               // x^3
      fe_mulsmall(rhs, qx, 3);
      fe_sub(rhs, t, rhs);            // x^3 - 3x
      fe_add(rhs, rhs, b);
      fe_canon(lhs);
      fe_canon(rhs);
      key_ok = in_range && fe_eq_canon(lhs, rhs);
    }
    if (!key_ok || !range_ok) {
      K.status[i] = key_ok ? ST_REJECT : ST_BAD_KEY;
      continue;
    }
    fe_canon(qx);  // canonical Montgomery: what a table-free key's entry holds (k_point_entries)
    fe_canon(qy);
    uint32_t U1[8], U2[8];
    load_scalars<LANE_INV>(A, i, U1, U2);
    bool inf = true;
    jac j;
    ladder_mul(j, inf, U2, qx, qy);
    comb_complete(j, inf, U1, K.tabG, K.wg);
    verify_finish_jac(A, i, j, inf);
  }
}

#ifdef MBFT_CLOCK_STAMP
// Clock builds only (tools/ab_build_def.sh clk "-DMBFT_CLOCK_STAMP"): per
// k_verify workgroup, shader cycles (s_memtime) and 100 MHz wall ticks
// (s_memrealtime) from its start to its end, summed: their ratio x 100 MHz is
// the in-kernel clock over the launches since the last reset
// (tools/clock_stamp_probe.py).  Stamps go to this buffer alone.
__device__ unsigned long long g_vclk[3];
extern "C" int mbft_debug_verify_clock(double out[3], int reset) {
  unsigned long long h[3];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_vclk), sizeof(h)) != hipSuccess) return -1;
  for (int k = 0; k < 3; k++) out[k] = (double)h[k];
  if (reset) {
    const unsigned long long z[3] = {0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_vclk), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// Grid-stride over items: the default grid has one 256-item block per 256
// items; a capped grid (MBFT_VERIFY_BPC blocks per CU) leaves wave slots
// free so the next batch's s^-1 kernels run concurrently.
template <int MINW>
__global__ void __launch_bounds__(256, MINW) k_verify(VerifyArgs A) {
#ifdef MBFT_CLOCK_STAMP
  unsigned long long clk0 = 0, rt0 = 0;
  if (threadIdx.x == 0) {
    clk0 = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  __shared__ uint4 coop[4][256];  // per wave: one slot of 64 entries x 64 B (gather_issue)
  uint4* buf = coop[threadIdx.x >> 6];
  const long stride = (long)gridDim.x * blockDim.x;
  // block-uniform loop: all lanes of a wave take part in every step
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < A.n; base += stride) {
    const long i = base + threadIdx.x;
    verify_one(A, i, i < A.n, buf);
  }
#ifdef MBFT_CLOCK_STAMP
  if (threadIdx.x == 0) {
    const unsigned long long clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
    atomicAdd(&g_vclk[0], clk1 - clk0);
    atomicAdd(&g_vclk[1], rt1 - rt0);
    atomicAdd(&g_vclk[2], 1ull);
  }
#endif
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h and verify_launch.h)
namespace mbft_launch {

int device_cus() {
  static const int ncu = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess)
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
  }();
  return ncu;
}

// The launches of one batch, as its plan says (verify_plan.h; the measurements
// behind the small forms: profiles/round6_planes_ab.json, round6_quads_ab.json,
// round6_quads_inline_ab.json).
hipError_t verify(const VerifyBatch& b, const VerifyTables& t, const VerifyPlan& plan, hipStream_t st) {
  const long n = b.n;
  if (n <= 0) return hipSuccess;
  VerifyArgs A{b.e, b.r, b.s, b.slot, nullptr, t.tabG, t.keys, t.nslots, t.wg, n, b.status, b.slowq, b.slowq + n,
               b.host_status ? kArgHostStatus : 0u, b.slowq + verify_scratch_offset(n), 0u, b.ndev};
  const long blocks = (plan.threads + 255) / 256;
  if (!verify_form_split(plan.form)) A.sstride = (uint32_t)(blocks * 256);
  if (plan.ninv_first) {
    hipError_t e0 = batch_inverse_s_small(b.s, n, b.planes_ws, b.ndev, st);
    if (e0 != hipSuccess) return e0;
    A.winv = b.planes_ws;
  }
  const dim3 grid((unsigned)blocks), block(256);
  switch (plan.form) {
    case VerifyForm::kSplitHost:
      A.winv = b.winv;
      A.uhost = b.winv + 9 * n;
      [[fallthrough]];
    case VerifyForm::kSplitWave:
      verify_split(A, st);
      break;
    case VerifyForm::kQuadsInline:
      verify_quads(A, true, grid, st);
      break;
    case VerifyForm::kQuadsHost:
      A.winv = b.winv;
      [[fallthrough]];
    case VerifyForm::kQuadsPlanes:
      verify_quads(A, false, grid, st);
      break;
    case VerifyForm::kPairsPlanes:
      verify_pairs(A, false, grid, st);
      break;
    case VerifyForm::kPairsLane:
      verify_pairs(A, true, grid, st);
      break;
    case VerifyForm::kLarge: {
      A.winv = b.winv;
      if (t.table_free) {
        if (plan.queue_reset) {
          hipError_t me = hipMemsetAsync(b.slowq + n + 1, 0, 4, st);
          if (me != hipSuccess) return me;
        }
        A.host_status |= kArgTableFree;
      }
      static const int bpc = (int)env_long("MBFT_VERIFY_BPC", 0);
      const long ncu = device_cus();
      const long vblocks = verify_large_blocks(blocks, bpc, ncu);
      A.sstride = (uint32_t)(vblocks * 256);
      // MINW = 3 waves/SIMD (the trace summaries under profiles/ name k_verify<3>)
      hipLaunchKernelGGL((k_verify<3>), dim3((unsigned)vblocks), block, 0, st, A);
      // the queued items: a grid of up to kSlowBpc blocks per CU (one wave per
      // SIMD) that exits at once when the queue is empty; its threads index
      // the same spill planes (A.sstride): verify_slow_blocks keeps it inside them
      const long sblocks = verify_slow_blocks(blocks, vblocks, ncu);
      hipLaunchKernelGGL(k_verify_slow, dim3((unsigned)sblocks), block, 0, st, A);
      // the table-free items: two blocks per CU at the most (the kernel's
      // occupancy), grid-stride over the queue
      if (t.table_free) {
        const long lblocks = verify_ladder_blocks(blocks, ncu);
        hipLaunchKernelGGL(k_verify_ladder, dim3((unsigned)lblocks), block, 0, st, A);
      }
      break;
    }
  }
  if (plan.account) {
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return le;
    return key_account(KeyAccount{b.slot, b.status, n, b.ndev, t.keys, t.nslots, t.uses, t.rejects}, st);
  }
  return hipGetLastError();
}

// The inline-key form, as its plan says (verify_plan.h, verify_keys_plan).
hipError_t verify_keys(const KeysBatch& b, const uint32_t* tabG, int wg, const mbft::KeysPlan& plan, hipStream_t st) {
  if (b.n <= 0) return hipSuccess;
  if (plan.blocks <= 0 || (!plan.lane_inv && !b.winv)) return hipErrorInvalidValue;
  const KeysArgs K{b.e, b.r, b.s, b.xy, plan.lane_inv ? nullptr : b.winv, tabG, wg, b.n, b.status};
  const dim3 grid((unsigned)plan.blocks), block(256);
  if (plan.lane_inv)
    hipLaunchKernelGGL(k_verify_keys<true>, grid, block, 0, st, K);
  else
    hipLaunchKernelGGL(k_verify_keys<false>, grid, block, 0, st, K);
  return hipGetLastError();
}

}  // namespace mbft_launch
