// The verifier's launch plan: the kernel form a batch takes, its grid and what
// runs before it, decided ONCE -- verify_device sizes the batch's `slowq`
// buffer from it and mbft_launch::verify launches it.  Plain C++, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mbft {

// The small-batch forms (all but kLarge) run the exact path and the table-free
// keys inline; kLarge queues both (k_verify_slow, k_verify_ladder).
enum class VerifyForm : int {
  kSplitHost,    // k_verify_split, one item per workgroup; s^-1 R and u1, u2 staged by the host
  kSplitWave,    // k_verify_split, every wave inverts s itself
  kQuadsInline,  // k_verify_quads<true>: one item per lane quad, s^-1 by each wave in the kernel
  kQuadsPlanes,  // k_ninv_local<1> into the planes workspace, then k_verify_quads<false>
  kQuadsHost,    // k_verify_quads<false> on the host's planes
  kPairsPlanes,  // k_ninv_local<1>, then k_verify_pairs<false>: one item per lane pair
  kPairsLane,    // k_verify_pairs<true>: s^-1 by each lane
  kLarge         // k_verify<3>, one item per lane, on the batch's planes
};
constexpr bool verify_form_split(VerifyForm f) { return f == VerifyForm::kSplitHost || f == VerifyForm::kSplitWave; }

// Where s^-1 comes from: the form itself, the batch's own s^-1 kernels
// (verify_device runs them first), the host's planes.
enum class InvSource : int { kNone, kBatch, kHost };

// has_count: n is an upper bound, the count is on the device -- the small-batch
// kernels only, which read it (a batched chain is sized by n on the host).
constexpr InvSource verify_inv_source(long n, size_t lane_inv_max, bool host_planes, bool has_count) {
  return host_planes ? InvSource::kHost
                     : ((size_t)n <= lane_inv_max || has_count) ? InvSource::kNone : InvSource::kBatch;
}

struct VerifyPlan {
  VerifyForm form;
  long threads;      // the grid's threads (256 a block); kLarge: before the MBFT_VERIFY_BPC cap
  bool ninv_first;   // k_ninv_local<1> into the planes workspace runs first
  bool queue_reset;  // a memset resets the table-free queue's counter in front of the kernel (where
                     // a key of that class exists; the exact-path queue's: the s^-1 kernels)
  bool account = false;  // k_key_account ends the batch: after the form's last kernel that writes a
                         // status (kLarge: after k_verify_slow and k_verify_ladder)
  bool memo = false;  // the batch is the misses of a memo pass (memo_plan.h): k_memo_probe ran in front
                      // of it over the original items and k_memo_commit follows it; the use-count
                      // stage then runs over the ORIGINAL items, after the commit, not here
};

// The per-key use counts (mbft_set_key_accounting): the stage is part of the
// plan, off unless the context asks for it.
constexpr VerifyPlan verify_plan_account(VerifyPlan p, bool accounting) {
  p.account = accounting;
  return p;
}
// The verified-call memo (mbft_set_verified_memo): likewise off unless the
// pass runs under one.  The plan of the misses never accounts itself.
constexpr VerifyPlan verify_plan_memo(VerifyPlan p, bool memo) {
  p.memo = memo;
  if (memo) p.account = false;
  return p;
}
// Its grid: one item per lane, 256 a block, grid-stride past kAccountBpc blocks
// per CU -- a wave carries its last slot's sums from one step to the next, so
// fewer, longer waves mean fewer atomics on a hot key's counters.
constexpr long kAccountBpc = 4;
constexpr long key_account_blocks(long n, long ncu) {
  return (n + 255) / 256 < ncu * kAccountBpc ? (n + 255) / 256 : ncu * kAccountBpc;
}

// split_max: 0 disables the split form.  small_form (0 .. 3,
// mbft_set_small_batch_inverse) is the form past it: 0 lane pairs inverting
// per lane, 1 lane pairs on planes, 2 lane quads inverting in the kernel, 3
// lane quads on planes; without a planes workspace only 0 is left.  Host
// planes past split_max (MBFT_HOST_INV_MAX above it) serve the lane quads;
// under small_form < 2 they are dropped.
constexpr VerifyPlan verify_plan(long n, InvSource src, bool has_count, bool has_planes_ws, long split_max,
                                 int small_form) {
  if (src == InvSource::kHost) {
    if (n <= split_max) return {VerifyForm::kSplitHost, 256 * n, false, false};
    if (small_form >= 2) return {VerifyForm::kQuadsHost, 4 * n, false, false};
    src = InvSource::kNone;
  }
  if (src == InvSource::kBatch && !has_count) return {VerifyForm::kLarge, n, false, true};
  if (src == InvSource::kNone) {
    if (n <= split_max) return {VerifyForm::kSplitWave, 256 * n, false, false};
    if (has_planes_ws && small_form == 2) return {VerifyForm::kQuadsInline, 4 * n, false, false};
    if (has_planes_ws && small_form == 3) return {VerifyForm::kQuadsPlanes, 4 * n, true, false};
    if (has_planes_ws && small_form != 0) return {VerifyForm::kPairsPlanes, 2 * n, true, false};
  }
  return {VerifyForm::kPairsLane, 2 * n, false, false};
}

// The kLarge form's three grids (mbft_launch::verify), in blocks of 256; every
// kernel strides over what its grid does not cover.  `blocks`: the plan's
// threads in whole blocks, ncu: the device's compute units.
// k_verify: one item per lane; bpc > 0 (MBFT_VERIFY_BPC) caps the grid at bpc
// blocks per CU.  Its threads are the spill planes' stride (VerifyArgs.sstride).
constexpr long verify_large_blocks(long blocks, long bpc, long ncu) {
  return bpc > 0 && blocks > bpc * ncu ? bpc * ncu : blocks;
}
// k_verify_slow: one queued item per lane pair, up to kSlowBpc blocks per CU
// (one wave per SIMD), never more than k_verify's grid (vblocks): its threads
// index the same spill planes.
constexpr long kSlowBpc = 4;
constexpr long verify_slow_blocks(long blocks, long vblocks, long ncu) {
  const long s = blocks < ncu * kSlowBpc ? blocks : ncu * kSlowBpc;
  return s > vblocks ? vblocks : s;
}
// k_verify_ladder: one queued item per lane, two blocks per CU at the most
// (the kernel's occupancy).
constexpr long kLadderBpc = 2;
constexpr long verify_ladder_blocks(long blocks, long ncu) {
  return blocks < ncu * kLadderBpc ? blocks : ncu * kLadderBpc;
}

// The inline-key form (k_verify_keys, mbft_verify_prehashed_keys*): one item
// per lane of 256-thread blocks, grid-stride past kKeysBpc blocks per CU -- the
// kernel's occupancy (2 waves a SIMD), as k_verify_ladder's grid.  s^-1 by the
// lane up to lane_inv_max items, from the batch's planes above (the rule of
// verify_inv_source: no host planes, no count on the device).  The host path
// sizes the planes from `lane_inv`, the launcher takes the rest.
constexpr long kKeysBpc = 2;
struct KeysPlan {
  bool lane_inv;  // k_verify_keys<true>: no planes, no s^-1 kernel in front
  long threads;   // one per item, whole blocks of 256
  long blocks;    // the grid: threads / 256, at most kKeysBpc per CU
};
constexpr KeysPlan verify_keys_plan(long n, size_t lane_inv_max, long ncu) {
  const long want = n <= 0 ? 0 : (n + 255) / 256;
  const long cap = (ncu < 1 ? 1 : ncu) * kKeysBpc;
  return {verify_inv_source(n, lane_inv_max, false, false) == InvSource::kNone, want * 256,
          want < cap ? want : cap};
}

// The P-384 class (k_verify_p384, mbft_verify_prehashed_p384_keys*; DESIGN.md
// §4.14): one item per lane of 256-thread blocks, grid-stride past kP384Bpc
// blocks per CU -- the kernel's occupancy (one wave a SIMD: the lane's three
// table points, the accumulator and a product's columns take more than half
// the register file).  s^-1 is always the lane's own.
constexpr long kP384Bpc = 1;
struct P384Plan {
  long threads;  // one per item, whole blocks of 256
  long blocks;   // the grid: threads / 256, at most kP384Bpc per CU
};
constexpr P384Plan verify_p384_plan(long n, long ncu) {
  const long want = n <= 0 ? 0 : (n + 255) / 256;
  const long cap = (ncu < 1 ? 1 : ncu) * kP384Bpc;
  return {want * 256, want < cap ? want : cap};
}

// `slowq`: the exact-path queue (n words), its length, the table-free queue's
// length (side by side), then (64-word aligned) the table-free queue (n
// words) and (64-word aligned) kSpillPlanes planes of one word per grid
// thread for the rare comb steps' spills.  Both queues are there for every
// form; the split forms spill nothing.
constexpr int kSpillPlanes = 36;
constexpr size_t ladder_queue_offset(long n) { return ((size_t)n + 2 + 63) & ~(size_t)63; }
constexpr size_t verify_scratch_offset(long n) { return (ladder_queue_offset(n) + (size_t)n + 63) & ~(size_t)63; }
constexpr size_t verify_spill_threads(const VerifyPlan& p) {
  return verify_form_split(p.form) ? 0 : ((size_t)p.threads + 255) & ~(size_t)255;
}
constexpr size_t verify_slowq_words(long n, const VerifyPlan& p) {
  return verify_scratch_offset(n) + (size_t)kSpillPlanes * verify_spill_threads(p);
}

}  // namespace mbft
