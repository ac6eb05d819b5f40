// Test-only: the verifier's launch plan (minbft_amd/csrc/verify_plan.h) on the
// HOST, so the CPU suite can check the form, the grid and the `slowq` size of
// every kind of batch, and the kLarge form's three grids
// (tests/test_verify_plan.py).  Built into
// tests/libverify_plan_check.so by __graft_entry__.build().
#include "../../minbft_amd/csrc/verify_plan.h"

extern "C" {

// out: form, threads, ninv_first, queue_reset, slowq words, scratch offset
// (words), spill threads.  host_planes / has_count / has_ws: 0 or 1.
void verify_plan_check(long n, unsigned long lane_inv_max, int host_planes, int has_count, int has_ws,
                       long split_max, int small_form, long out[7]) {
  const mbft::InvSource src = mbft::verify_inv_source(n, (size_t)lane_inv_max, host_planes != 0, has_count != 0);
  const mbft::VerifyPlan p = mbft::verify_plan(n, src, has_count != 0, has_ws != 0, split_max, small_form);
  out[0] = (long)p.form;
  out[1] = p.threads;
  out[2] = p.ninv_first;
  out[3] = p.queue_reset;
  out[4] = (long)mbft::verify_slowq_words(n, p);
  out[5] = (long)mbft::verify_scratch_offset(n);
  out[6] = (long)mbft::verify_spill_threads(p);
}

// The kLarge form's grids for a plan of `blocks` blocks under a MBFT_VERIFY_BPC
// of bpc (0: none) on ncu compute units.  out: k_verify's blocks, k_verify_slow's,
// k_verify_ladder's, then the constants kSlowBpc, kLadderBpc.
void verify_large_grids_check(long blocks, long bpc, long ncu, long out[5]) {
  const long vblocks = mbft::verify_large_blocks(blocks, bpc, ncu);
  out[0] = vblocks;
  out[1] = mbft::verify_slow_blocks(blocks, vblocks, ncu);
  out[2] = mbft::verify_ladder_blocks(blocks, ncu);
  out[3] = mbft::kSlowBpc;
  out[4] = mbft::kLadderBpc;
}

}  // extern "C"
