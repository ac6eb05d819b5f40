// One item per lane pair (verify_pair): the body of k_verify_pairs
// (verify_pairs.hip) and of the exact-path kernel k_verify_slow
// (verify_large.hip).
#pragma once
#include "verify_dev.h"

// Small batches (verify_device, n <= MBFT_LANE_INV_MAX): one item per LANE
// PAIR.  The even lane sums the G windows, the odd lane the Q windows, at the
// same time (the same comb loop with per-lane table, window and first step;
// per-lane gathers, as the halves read different tables), and one x-only
// Chudnovsky addition joins them on the even lane: an item's latency is the
// longer half (9 of the 17 additions at W = 29) plus one addition, not the
// whole chain.  Each half is a single-scalar comb, never degenerate (the
// G-phase argument); a degenerate join (u1 G == +-u2 Q) goes to
// the exact path inline.  s^-1 per lane (divsteps), no queue.
template <bool LANE_INV>
MBFT_DEV void verify_pair(const VerifyArgs& A, long i, int half, bool in_batch, uint4* buf,
                          const Spill& sp) {
  const long ii = in_batch ? i : 0;
  Admission ad;
  admit(ad, A, ii, in_batch);  // (a tfree item: its even lane runs the ladder at the end)
  const KeyDesc& kd = ad.kd;
  const uint32_t(&sw)[8] = ad.sw;
  const bool live = ad.live;
  uint32_t U1[8], U2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) U1[j] = U2[j] = 0u;
  if (LANE_INV) {
    // A wave holding ONE live item (a single VerifyMessageAuthenTag call):
    // its s^-1 by all 64 lanes together (modinv_n_var_wave, ~24 us) instead
    // of the pair's own per-lane divsteps (~38 us).  Wave-uniform: live
    // lanes come in pairs, so <= 2 live lanes is one item.
    const uint64_t lm = __ballot(live);
    if (lm != 0 && __popcll(lm) <= 2) {
      const int leader = __ffsll((unsigned long long)lm) - 1;
      uint32_t xs[8], iw[8];
#pragma unroll
      for (int j = 0; j < 8; j++) xs[j] = (uint32_t)__builtin_amdgcn_readlane((int)sw[j], leader);
      if (!modinv_n_var_wave(iw, xs)) {
#pragma unroll
        for (int k = 0; k < 8; k++) iw[k] = 0;  // not reachable: 0 < s < N for a live item
      }
      fe wv;
      fe_from_words(wv, iw);
      fn_to_mont(wv, wv);  // s^-1 R
      if (live) load_scalars<LANE_INV>(A, ii, U1, U2, &wv);
    } else if (live) {
      load_scalars<LANE_INV>(A, ii, U1, U2);
    }
  } else if (live) {
    load_scalars<LANE_INV>(A, ii, U1, U2);
  }
  // this lane's half (dead lanes sum zero scalars over the generator table)
  const bool qh = half != 0;
  const uint32_t* tab = qh && live ? kd.tab : A.tabG;
  const int W = qh && live ? (int)kd.wbits : A.wg;
  uint32_t U[8];
#pragma unroll
  for (int j = 0; j < 8; j++) U[j] = qh ? U2[j] : U1[j];
  chud acc;
  fe_zero(acc.X);
  fe_zero(acc.Y);
  fe_one_mont(acc.ZZ);
  fe_one_mont(acc.ZZZ);
  bool inf = true, yneg = false;
  uint32_t carry = 0;
  int step0 = 0;
  if (!qh) {
    comb_start_affine(acc, inf, yneg, U, carry, tab, W);
    step0 = 2;
  }
  StepClock sc;
  comb_run<false>(acc, inf, yneg, U, tab, W, step0, carry, buf, sp, live, sc);
  fe_norm_lazy(acc.ZZ);
  fe_norm_lazy(acc.ZZZ);
  // the odd lane's half to the even lane
  chud o;
  chud_shfl_xor(o, acc, 1);
  const bool oinf = __shfl_xor(inf ? 1 : 0, 1) != 0;
  const bool oyneg = __shfl_xor(yneg ? 1 : 0, 1) != 0;
  if (qh) return;
  if (!live) {
    verify_dead(A, i, in_batch, ad);
    return;
  }
  verify_join(A, i, acc, inf, o, oinf, yneg == oyneg);
}
