// The verifier's mid-size form, one item per lane quad: verify_quad,
// k_verify_quads and its launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify_dev.h"
#include "verify_launch.h"

using namespace mbft;

// Mid-size batches (k_verify_quads): one item per lane QUAD, s^-1 from the
// batched planes.  Lane q of the quad sums one half of one scalar's comb
// windows: q = 0 G windows [0, mid) (the first two affine + affine), 1 G
// [mid, S), 2 Q [0, mid), 3 Q [mid, S) -- per-lane table, window and range,
// per-lane gathers -- so an item's latency is ~half a scalar's additions
// (4 of 9 at W = 29) plus two joins, against 8 additions plus one join per
// lane pair (verify_pair).  The halves of one scalar join by a full
// Chudnovsky addition on lanes 0 and 2 (never degenerate: with u = a + b the
// low and high parts of a scalar in [1, N), a == -b mod N is u == 0, and a ==
// b mod N needs u = 2 a + N with a the low part of u itself, which no window
// size admits -- tests/test_quad_joins.py checks it for W = 4..29; a zero part
// is infinity, flagged), then G and Q by the x-only addition on lane 0 (u1 G
// == +-u2 Q takes the exact path, as in verify_pair).  Neither half of a range
// degenerates: every partial sum of a range is a multiple of 2^(W lo), smaller
// in magnitude than the next addend (verify_pair's argument).
// INLINE: s^-1 by the wave itself instead of the planes -- k_ninv_local's
// arithmetic with chains of one item over the wave's 16 quads (a butterfly at
// lane distances 4 .. 32, ONE wave-cooperative inversion, the butterfly back),
// so no separate launch and no planes round trip.
template <bool INLINE>
MBFT_DEV void verify_quad(const VerifyArgs& A, long i, int q, bool in_batch, uint4* buf, const Spill& sp) {
  const long ii = in_batch ? i : 0;
  Admission ad;
  admit(ad, A, ii, in_batch);  // (a tfree item: its first lane runs the ladder at the end)
  const KeyDesc& kd = ad.kd;
  const uint32_t(&sw)[8] = ad.sw;
  const bool live = ad.live;
  uint32_t U1[8], U2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) U1[j] = U2[j] = 0u;
  if (INLINE) {
    // every lane of the wave (dead ones carry 1: Montgomery's trick stays
    // consistent and nothing of theirs is used)
    fe v;
    fe_from_words(v, sw);
    if (!live) {
      fe_zero(v);
      v.v[0] = 1;
    }
    fe acc;
    fe_set(acc, kRN);  // Montgomery one
    fn_mul(acc, acc, v);
    fe sib[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int k = 0; k < NL; k++) sib[j].v[k] = __shfl_xor(acc.v[k], 4 << j);
      fn_mul(acc, acc, sib[j]);
    }
    fe r = acc;
    fn_canon(r);
    uint32_t w[8], iw[8];
    fe_to_words(w, r);
    if (!modinv_n_var_wave(iw, w)) {
#pragma unroll
      for (int k = 0; k < 8; k++) iw[k] = 0;  // not reachable: every value is in [1, N)
    }
    fe_from_words(r, iw);
    fn_to_mont(r, r);
#pragma unroll
    for (int j = 3; j >= 0; j--) fn_mul(r, r, sib[j]);  // this quad's s^-1 R
    if (live) load_scalars<true>(A, ii, U1, U2, &r);
  } else if (live) {
    load_scalars<false>(A, ii, U1, U2);
  }
  const bool qh = q >= 2, high = (q & 1) != 0;
  const uint32_t* tab = qh && live ? kd.tab : A.tabG;
  const int W = qh && live ? (int)kd.wbits : A.wg;
  const int S = (256 + W - 1) / W, mid = (S + 1) / 2;
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
  if (high) {
    // the recoding carry into window mid, U shifted to it
#pragma unroll 1
    for (int k = 0; k < mid; k++) {
      bool ng, zr;
      (void)comb_digit(U[0], carry, W, k + 1 >= S, ng, zr);
      shr_words(U, W);
    }
    step0 = mid;
  } else if (!qh) {
    comb_start_affine(acc, inf, yneg, U, carry, tab, W);
    step0 = 2;
  }
  StepClock sc;
  comb_run<false>(acc, inf, yneg, U, tab, W, step0, carry, buf, sp, live, sc, high ? -1 : mid);
  fe_norm_lazy(acc.ZZ);
  fe_norm_lazy(acc.ZZZ);
  if (!inf && yneg) fe_neg(acc.Y, acc.Y);  // the true Y from here on
  // level 1: lanes 0 / 2 take the high half from lanes 1 / 3
  chud o;
  chud_shfl_xor(o, acc, 1);
  const bool oinf = __shfl_xor(inf ? 1 : 0, 1) != 0;
  if (high) return;
  bool degen = false;
  if (!oinf) {
    if (inf) {
      acc = o;
      inf = false;
    } else {
      chud t;
      if (ec_add_chud_full(t, acc, o))
        acc = t;
      else
        degen = true;  // not reachable (above); the exact path if it were
    }
  }
  // level 2: lane 0 takes Q's sum from lane 2
  chud_shfl_xor(o, acc, 2);
  const bool qinf = __shfl_xor(inf ? 1 : 0, 2) != 0;
  const bool qdegen = __shfl_xor(degen ? 1 : 0, 2) != 0;
  if (qh) return;
  if (!live) {
    verify_dead(A, i, in_batch, ad);
    return;
  }
  if (degen || qdegen) {
    verify_exact(A, i);
    return;
  }
  verify_join(A, i, acc, inf, o, qinf, true);  // (both Ys true since level 1)
}

// One item per lane quad (verify_quad), s^-1 from the batched planes
// (A.winv) or, INLINE, by each wave; the item count n, or the device's when
// the grid was sized for an upper bound.
template <bool INLINE>
__global__ void __launch_bounds__(256, 2) k_verify_quads(VerifyArgs A) {
  __shared__ uint4 coop[4][256];  // per wave: 64 lanes x 64 B (per-lane gathers)
  uint4* buf = coop[threadIdx.x >> 6];
  const Spill sp{A.scr, blockIdx.x * blockDim.x + threadIdx.x, A.sstride};
  const long stride = (long)gridDim.x * blockDim.x;
  long n = A.n;
  if (A.ndev && (long)*A.ndev < n) n = (long)*A.ndev;
  const long wave0 = (long)(threadIdx.x & ~63u);
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < 4 * n; base += stride) {
    if (base + wave0 >= 4 * n) break;
    const long t = base + threadIdx.x;
    verify_quad<INLINE>(A, t >> 2, (int)(t & 3), (t >> 2) < n, buf, sp);
  }
}

namespace mbft_launch {

void verify_quads(const VerifyArgs& A, bool inline_inv, dim3 grid, hipStream_t st) {
  if (inline_inv)
    hipLaunchKernelGGL(k_verify_quads<true>, grid, dim3(256), 0, st, A);
  else
    hipLaunchKernelGGL(k_verify_quads<false>, grid, dim3(256), 0, st, A);
}

}  // namespace mbft_launch
