// One item per 256-thread workgroup (comb_range_uniform, split_item): the body
// of k_verify_split (verify_split.hip) and of the resident k_verify_server
// (verify_server.hip).
#pragma once
#include "verify_dev.h"

// The signed-digit comb sum of windows [lo, hi) of one scalar (U: its
// words shifted right by W lo, carry: the recoding carry into window lo),
// for k_verify_split: ONE item per wave (every lane holds the same values),
// so zero digits and infinity are plain (wave-uniform) branches.  The first
// two windows of the range are one affine + affine addition, the rest mixed
// additions on the Chudnovsky accumulator (ecc.h sign convention, fixed at
// the end: acc.Y is the TRUE Y).  A degenerate addition leaves ZZ == 0 (the
// caller checks).
// The range's table entries (up to kSplitPre windows) are fetched first, all
// at once -- lane 4 j + q loads quarter q of window lo + j's 64-B entry into
// the wave's LDS slice `pre` -- so the HBM (and TLB) latency of the random
// 64-B reads is paid once instead of once per addition; windows past
// kSplitPre (ranges of 19 to 32 windows: comb windows 4 to 7 split in two)
// load as they go.
// (timing builds, -DMBFT_SPLIT_TIMING: the stamps go to g_split_t and
// g_split_clk, verify_split.hip)
constexpr int kSplitPre = 16;
// WIDE: the lane-group parallel additions (ecc.h ec_*_wide: the same results).
// extra (the resident kernel's one-scalar form): a range of 3 or more
// windows leaves its last window's entry out of the sum and returns it as a
// point of its own (affine, ZZ = ZZZ = 1, the digit's sign applied; *extra_inf
// if the digit is zero) for the host to join -- no mixed addition after the
// first pair.
template <bool WIDE>
MBFT_DEV void comb_range_uniform(chud& acc, bool& inf, uint32_t (&U)[8], uint32_t carry,
                                 const uint32_t* tab, int W, int S, int lo, int hi, uint4* pre,
                                 chud* extra = nullptr, bool* extra_inf = nullptr) {
  {
    uint32_t V[8];
#pragma unroll
    for (int j = 0; j < 8; j++) V[j] = U[j];
    uint32_t cy = carry;
    const int slot = (int)(__lane_id() >> 2);
    const uint4* src = nullptr;
#pragma unroll 1
    for (int k = lo; k < hi && k < lo + kSplitPre; k++) {
      bool neg, zero;
      const uint32_t idx = comb_digit(V[0], cy, W, k + 1 >= S, neg, zero);
      shr_words(V, W);
      if (slot == k - lo && !zero) src = comb_entry(tab, W, k, idx) + (__lane_id() & 3);
    }
    if (src) pre[__lane_id()] = *src;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef MBFT_SPLIT_TIMING
    if (__lane_id() == 0 && blockIdx.x < 2) g_split_t[5 * blockIdx.x + (threadIdx.x >> 6)][9] = wall_clock64();
#endif
  }
  auto entry = [&](int k, uint32_t idx) -> const uint4* {
    return k - lo < kSplitPre ? pre + 4 * (k - lo) : comb_entry(tab, W, k, idx);
  };
  inf = true;
  bool yneg = false;
  int k = lo;
  const int last = hi;
  if (extra) {
    *extra_inf = true;
    if (hi - lo >= 3) hi--;  // the last window goes out on its own
  }
  if (hi - lo >= 2) {
    bool neg0, zero0, neg1, zero1;
    const uint32_t i0 = comb_digit(U[0], carry, W, lo + 1 >= S, neg0, zero0);
    shr_words(U, W);
    const uint32_t i1 = comb_digit(U[0], carry, W, lo + 2 >= S, neg1, zero1);
    shr_words(U, W);
    fe x0, y0, x1, y1;
    load_point(x0, y0, entry(lo, i0));
    load_point(x1, y1, entry(lo + 1, i1));
    if (!zero0 && !zero1) {
      if (WIDE)
        ec_add_affine_chud_wide(acc, x0, y0, x1, y1, neg0 != neg1);
      else
        ec_add_affine_chud(acc, x0, y0, x1, y1, neg0 != neg1);
      yneg = !neg0;
      inf = false;
    } else if (zero0 != zero1) {
      acc.X = zero0 ? x1 : x0;
      acc.Y = zero0 ? y1 : y0;
      fe_one_mont(acc.ZZ);
      fe_one_mont(acc.ZZZ);
      yneg = zero0 ? neg1 : neg0;
      inf = false;
    }
    k = lo + 2;
  }
#pragma unroll 1
  for (; k < hi; k++) {
    bool neg, zero;
    const uint32_t idx = comb_digit(U[0], carry, W, k + 1 >= S, neg, zero);
    shr_words(U, W);
    if (zero) continue;
    fe px, py;
    load_point(px, py, entry(k, idx));
    if (inf) {
      acc.X = px;
      acc.Y = py;
      fe_one_mont(acc.ZZ);
      fe_one_mont(acc.ZZZ);
      yneg = neg;
      inf = false;
    } else {
      if (WIDE)
        ec_madd_chud_wide(acc, acc, px, py, yneg != neg);
      else
        ec_madd_chud<false, false>(acc, acc, px, py, yneg != neg);
      yneg = neg;
    }
  }
  if (!inf && yneg) fe_neg(acc.Y, acc.Y);
  if (extra && hi < last) {
    bool neg, zero;
    const uint32_t idx = comb_digit(U[0], carry, W, hi + 1 >= S, neg, zero);
    if (!zero) {
      fe px, py;
      load_point(px, py, entry(hi, idx));
      extra->X = px;
      extra->Y = py;
      if (neg) fe_neg(extra->Y, extra->Y);
      fe_one_mont(extra->ZZ);
      fe_one_mont(extra->ZZZ);
      *extra_inf = false;
    }
  }
}

#ifdef MBFT_SPLIT_TIMING
// Phase timestamps of the last k_verify_split item (timing builds only,
// tools/split_timing.py): [wave][phase] wall clock (100 MHz), plus the shader
// clock at phases 0 and 7 of wave 0.
#define SPLIT_T(ph)                                                   \
  do {                                                                \
    if (lane == 0 && blockIdx.x < 2) g_split_t[5 * blockIdx.x + wave][ph] = wall_clock64(); \
  } while (0)
#else
#define SPLIT_T(ph) \
  do {              \
  } while (0)
#endif

// Item i of A on the whole 256-thread workgroup (k_verify_split, and the
// resident k_verify_server between mailbox posts): part / pre are the
// workgroup's LDS.  Every wave returns when its share is done; the status is
// written by wave 0 (or, for inputs rejected up front, thread 0).
// half (the resident kernel's two-workgroup form): -1 = both scalars here
// (waves 0, 1: G's windows in two ranges, waves 2, 3: Q's); 0 / 1 = only G
// (u1) / only Q (u2), its windows in four ranges, one a wave -- the other
// workgroup of the item does the other scalar on another CU (its own table
// walks).  pout: the partial sums go there for the host to join, no joins
// here.
// uin (the resident kernel, and k_verify_split's host-staged batches: the
// host computed them): u1, u2 as 16 LE words, loaded with the other inputs,
// so the waves skip s^-1 and the two mod-N products (~3 us of a lone call's
// critical path on one wave).
// TFREE: table-free keys are served (thread 0 runs the ladder); the resident
// kernel's instances are not (resident.cpp keeps such keys off the mailbox:
// a slot that held one would read BAD_KEY).
template <bool WIDE, int NP = 4, bool TFREE = true>
MBFT_DEV void split_item(const VerifyArgs& A, long i, uint32_t (&part)[NP][4 * NL + 1],
                         uint4 (&pre)[4][4 * kSplitPre], uint32_t* pout = nullptr, int half = -1,
                         const uint32_t* uin = nullptr) {
  constexpr int NW = 4;  // waves
  static_assert(NP == 4 || NP == 8, "partial sums: 4 (both scalars), 8 (one scalar, extras)");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool qh = half < 0 ? wave >= 2 : half == 1;  // this wave's scalar: u2 (Q) or u1 (G)
  // every input load issued at once (zero-copy staging: one PCIe round trip)
  // (admit's rules, open-coded: through the helper the resident kernels'
  // scratch and this kernel's registers moved)
  uint32_t ew[8], rw[8], sw[8], U[8];
  load_be256(ew, A.e + 32 * i);
  load_be256(rw, A.r + 32 * i);
  load_be256(sw, A.s + 32 * i);
  if (uin) {
#pragma unroll
    for (int j = 0; j < 8; j++) U[j] = uin[(qh ? 8 : 0) + j];
  }
  const uint32_t slot = A.slot[i];
  fe wv;
  if (A.winv && !uin) plane_load(wv, A.winv, A.n, i);  // s^-1 R from the host (lone calls)
  const bool range_ok = !words_is_zero(rw) && words_lt(rw, kNw) && !words_is_zero(sw) && words_lt(sw, kNw);
  KeyDesc kd{A.tabG, (uint32_t)A.wg, 0u};
  if (slot < A.nslots) kd = A.keys[slot];
  const bool tfree = slot < A.nslots && kd.valid && key_class_queued(kd.wbits);
  const bool key_ok = slot < A.nslots && kd.valid && (TFREE || !tfree);
  if (!(key_ok && range_ok) || tfree) {  // block-uniform: the whole workgroup returns
    // the status last, after every wave has read the inputs: the host may
    // reuse zero-copy staging as soon as it sees it (batch.cpp spin_statuses)
    __syncthreads();
    if (threadIdx.x == 0) {
      if (TFREE && tfree && range_ok)
        verify_ladder_inline(A, i);
      else
        A.status[i] = key_ok ? ST_REJECT : ((A.host_status & kArgHostStatus) && slot >= kHostSlot ? (uint8_t)slot : ST_BAD_KEY);
    }
    return;
  }
  SPLIT_T(1);
  if (!uin) {
    if (!A.winv) {
      uint32_t iw[8];
      if (!modinv_n_var_wave(iw, sw)) {
#pragma unroll
        for (int k = 0; k < 8; k++) iw[k] = 0;  // not reachable: 0 < s < N
      }
      fe_from_words(wv, iw);
      fn_to_mont(wv, wv);  // s^-1 R
    }
    SPLIT_T(2);
    uint32_t U1[8], U2[8];
    {
      fe e, r;
      fe_from_words(e, ew);
      fe_from_words(r, rw);
      scalars(U1, U2, e, r, wv);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) U[j] = qh ? U2[j] : U1[j];
  }
  SPLIT_T(3);
  const uint32_t* tab = qh ? kd.tab : A.tabG;
  const int W = qh ? (int)kd.wbits : A.wg;
  const int S = (256 + W - 1) / W, mid = (S + 1) / 2;
  // this wave's range of the scalar's windows
  const int lo = half < 0 ? ((wave & 1) ? mid : 0) : wave * S / NW;
  const int hi = half < 0 ? ((wave & 1) ? S : mid) : (wave + 1) * S / NW;
  uint32_t carry = 0;
#pragma unroll 1
  for (int k = 0; k < lo; k++) {
    bool ng, zr;
    (void)comb_digit(U[0], carry, W, k + 1 >= S, ng, zr);
    shr_words(U, W);
  }
  chud acc, ex;
  bool inf, exinf = true;
  comb_range_uniform<WIDE>(acc, inf, U, carry, tab, W, S, lo, hi, pre[wave], NP == 8 ? &ex : nullptr,
                           &exinf);
  SPLIT_T(4);
  bool degen = false;
  if (!inf) {
    fe zc = acc.ZZ;
    fe_canon(zc);
    degen = fe_is_zero_canon(zc);
  }
  auto put = [&](int slot_, const chud& p, uint32_t flags) {
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < NL; k++) {
        part[slot_][k] = p.X.v[k];
        part[slot_][NL + k] = p.Y.v[k];
        part[slot_][2 * NL + k] = p.ZZ.v[k];
        part[slot_][3 * NL + k] = p.ZZZ.v[k];
      }
      part[slot_][4 * NL] = flags;
    }
  };
  auto get = [&](int slot_, chud& p) -> uint32_t {
#pragma unroll
    for (int k = 0; k < NL; k++) {
      p.X.v[k] = part[slot_][k];
      p.Y.v[k] = part[slot_][NL + k];
      p.ZZ.v[k] = part[slot_][2 * NL + k];
      p.ZZZ.v[k] = part[slot_][3 * NL + k];
    }
    return part[slot_][4 * NL];
  };
  // flags: 1 = infinity, 2 = degenerate (the exact path decides)
  put(wave, acc, (inf ? 1u : 0u) | (degen ? 2u : 0u));
  if constexpr (NP == 8) put(NW + wave, ex, exinf ? 1u : 0u);  // (affine: never degenerate)
  __syncthreads();
  if (pout) {  // the resident kernel: the host joins the NW sums (join_host.cpp)
    if (wave != 0) return;
    uint32_t fl = 0;
#pragma unroll
    for (int w = 0; w < NP; w++) fl |= part[w][4 * NL];
    if (fl & 2u) {
      verify_exact(A, i);
      return;
    }
    for (int k = lane; k < NP * 40; k += 64) {
      const int w = k / 40, j = k - 40 * w;
      pout[k] = j <= 4 * NL ? part[w][j] : 0u;
    }
    // (thread 0 -- this wave's lane 0 -- stores the done word after
    // sys_release, which waits for these stores and writes them back)
    if (lane == 0) A.status[i] = kSrvPartials;
    return;
  }
  // The joins as a two-level tree -- level 0: waves 0 and 2 add the halves
  // (G: slots 0 + 1, Q: 2 + 3), level 1: wave 0 adds the two sums -- in ONE
  // loop body, so the second level runs the first's instructions from a warm
  // instruction cache (a lone item's cold straight-line code costs ~2x:
  // tools/split_timing.py measured 9 us for a cold x-only join against
  // 3.6 us warm).  The full join's Y3 / ZZZ3 at level 1 are not needed
  // (the x-check reads X and ZZ) but cost less than cold code.
  if constexpr (NP != 4) return;  // (the one-scalar form always has pout)
#pragma unroll 1
  for (int lvl = 0; lvl < 2; lvl++) {
    const int step = 1 << lvl;
    if ((wave & (2 * step - 1)) == 0) {
      chud a, b, o;
      const uint32_t fa = get(wave, a), fb = get(wave + step, b);
      uint32_t fo = 0;
      if ((fa | fb) & 2u) {
        fo = 2u;
      } else if (fa & 1u) {
        o = b;
        fo = fb;
      } else if (fb & 1u) {
        o = a;
      } else if (!(WIDE ? ec_add_chud_full_wide(o, a, b) : ec_add_chud_full(o, a, b))) {
        fo = 2u;  // H == 0: equal or opposite partial sums
      }
      put(wave, o, fo);
    }
    if (lvl == 0) SPLIT_T(5);
    __syncthreads();
  }
  if (wave != 0) return;
  SPLIT_T(7);
  chud g;
  const uint32_t fg = get(0, g);
  if (fg & 2u) {
    verify_exact(A, i);
    return;
  }
  if (fg & 1u) {
    if (lane == 0) A.status[i] = ST_REJECT;  // u1 G + u2 Q = infinity: (0, 0) -> false
    return;
  }
  fe zc = g.ZZ;
  fe_canon(zc);
  if (fe_is_zero_canon(zc)) {
    verify_exact(A, i);
    return;
  }
  verify_finish(A, i, g.X, g.ZZ, rw);
  SPLIT_T(8);
#ifdef MBFT_SPLIT_TIMING
  if (threadIdx.x == 0 && blockIdx.x == 0) g_split_clk[1] = clock64();
#endif
}
