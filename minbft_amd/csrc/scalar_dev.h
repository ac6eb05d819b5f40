// The verifier's scalar side, device code shared by the verifier's kernel units and the
// test-only harness tests/csrc/field_check.hip: the window shift and signed
// recoding of the comb (shr_words, comb_digit), u1 = e / s and u2 = r / s
// from the s^-1 planes (scalars), the whole-wave inversion mod N
// (quad_bcast, modinv_n_var_wave) and the accept test x(R) mod N == r
// (x_matches_r).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fe29.h"
#include "modinv.h"

namespace mbft {

// Shift an 8-word scalar right by W bits (0 < W < 32).
MBFT_DEV void shr_words(uint32_t (&U)[8], int W) {
#pragma unroll
  for (int j = 0; j < 7; j++) U[j] = __builtin_amdgcn_alignbit(U[j + 1], U[j], W);
  U[7] >>= W;
}

// Signed recoding of the current window (layout: table_kernels.hip, k_table_fill): `u` =
// the scalar's low word after the previous shifts, `carry` in/out.  Returns
// the table index of |d| (0 for d == 0, an entry that exists; `zero` flags
// the digit), `neg` = d < 0.
MBFT_DEV uint32_t comb_digit(uint32_t u, uint32_t& carry, int W, bool top, bool& neg,
                             bool& zero) {
  const uint32_t x = (u & ((1u << W) - 1u)) + carry;
  neg = !top && x > (1u << (W - 1));
  carry = neg ? 1u : 0u;
  const uint32_t mag = neg ? (1u << W) - x : x;
  zero = mag == 0u;
  return zero ? 0u : mag - 1u;
}

// u1 = e w, u2 = r w (mod N, canonical) as little-endian words.  One
// conditional subtraction makes them canonical: e, r < 2^256 and every w the
// s^-1 kernels produce is < 2^258 (an fn_mul output: < a b / R + N), so
// fn_mul's output is < 2^256 2^258 / 2^261 + N < 2N.
MBFT_DEV void scalars(uint32_t (&U1)[8], uint32_t (&U2)[8], const fe& e, const fe& r,
                      const fe& w) {
  fe u;
  fn_mul(u, e, w);
  fn_csub(u, 1);
  fe_to_words(U1, u);
  fn_mul(u, r, w);
  fn_csub(u, 1);
  fe_to_words(U2, u);
}

// x^-1 mod N (modinv.h's divsteps) by ALL 64 lanes of a wave together, on
// ONE value (every lane passes the same x; the roots of the batched s^-1).
// The two halves of each 30-divstep batch run where they are cheap:
//  * the 30 divsteps themselves on the SCALAR unit: f0, g0 and eta are
//    wave-uniform (v_readlane), so divsteps_30_var compiles to single
//    32-bit SALU instructions (s_ff1, shifts, s_mul) and uniform branches;
//  * the 2x2 matrix applied to the four 9-limb numbers on the VALU, split
//    over every quad of lanes: lane L = lane & 3 computes d' (0), e' (1)
//    (mod N) or f' (2), g' (3) (exact), and DPP quad broadcasts hand each
//    lane its next two operands ((d, e) on lanes 0, 1, (f, g) on 2, 3), so
//    the numbers stay in VGPRs.
// (Round 2's form gathered the four outputs to every lane with 36
// v_readlane per batch, which put the whole update on the scalar unit as
// multi-instruction 64-bit SALU arithmetic: ~840 SALU + 390 VALU per batch,
// ~43 us per inversion; tools/isa_hist.py.)  Returns the same as
// modinv_n_var.
MBFT_DEV int32_t quad_bcast(int32_t v, int sel) {
  // sel 0: lanes (0,0,2,2) of the quad, sel 1: lanes (1,1,3,3)
  return sel == 0 ? __builtin_amdgcn_mov_dpp(v, 0xA0, 0xF, 0xF, true)
                  : __builtin_amdgcn_mov_dpp(v, 0xF5, 0xF, 0xF, true);
}

MBFT_DEV bool modinv_n_var_wave(uint32_t out[8], const uint32_t x[8]) {
  const int L = __lane_id() & 3;
  const bool modn = L < 2;
  s30 M, xs;
  s30_modulus(M);
  s30_from_words(xs, x);
  // this lane's operands: (d, e) = (0, 1) on lanes 0, 1; (f, g) = (N, x) on 2, 3
  int32_t a[9], b[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    a[i] = modn ? 0 : M.v[i];
    b[i] = modn ? (i == 0 ? 1 : 0) : xs.v[i];
  }
  int32_t eta = -1;
#pragma unroll 1
  for (int it = 0; it < 64; it++) {
    trans2x2 t;
    const uint32_t f0 = (uint32_t)__builtin_amdgcn_readlane(a[0], 2);
    const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane(b[0], 2);
    eta = divsteps_30_var(eta, f0, g0, t);
    // this lane's output: L = 0 -> d', 1 -> e' (mod N), 2 -> f', 3 -> g'
    const int32_t c1 = (L & 1) ? t.q : t.u, c2 = (L & 1) ? t.r : t.v;
    int64_t c = (int64_t)c1 * a[0] + (int64_t)c2 * b[0];
    int32_t m = (c1 & (a[8] >> 31)) + (c2 & (b[8] >> 31));
    m -= (int32_t)((kNinv30 * (uint32_t)c + (uint32_t)m) & (uint32_t)kM30);
    m = modn ? m : 0;  // f, g: exact division, no multiple of N
    c += (int64_t)M.v[0] * m;
    c >>= 30;
    int32_t o[9];
#pragma unroll
    for (int i = 1; i < 9; i++) {
      c += (int64_t)c1 * a[i] + (int64_t)c2 * b[i] + (int64_t)M.v[i] * m;
      o[i - 1] = (int32_t)c & kM30;
      c >>= 30;
    }
    o[8] = (int32_t)c;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      a[i] = quad_bcast(o[i], 0);
      b[i] = quad_bcast(o[i], 1);
    }
    int32_t z = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) z |= b[j];
    if (__builtin_amdgcn_readlane(z, 2) == 0) {  // g == 0 (lane 2's b)
      s30 f, d;
#pragma unroll
      for (int j = 0; j < 9; j++) {
        f.v[j] = __builtin_amdgcn_readlane(a[j], 2);
        d.v[j] = __builtin_amdgcn_readlane(a[j], 0);
      }
      int32_t lo0 = 0, lo1 = 0;
#pragma unroll
      for (int j = 1; j < 9; j++) lo0 |= f.v[j];
#pragma unroll
      for (int j = 0; j < 8; j++) lo1 |= f.v[j] ^ kM30;
      const bool one = f.v[0] == 1 && lo0 == 0;
      const bool neg = lo1 == 0 && f.v[8] == -1;
      if (!one && !neg) return false;
      s30_to_words_mod(out, d, neg ? 1 : 0, M);
      return true;
    }
  }
  return false;
}

// x(R) mod N == r  <=>  X == r Z^2  or (r + N < p and X == (r + N) Z^2).
// With ZZ = Z^2 R and X = x R (Montgomery), one merged product gives
// (r ZZ + X (p - 1)) / R == r Z^2 - x (mod p): zero iff accepted.
MBFT_DEV bool x_matches_r(const fe& X, const fe& ZZ, const uint32_t rw[8]) {
  fe r, pm1, d;
  fe_from_words(r, rw);
  fe_set(pm1, kPm1);
  fe_mul2(d, r, ZZ, X, pm1);
  fe_canon(d);
  bool ok = fe_is_zero_canon(d);
  if (!ok && words_lt(rw, kPmNw)) {
    fe nn;
    fe_set(nn, kN);
    fe_add(r, r, nn);
    fe_mul2(d, r, ZZ, X, pm1);
    fe_canon(d);
    ok = fe_is_zero_canon(d);
  }
  return ok;
}

}  // namespace mbft
