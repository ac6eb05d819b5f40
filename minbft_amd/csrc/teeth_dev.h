// The compact key class (mbft_set_key_teeth, t = 2 .. 8 teeth): u Q for a key
// that owns a SMALL table, by a Lim-Lee comb WITH doublings.  With d =
// ceil(256 / t) columns the table holds 2^t entries of 64 bytes (256 B at
// t = 2, 1 KiB at t = 4, 16 KiB at t = 8), entry v = (sum_j bit_j(v) 2^(j d)) Q
// for v = 1 .. 2^t - 1 (entry 0 is never read), and a scalar costs d - 1
// doublings and at most d mixed additions.  Between the table-free class (64
// bytes, ladder_dev.h) and the comb without doublings (>= 32 KiB at W = 4).
// No LDS, no scratch memory; the entry address is per lane (the key's own
// table).
//
// Two parts, as in ladder_dev.h:
//  * the recoding (teeth_columns, teeth_column) in plain C++ that also
//    compiles for the host (tests/csrc/teeth_check.cpp runs it on the CPU
//    against Python integers, tests/test_teeth_host.py);
//  * the evaluation over the curve (teeth_mul; HIP only).
//
// RECODING.  u in [0, 2^256) is read as t teeth of d bits: tooth j holds the
// bits j d .. j d + d - 1, and bits at positions >= 256 are zero (the ragged
// top tooth when t d > 256: t = 3, 5, 6, 7).  Column c in [0, d) is
//     v_c = sum_j bit(u, j d + c) << j,      u = sum_c val(v_c) 2^c,
//     val(v) = sum_j bit_j(v) 2^(j d)        (the table's multiplier of entry v).
// No digit array: teeth_column picks each bit out of the eight scalar words
// with compile-time word indices (a select per word, so the words stay in
// registers), ~20 t instructions a column beside ~18 field reductions.
//
// EVALUATION.  acc = infinity; for c = d - 1 .. 0: acc = 2 acc (unless still
// infinity), then acc += entry[v_c] if v_c != 0 (acc = entry if still
// infinity).  v_(c-1) depends on u alone, so the NEXT column's entry is loaded
// before the current column's doubling and addition: its latency sits under
// ~18 reductions of arithmetic.
//
// DEGENERATE ADDITIONS: none, for u in [1, N).  After column c the
// accumulator is m_c Q with the prefix m_c = sum_(c' >= c) val(v_c') 2^(c' - c).
//  * m_c is u's bits at positions j d + e, e >= c, moved down by c: m_c =
//    sum_j ((tooth_j >> c) << (j d)).  The moved teeth do not overlap and
//    m_c 2^c <= u (tooth by tooth), so m_c <= u < N, and m_c > 0 from the
//    first nonzero column on.  N is prime: m Q = infinity only for N | m, so
//    acc is never infinity after its first entry, and a doubling never meets
//    a point of order 2 (there is none).
//  * a step with k = val(v_c) != 0 adds k Q to 2 m' Q (m' = m_(c+1) > 0).
//    2 m' has its bits at positions j d + e with 1 <= e <= d - 1 - c (tooth
//    j of m' has d - 1 - c bits), k at positions j d: disjoint, so 2 m' + k =
//    m_c with no carry, and 2 m' != k as integers (both nonzero, disjoint
//    bits).  Both lie in [1, m_c] and m_c < N, so 2 m' = k (mod N) would need
//    2 m' = k; and 2 m' = -k (mod N) would need m_c = 0 (mod N), but 0 < m_c <
//    N.  Neither holds: the mixed addition is never degenerate.
//  * every table multiplier val(v), v in [1, 2^t), is a nonzero integer with
//    its top bit at (t - 1) d <= 224 < 2^255 < N: in [1, N), never infinity,
//    and pairwise distinct (distinct bit sets).
// teeth_mul does not rely on this: it runs the unchecked formulas (a
// degenerate mixed addition leaves Z == 0 for good, ecc.h) and, where the
// final Z is zero, recomputes the scalar with ec_madd_complete at every
// addition -- a hole in the argument costs time, never a wrong status.
// tests/test_teeth_host.py checks the argument on the integer model;
// tests/golden/teeth_edges.json holds the corner columns.
//
// COST per scalar, in field reductions (doubling 8, mixed addition 10):
// t = 2: 128 columns, ~1,980; t = 3: 86, ~1,430; t = 4: 64, ~1,100; t = 6:
// 43, ~760; t = 8: 32, ~570 -- against ~2,900 for the table-free ladder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbft {

#ifndef MBFT_HD
#define MBFT_HD __host__ __device__ __forceinline__
#endif

// (a compact key's KeyDesc.wbits is kTeethFlag | t: kernels.h)
constexpr int kTeethMin = 2, kTeethMax = 8;

MBFT_HD int teeth_columns(int t) { return (256 + t - 1) / t; }

// bit p of u (8 little-endian words); 0 for p >= 256
MBFT_HD uint32_t teeth_bit(const uint32_t (&u)[8], int p) {
  const int wi = p >> 5;
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) w = wi == k ? u[k] : w;
  return (w >> (p & 31)) & 1u;
}

// v_c: bit j = bit (j d + c) of u, j < t
MBFT_HD uint32_t teeth_column(const uint32_t (&u)[8], int t, int d, int c) {
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < kTeethMax; j++)
    if (j < t) v |= teeth_bit(u, j * d + c) << j;
  return v;
}

}  // namespace mbft

#ifdef __HIP__
#include "ecc.h"

namespace mbft {

// One table entry as loaded (16 words), converted to field elements at use.
struct TeethRaw {
  uint4 a, b, c, d;
};

MBFT_DEV void teeth_load(TeethRaw& e, const uint32_t* tab, uint32_t v) {
  const uint4* p = reinterpret_cast<const uint4*>(tab + 16 * (size_t)v);
  e.a = p[0];
  e.b = p[1];
  e.c = p[2];
  e.d = p[3];
}

MBFT_DEV void teeth_point(fe& x, fe& y, const TeethRaw& e) {
  const uint32_t wx[8] = {e.a.x, e.a.y, e.a.z, e.a.w, e.b.x, e.b.y, e.b.z, e.b.w};
  const uint32_t wy[8] = {e.c.x, e.c.y, e.c.z, e.c.w, e.d.x, e.d.y, e.d.z, e.d.w};
  fe_from_words(x, wx);
  fe_from_words(y, wy);
}

// (acc, inf) = u Q for u in [0, N) over the key's compact table `tab` (t
// teeth), acc and inf overwritten.  COMPLETE: every addition by
// ec_madd_complete; else unchecked (a degenerate addition leaves acc.Z == 0
// for good).
template <bool COMPLETE>
MBFT_DEV void teeth_run(jac& acc, bool& inf, const uint32_t (&U)[8], const uint32_t* tab, int t) {
  const int d = teeth_columns(t);
  inf = true;
  uint32_t v = teeth_column(U, t, d, d - 1);
  TeethRaw nxt{};
  if (v) teeth_load(nxt, tab, v);
#pragma unroll 1
  for (int c = d - 1; c >= 0; c--) {
    const uint32_t cur_v = v;
    const TeethRaw cur = nxt;
    // the next column's entry, in flight under this column's arithmetic
    v = c > 0 ? teeth_column(U, t, d, c - 1) : 0u;
    if (v) teeth_load(nxt, tab, v);
    if (!inf) ec_dbl(acc, acc);
    if (cur_v == 0u) continue;
    fe px, py;
    teeth_point(px, py, cur);
    if (COMPLETE) {
      ec_madd_complete(acc, inf, px, py);
    } else if (inf) {
      acc.X = px;
      acc.Y = py;
      fe_one_mont(acc.Z);
      inf = false;
    } else {
      ec_madd(acc, acc, px, py);
    }
  }
}

// The exact u Q: the unchecked comb, recomputed with complete additions where
// it met a degenerate one (none, by the argument above).  acc is Jacobian with
// Z != 0 unless inf.
MBFT_DEV void teeth_mul(jac& acc, bool& inf, const uint32_t (&U)[8], const uint32_t* tab, int t) {
  teeth_run<false>(acc, inf, U, tab, t);
  if (inf) return;
  fe z = acc.Z;
  fe_canon(z);
  if (fe_is_zero_canon(z)) teeth_run<true>(acc, inf, U, tab, t);
}

}  // namespace mbft
#endif  // __HIP__
