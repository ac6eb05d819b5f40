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
// The SIGNED compact class (mbft_set_key_signed_teeth, t = 2 .. 9, half the
// table) shares both parts: its recoding is described below, beside
// steeth_flip and teeth_pick (tests/csrc/steeth_check.cpp,
// tests/test_steeth_host.py), and the evaluation takes the class as a flag.
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
// (a signed compact key's is kSignedTeethFlag | t; see SIGNED COMPACT KEYS below)
constexpr int kSteethMin = 2, kSteethMax = 9;

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
  for (int j = 0; j < kSteethMax; j++)
    if (j < t) v |= teeth_bit(u, j * d + c) << j;
  return v;
}

// SIGNED COMPACT KEYS (mbft_set_key_signed_teeth, t = 2 .. 9 teeth): the same
// comb over a signed all-nonzero recoding, which stores only the entries
// whose top tooth is positive -- 2^(t-1) entries, 128 B at t = 2 to 16 KiB at
// t = 9, half the unsigned table of the same t.  With d = ceil(256 / t) and
// L = t d:
//  * the key side sees u in [1, N).  An even u is evaluated as k = N - u
//    (odd, in [1, N)) and the result's Y negated at the end; else k = u
//    (steeth_flip);
//  * an odd k < 2^L is sum_(i < L) b_i 2^i with every b_i in {+1, -1}:
//    b_(L-1) = +1 and b_i = +1 iff bit i + 1 of k is set (the sum is
//    2^(L-1) + (k - 1) - (2^(L-1) - 1) = k).  Bits of k at positions >= 256
//    are zero, so those digits are -1 (the ragged top, t = 3, 5, 6, 7, 9);
//  * column c holds the tooth digits s_j = b_(j d + c): its raw bits are
//    teeth_column(k, t, d, c + 1) with the top tooth's bit forced to 1 at
//    c = d - 1.  neg = (s_(t-1) < 0); the table index is the low t - 1 raw
//    bits, complemented when neg: index bit j says "tooth j has the top
//    tooth's sign".  The top column is always positive;
//  * entry idx = (2^((t-1) d) + sum_(j < t-1) sigma_j 2^(j d)) Q, sigma_j = +1
//    iff bit j of idx is set: odd, positive, pairwise distinct multipliers
//    below 2^234 ((t - 1) d <= 232, at t = 9).  Entry 0 IS read.
// There is no zero column: the accumulator is the top column's entry, then
// every column doubles it and adds an entry (Y negated when neg), d - 1
// doublings and d - 1 mixed additions in all -- 18 (d - 1) reductions: s2
// 2,286; s3 1,530; s4 1,134; s5 918; s6 756; s7 648; s8 558; s9 504.
//
// DEGENERATE ADDITIONS of the signed comb.  After column c the accumulator is
// m_c Q, m_c = sum_(c' >= c) val_c' 2^(c' - c) with val_c = sum_j s_j 2^(j d)
// odd, so m_c is odd; tests/test_steeth_host.py checks 0 < m_c < N on the
// integer model (10,000 random scalars and the corners for every t).  The
// step at column c adds val_c Q to 2 m_(c+1) Q: opposite points would need
// m_c = 0 (mod N), which 0 < m_c < N rules out; EQUAL points, 2 m_(c+1) =
// val_c (mod N), means m_c = 2 val_c (mod N) and DOES happen at the last
// column: k = 2 val_0(k) (mod N) has solutions for t = 2, 3, 8, 9 (two each,
// one of them even and reached through N - u; tests/golden/
// make_steeth_edges.py derives them).  Those scalars are reachable -- who
// chooses s chooses u2 -- so, as for the unsigned comb, teeth_mul runs the
// unchecked formulas and recomputes with ec_madd_complete at every addition
// where the final Z is zero.
//
// k = (sg and u even) ? N - u : u; returns whether it flipped.  u < N.
MBFT_HD bool steeth_flip(uint32_t (&k)[8], const uint32_t (&u)[8], bool sg) {
  const uint32_t n[8] = {0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu,
                         0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu};
  const bool flip = sg && (u[0] & 1u) == 0u;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t df = (uint64_t)n[i] - u[i] - borrow;
    borrow = (uint32_t)(df >> 32) & 1u;
    k[i] = flip ? (uint32_t)df : u[i];
  }
  return flip;
}

// Column c of either class: the table index v, whether the column adds an
// entry at all (`have`: always for a signed key, v != 0 for an unsigned one)
// and whether the entry is subtracted (`neg`: signed keys only).  k is the
// scalar steeth_flip returned.
MBFT_HD void teeth_pick(uint32_t& v, bool& have, bool& neg, const uint32_t (&k)[8], int t, int d, int c, bool sg) {
  const uint32_t top = 1u << (t - 1);
  uint32_t raw = teeth_column(k, t, d, c + (sg ? 1 : 0));
  if (sg && c == d - 1) raw |= top;
  neg = sg && (raw & top) == 0u;
  v = sg ? ((neg ? ~raw : raw) & (top - 1u)) : raw;
  have = sg || raw != 0u;
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

// (acc, inf) = k Q over the key's compact table `tab` (t teeth; sg: the
// signed class, k odd), acc and inf overwritten.  One body for both classes,
// the class a per-lane flag: a wave that holds both costs the longer of the
// two.  COMPLETE: every addition by ec_madd_complete; else unchecked (a
// degenerate addition leaves acc.Z == 0 for good).
template <bool COMPLETE>
MBFT_DEV void teeth_run(jac& acc, bool& inf, const uint32_t (&K)[8], const uint32_t* tab, int t, bool sg) {
  const int d = teeth_columns(t);
  inf = true;
  uint32_t v;
  bool have, neg;
  teeth_pick(v, have, neg, K, t, d, d - 1, sg);
  TeethRaw nxt{};
  if (have) teeth_load(nxt, tab, v);
#pragma unroll 1
  for (int c = d - 1; c >= 0; c--) {
    const bool cur_have = have, cur_neg = neg;
    const TeethRaw cur = nxt;
    // the next column's entry, in flight under this column's arithmetic
    have = false;
    if (c > 0) teeth_pick(v, have, neg, K, t, d, c - 1, sg);
    if (have) teeth_load(nxt, tab, v);
    if (!inf) ec_dbl(acc, acc);
    if (!cur_have) continue;
    fe px, py;
    teeth_point(px, py, cur);
    if (cur_neg) fe_neg(py, py);
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
// it met a degenerate one (none for an unsigned key, the last column's
// doubling case for a signed one, above).  acc is Jacobian with Z != 0 unless
// inf.
MBFT_DEV void teeth_mul(jac& acc, bool& inf, const uint32_t (&U)[8], const uint32_t* tab, int t, bool sg) {
  uint32_t K[8];
  const bool flip = steeth_flip(K, U, sg);
  teeth_run<false>(acc, inf, K, tab, t, sg);
  if (inf) return;
  fe z = acc.Z;
  fe_canon(z);
  if (fe_is_zero_canon(z)) teeth_run<true>(acc, inf, K, tab, t, sg);
  if (flip && !inf) fe_neg(acc.Y, acc.Y);
}

}  // namespace mbft
#endif  // __HIP__
