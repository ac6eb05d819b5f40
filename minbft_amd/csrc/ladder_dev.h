// The table-free key class (key window 0, MBFT_WINDOW_NONE): u Q for an
// affine Q that owns no comb table, by a signed-digit double-and-add ladder
// with +-Q as the only addend.  No per-lane table, no scratch memory, no LDS.
//
// Two parts:
//  * the recoding (NafTop, naf_init, naf_next) in plain C++ that also
//    compiles for the host (tests/csrc/ladder_check.cpp runs it on the CPU
//    against Python integers, tests/test_ladder_host.py);
//  * the ladder over the curve (ladder_mul; HIP only, ecc.h's ec_dbl, ec_madd
//    and ec_madd_complete).
//
// RECODING.  The non-adjacent form of u in [0, 2^256): digits d_i in
// {-1, 0, 1}, i = 0 .. 256, u = sum d_i 2^i, no two adjacent digits nonzero,
// so about a third of them are nonzero (256 doublings and ~86 additions per
// scalar, against 128 additions for plain binary).  With h = 3 u,
//     d_i = bit_(i+1)(h) - bit_(i+1)(u)
// (h - u = 2 u: the carries of u + 2 u mark exactly the runs NAF rewrites),
// which gives the digits from the TOP down with no digit storage: NafTop
// holds u and 3 u (258 bits: 9 words each) and naf_next reads bit 257 of both
// and shifts them left.  257 calls yield d_256 .. d_0.
//
// DEGENERATE ADDITIONS.  The ladder keeps acc = m Q, m the prefix value
// m_j = sum_(i >= j) d_i 2^(i - j).  For u in [1, N):
//  * every prefix from the first nonzero digit on is an integer in [1, N):
//    the leading digit is +1, the one after it is 0, so m_j >= 2^k - 2^(k-2)
//    - .. > 0; and m_j is u / 2^j rounded to a neighbour (|u - m_j 2^j| <
//    (2/3) 2^j), so m_j <= u < N for j = 0 and m_j < N / 2 + 1 for j >= 1.
//    Hence acc is never infinity after its first addition (N is prime: m Q =
//    infinity only for N | m), and a doubling never meets a point of order 2.
//  * a step with digit d != 0 adds d Q to 2 m_(j+1) Q.  The mixed addition
//    is degenerate iff 2 m_(j+1) = +-d (mod N).  2 m_(j+1) = -d would make
//    the step's result m_j = 2 m_(j+1) + d = 0 (mod N): excluded above.
//    2 m_(j+1) = d (mod N) with 0 < 2 m_(j+1) < 2 N and even: 2 m_(j+1) = d
//    is impossible (|d| = 1 is odd, or not positive), so 2 m_(j+1) = N + d;
//    d = +1 gives m_j = N + 2 > N, no prefix; d = -1 gives 2 m_(j+1) = N - 1
//    and m_j = N - 2, which exceeds N / 2 + 1, so j = 0 and u = N - 2 (odd,
//    N - 2 = 3 mod 4: its last digit is indeed -1).
//   So exactly ONE scalar in [1, N) meets a degenerate addition: u = N - 2,
//   at its last step, where -Q is added to (N - 1) Q = -Q: a doubling.  Anyone
//   can craft it (choose s = r / (N - 2)), no discrete log needed.
//  * the first nonzero digit finds acc at infinity: the ladder sets acc = +Q
//    there (leading zero digits double nothing).
// ladder_mul does not rely on this count: it runs the unchecked formulas
// (a degenerate mixed addition leaves Z == 0 for good, ecc.h) and, where the
// final Z is zero, recomputes the scalar with ec_madd_complete at every
// addition.  tests/test_ladder_host.py checks the argument on the integer
// model; tests/golden/ladder_edges.json holds u2 = N - 2 and its neighbours.
//
// COST per scalar: 256 doublings at 8 reductions + ~86 mixed additions at 10
// (Jacobian madd-2004-hmv with the merged Y3) = ~2,900 reductions, against
// ~170 for a whole W = 29 / 29 verify.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbft {

#ifndef MBFT_HD
#define MBFT_HD __host__ __device__ __forceinline__
#endif

constexpr int kNafDigits = 257;  // d_256 .. d_0

struct NafTop {
  uint32_t k[9], h[9];  // u and 3 u, shifted left by one per digit taken
};

// u: 8 little-endian words
MBFT_HD void naf_init(NafTop& f, const uint32_t u[8]) {
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    f.k[j] = u[j];
    c += (uint64_t)u[j] * 3u;
    f.h[j] = (uint32_t)c;
    c >>= 32;
  }
  f.k[8] = 0;
  f.h[8] = (uint32_t)c;
}

// The next digit from the top (-1, 0 or 1).
MBFT_HD int naf_next(NafTop& f) {
  const int d = (int)((f.h[8] >> 1) & 1u) - (int)((f.k[8] >> 1) & 1u);
#pragma unroll
  for (int j = 8; j > 0; j--) {
    f.k[j] = (f.k[j] << 1) | (f.k[j - 1] >> 31);
    f.h[j] = (f.h[j] << 1) | (f.h[j - 1] >> 31);
  }
  f.k[0] <<= 1;
  f.h[0] <<= 1;
  return d;
}

}  // namespace mbft

#ifdef __HIP__
#include "ecc.h"

namespace mbft {

// (acc, inf) = u Q for u in [0, N) and Q = (qx, qy) affine (canonical
// Montgomery, on the curve), acc and inf overwritten.  COMPLETE: every
// addition by ec_madd_complete; else unchecked (a degenerate addition leaves
// acc.Z == 0 for good: ec_madd's Z3 = Z1 H, ec_dbl's Z3 = 2 Y1 Z1).
template <bool COMPLETE>
MBFT_DEV void ladder_run(jac& acc, bool& inf, const uint32_t (&U)[8], const fe& qx, const fe& qy) {
  NafTop f;
  naf_init(f, U);
  inf = true;
#pragma unroll 1
  for (int i = 0; i < kNafDigits; i++) {
    const int d = naf_next(f);
    if (!inf) ec_dbl(acc, acc);
    if (d == 0) continue;
    fe py;
    fe_neg(py, qy);
    fe_select(py, d < 0, py, qy);
    if (COMPLETE) {
      ec_madd_complete(acc, inf, qx, py);
    } else if (inf) {
      acc.X = qx;
      acc.Y = py;
      fe_one_mont(acc.Z);
      inf = false;
    } else {
      ec_madd(acc, acc, qx, py);
    }
  }
}

// The exact u Q: the unchecked ladder, recomputed with complete additions
// where it met a degenerate one (u = N - 2, above).  acc is Jacobian with
// Z != 0 unless inf.
MBFT_DEV void ladder_mul(jac& acc, bool& inf, const uint32_t (&U)[8], const fe& qx, const fe& qy) {
  ladder_run<false>(acc, inf, U, qx, qy);
  if (inf) return;
  fe z = acc.Z;
  fe_canon(z);
  if (fe_is_zero_canon(z)) ladder_run<true>(acc, inf, U, qx, qy);
}

}  // namespace mbft
#endif  // __HIP__
