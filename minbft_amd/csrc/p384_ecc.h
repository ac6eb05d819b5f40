// P-384 points and the whole ECDSA check of one item, over
// p384_fe.h.  Compiles for the device (k_verify_p384) and for the host
// (mbft_pkix_parse_p384, tests/csrc/p384_host_check.cpp).
//
// POINTS.  Homogeneous projective (X : Y : Z), Montgomery coordinates, the
// point at infinity (0 : 1 : 0), and the COMPLETE formulas of Renes, Costello
// and Batina ("Complete addition formulas for prime order elliptic curves",
// EUROCRYPT 2016) for a = -3: algorithm 4 (addition) and algorithm 6
// (doubling).  They are branch-free and exact for every pair of points of a
// prime-order curve -- P + P, P + (-P), P + O, O + P and O + O included -- so
// nothing here detects a degenerate case and nothing is queued for an exact
// path.  The operation order is the paper's; only the small multiples (2 x,
// 3 x) are taken in one step.
//
// BOUNDS (p384_fe.h): every product is < 2^385 and every difference < 2^384 +
// 2^137; sums of up to four such terms are left unreduced.  The stored
// coordinates stay < 2^387 (p384_dbl's Z3 = 4 t0 t1 is the largest), and the
// largest product is (Y1 + Z1)(Y2 + Z2) < 2^387.6 * 2^387 < 2^776.
#pragma once
#include "p384_fe.h"

namespace mbft {

struct pt384 {
  fe384 X, Y, Z;
};

P384_HD void p384_set_inf(pt384& o) {
  fe384_zero(o.X);
  fe384_one_mont(o.Y);
  fe384_zero(o.Z);
}

P384_HD void p384_set_g(pt384& o) {
  fe384_set(o.X, kP384Gx);
  fe384_set(o.Y, kP384Gy);
  fe384_one_mont(o.Z);
}

// o = p + q (algorithm 4).  o may be p or q.
P384_HD void p384_add(pt384& o, const pt384& p, const pt384& q) {
  fe384 b, t0, t1, t2, t3, t4, x3, y3, z3;
  fe384_set(b, kP384B);
  fe384_mul(t0, p.X, q.X);
  fe384_mul(t1, p.Y, q.Y);
  fe384_mul(t2, p.Z, q.Z);
  fe384_add(t3, p.X, p.Y);
  fe384_add(t4, q.X, q.Y);
  fe384_mul(t3, t3, t4);
  fe384_add(t4, t0, t1);
  fe384_sub(t3, t3, t4);  // X1 Y2 + X2 Y1
  fe384_add(t4, p.Y, p.Z);
  fe384_add(x3, q.Y, q.Z);
  fe384_mul(t4, t4, x3);
  fe384_add(x3, t1, t2);
  fe384_sub(t4, t4, x3);  // Y1 Z2 + Y2 Z1
  fe384_add(x3, p.X, p.Z);
  fe384_add(y3, q.X, q.Z);
  fe384_mul(x3, x3, y3);
  fe384_add(y3, t0, t2);
  fe384_sub(y3, x3, y3);  // X1 Z2 + X2 Z1
  fe384_mul(z3, b, t2);
  fe384_sub(x3, y3, z3);
  fe384_tpl(x3, x3);
  fe384_sub(z3, t1, x3);
  fe384_add(x3, t1, x3);
  fe384_mul(y3, b, y3);
  fe384_tpl(t2, t2);
  fe384_sub(y3, y3, t2);
  fe384_sub(y3, y3, t0);
  fe384_tpl(y3, y3);
  fe384_tpl(t0, t0);
  fe384_sub(t0, t0, t2);
  fe384_mul(t1, t4, y3);
  fe384_mul(t2, t0, y3);
  fe384_mul(y3, x3, z3);
  fe384_add(o.Y, y3, t2);
  fe384_mul(x3, t3, x3);
  fe384_sub(o.X, x3, t1);
  fe384_mul(z3, t4, z3);
  fe384_mul(t1, t3, t0);
  fe384_add(o.Z, z3, t1);
}

// o = 2 p (algorithm 6).  o may be p.
P384_HD void p384_dbl(pt384& o, const pt384& p) {
  fe384 b, t0, t1, t2, t3, x3, y3, z3;
  fe384_set(b, kP384B);
  fe384_sqr(t0, p.X);
  fe384_sqr(t1, p.Y);
  fe384_sqr(t2, p.Z);
  fe384_mul(t3, p.X, p.Y);
  fe384_dbl(t3, t3);
  fe384_mul(z3, p.X, p.Z);
  fe384_dbl(z3, z3);
  fe384_mul(y3, b, t2);
  fe384_sub(y3, y3, z3);
  fe384_tpl(y3, y3);
  fe384_sub(x3, t1, y3);
  fe384_add(y3, t1, y3);
  fe384_mul(y3, x3, y3);
  fe384_mul(x3, x3, t3);
  fe384_tpl(t2, t2);
  fe384_mul(z3, b, z3);
  fe384_sub(z3, z3, t2);
  fe384_sub(z3, z3, t0);
  fe384_tpl(z3, z3);
  fe384_tpl(t0, t0);
  fe384_sub(t0, t0, t2);
  fe384_mul(t0, t0, z3);
  fe384_add(y3, y3, t0);
  fe384_mul(t0, p.Y, p.Z);
  fe384_dbl(t0, t0);
  fe384_mul(z3, t0, z3);
  fe384_sub(o.X, x3, z3);
  fe384_mul(z3, t0, t1);
  fe384_dbl(z3, z3);
  fe384_dbl(o.Z, z3);
  o.Y = y3;
}

// x, y as 12 little-endian words -> is (x, y) a point of the curve: both
// below p (on the words) and y^2 = x^3 - 3 x + b.  (0, 0) is none (b != 0).
// qx, qy: the Montgomery coordinates, set whatever the answer.
P384_HD bool p384_on_curve(fe384& qx, fe384& qy, const uint32_t x[12], const uint32_t y[12]) {
  const bool in_range = words384_lt(x, kP384w) && words384_lt(y, kP384w);
  fe384 b, l, r, t;
  fe384_set(b, kP384B);
  fe384_from_words(qx, x);
  fe384_from_words(qy, y);
  fe384_to_mont(qx, qx);
  fe384_to_mont(qy, qy);
  fe384_sqr(l, qy);
  fe384_sqr(r, qx);
  fe384_mul(r, r, qx);
  fe384_add(r, r, b);
  fe384_tpl(t, qx);
  fe384_sub(r, r, t);
  fe384_canon(l);
  fe384_canon(r);
  return in_range && fe384_eq_canon(l, r);
}

// u1 G + u2 Q by one joint double-and-add (Shamir) over {O, G, Q, G + Q}, the
// scalars 12 little-endian words each, Q = (qx, qy, 1).  G + Q comes from the
// complete addition: 2 G for Q = G, O for Q = -G.  Every step is a doubling
// and an addition of the selected entry (O where both bits are zero), so the
// work is the same for every scalar pair and no lane diverges.
P384_HD void p384_shamir(pt384& acc, const uint32_t u1[12], const uint32_t u2[12], const fe384& qx,
                         const fe384& qy) {
  pt384 g, q, gq, inf;
  p384_set_g(g);
  p384_set_inf(inf);
  q.X = qx;
  q.Y = qy;
  fe384_one_mont(q.Z);
  p384_add(gq, g, q);
  uint32_t a[12], b[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    a[i] = u1[i];
    b[i] = u2[i];
  }
  acc = inf;
#pragma unroll 1
  for (int step = 0; step < 384; step++) {
    const bool ba = a[11] >> 31, bb = b[11] >> 31;
#pragma unroll
    for (int i = 11; i > 0; i--) {
      a[i] = (a[i] << 1) | (a[i - 1] >> 31);
      b[i] = (b[i] << 1) | (b[i - 1] >> 31);
    }
    a[0] <<= 1;
    b[0] <<= 1;
    p384_dbl(acc, acc);
    pt384 sel;
    p384_set_g(sel);  // (constants: G costs no register across the loop)
    fe384_select(sel.X, bb, ba ? gq.X : q.X, ba ? sel.X : inf.X);
    fe384_select(sel.Y, bb, ba ? gq.Y : q.Y, ba ? sel.Y : inf.Y);
    fe384_select(sel.Z, bb, ba ? gq.Z : q.Z, ba ? sel.Z : inf.Z);
    p384_add(acc, acc, sel);
  }
}

// The finish, on the sum's X and Z (Montgomery, < 2^387): Z = 0 (infinity)
// rejects; otherwise x = X / Z in [0, p), and the signature holds iff x mod N
// == r, that is x = r, or x = r + N where r + N < p (p < 2 N).  r: 12
// little-endian words, in [1, N).
P384_HD bool p384_finish(const fe384& X, const fe384& Z, const uint32_t r[12]) {
  fe384 z = Z, x;
  fe384_canon(z);
  if (fe384_is_zero_canon(z)) return false;
  fe384_inv(x, Z);
  fe384_mul(x, x, X);
  fe384_from_mont(x, x);
  fe384_canon(x);
  uint32_t xw[12], rn[12];
  fe384_to_words(xw, x);
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    c += (uint64_t)r[i] + kN384w[i];
    rn[i] = (uint32_t)c;
    c >>= 32;
  }
  uint32_t d0 = 0, d1 = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    d0 |= xw[i] ^ r[i];
    d1 |= xw[i] ^ rn[i];
  }
  return d0 == 0 || (d1 == 0 && words384_lt(r, kPmN384w));
}

// Status codes of include/minbft_gpu.h, restated so that this header needs
// nothing else (p384.cpp asserts that they agree).
constexpr uint8_t kP384Accept = 0, kP384Reject = 1, kP384BadKey = 5;

// One item: e, r, s, x, y as 12 little-endian words each.  The precedence is
// the inline-key class's: a bad key first, also where r or
// s is out of range; then the range of r and s; then the curve.
P384_HD uint8_t p384_verify_item(const uint32_t e[12], const uint32_t r[12], const uint32_t s[12],
                                 const uint32_t x[12], const uint32_t y[12]) {
  fe384 qx, qy;
  if (!p384_on_curve(qx, qy, x, y)) return kP384BadKey;
  if (words384_is_zero(r) || words384_is_zero(s) || !words384_lt(r, kN384w) || !words384_lt(s, kN384w))
    return kP384Reject;
  uint32_t u1[12], u2[12];
  fn384_u1u2(u1, u2, e, r, s);
  pt384 acc;
  p384_shamir(acc, u1, u2, qx, qy);
  return p384_finish(acc.X, acc.Z, r) ? kP384Accept : kP384Reject;
}

// 48 big-endian bytes -> 12 little-endian words.
P384_HD void p384_words_from_be(uint32_t w[12], const uint8_t* be) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint8_t* b = be + 4 * (11 - i);
    w[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
}

}  // namespace mbft
