// The batch signer from the key's load to the bytes it writes, device only:
// what k_sign_tags and k_usig_uis (sign_kernels.hip) share, in pieces that the
// test-only harness tests/csrc/sign_dev_check.hip calls one at a time with
// inputs of its choosing -- a nonce cannot be chosen through the kernels, it
// comes out of HMAC.
//
// Per lane, from the digest input e and the role's private key d:
//   k      RFC 6979 3.2, HMAC-SHA-256 (sign_dev.h), at most kSignTries
//          candidates (SignNonces);
//   R = kG a signed fixed-window comb over a small dedicated generator table
//          (window 4..6: 33 / 52 / 87 KB, the layout of k_table_fill), one
//          mixed addition per window, unconditionally (sign_comb);
//   r      x(R) mod N, with 1 / Z by the fixed-exponent fe_inv (sign_r);
//   s      k^-1 (e + r d) mod N, with k^-1 by the fixed-exponent fn_inv
//          (sign_s);
//   the candidate loop with the zero checks of r and s (sign_loop), the whole
//   as sign_rs, and the bytes of a tag or a UI (sign_tag_finish,
//   usig_ui_finish).
//
// UNIFORM ACCESS.  No load address, branch condition or loop trip count
// depends on d, k, k^-1 or a value derived from them:
//  * the hash side is straight-line SHA-256 compressions over registers;
//  * every window's entries are ALL read, at addresses made of the window
//    number and a loop counter, and merged into the lane's entry by a mask
//    (sign_pick, which also keeps the compiler from predicating those loads
//    on the digit: the generated loop is unconditional global_load_dwordx4 +
//    v_bfi_b32); the entry's sign, the "digit is zero" and
//    "accumulator still at infinity" cases are selects (v_cndmask), never
//    branches;
//  * loop trip counts are the window count ceil(256 / W), the entries of a
//    window and the fixed exponent bits of the two inversions;
//  * field and scalar arithmetic (fe29.h) is carry-free multiply-add with
//    select-based conditional subtractions.
// The ONE exception is the RFC's retry: a candidate outside [1, q), or one
// giving r == 0 or s == 0, is discarded and the lane draws the next, which
// tells only that a discarded candidate was unusable (probability 2^-32 per
// item with q = N; r == 0 / s == 0 cannot be met with real inputs).  The
// tag's length and bytes are the public output.
//
// Plain C++ and vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "der_enc_dev.h"
#include "ecc.h"
#include "sign_dev.h"

namespace mbft {

// 32 bytes at p (4-byte aligned) as big-endian-numeric words
MBFT_DEV void load_be_words(uint32_t w[8], const uint8_t* p) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(q[j]);
}

// acc = k G for 1 <= k < N (little-endian words), uniform access: see the
// header of this file.  tab: the signer's generator table for window W.
//
// NO DEGENERATE ADDITION AMONG THE KEPT RESULTS.  Windows go low to high.
// Before window i the accumulator holds m G with m = sum_{j<i} d_j 2^(Wj),
// |d_j| <= 2^(W-1), so |m| <= 2^(W-1) (2^(Wi) - 1) / (2^W - 1) < (4/7) 2^(Wi)
// for W >= 3.  A sum is KEPT only when d_i != 0 and m != 0 (otherwise the
// select keeps the old accumulator, or takes the entry itself); the entry is
// c G with c = d_i 2^(Wi), |c| >= 2^(Wi) > |m|.  The addition degenerates
// iff m == +-c (mod N), i.e. iff N divides m - c or m + c, both nonzero.
//  * Windows i < S - 1: |c| <= 2^(W(i+1)-1) <= 2^(W(S-1)-1) <= 2^254, so
//    0 < |m -+ c| < 2^255 < N.
//  * The last window: 0 < d <= 2^L, c = d 2^(W(S-1)) <= 2^256, and m + c = k
//    with 0 < k < N, so N does not divide m + c; and 0 < c - m <= 2^256 +
//    |m| < 2N, so c - m == N would be needed: then k = m + c = N + 2m, and
//    0 < k < N forces m < 0 and d 2^(W(S-1)) = N + m in (N - (4/7) 2^(W(S-1)),
//    N).  With v = W(S-1) >= 252 (W = 4, 5, 6: v = 252, 255, 252) and N =
//    2^256 - delta, delta < 2^225, the multiples of 2^v below N are at most
//    2^256 - 2^v = N - (2^v - delta) < N - (4/7) 2^v: none lies in the range.
// So H != 0 in every kept addition, Z stays nonzero, and the final kG (k in
// [1, N)) is a finite point.  (tests/test_sign_host.py checks the recoding's
// digits and this property on the host build of sign_digit;
// tests/test_gpu_sign_dev.py runs this function over the recoding's corners.)
MBFT_DEV void sign_comb(jac& acc, const uint32_t k[8], const uint32_t* __restrict__ tab, int W) {
  uint32_t U[8];
#pragma unroll
  for (int j = 0; j < 8; j++) U[j] = k[j];
  fe_zero(acc.X); fe_zero(acc.Y); fe_zero(acc.Z);
  fe one;
  fe_one_mont(one);
  bool inf = true;
  uint32_t carry = 0;
  const int S = sign_steps(W);
#pragma unroll 1
  for (int step = 0; step < S; step++) {
    bool neg;
    const uint32_t mag = sign_digit(U, carry, W, step + 1 == S, neg);
    uint32_t w[16];
    sign_pick(w, tab + (((size_t)step << (W - 1)) * 16u), sign_window_entries(W, step), mag);
    fe px, py, ny;
    fe_from_words(px, w);
    fe_from_words(py, w + 8);
    fe_neg(ny, py);
    fe_select(py, neg, ny, py);
    jac sum;
    ec_madd(sum, acc, px, py);  // always; its result is dropped by the selects below
    const bool zero = mag == 0;
    // digit 0: keep acc; acc at infinity: take the entry; else the sum
    fe_select(sum.X, inf, px, sum.X);
    fe_select(sum.Y, inf, py, sum.Y);
    fe_select(sum.Z, inf, one, sum.Z);
    fe_select(acc.X, zero, acc.X, sum.X);
    fe_select(acc.Y, zero, acc.Y, sum.Y);
    fe_select(acc.Z, zero, acc.Z, sum.Z);
    inf = inf && zero;
  }
}

// r = x mod N of the Jacobian point (X, ., Z), Z != 0 (coordinates within
// ec_madd's output bounds: X < 2^257 + 2^234, Z < 2^258): canonical limbs and
// the same as 8 little-endian words.
MBFT_DEV void sign_r(fe& r, uint32_t (&rw)[8], const fe& X, const fe& Z) {
  fe zi;
  fe_inv(zi, Z);
  fe_sqr(zi, zi);
  fe_mul(r, X, zi);
  fe_from_mont(r, r);
  fe_canon(r);
  fn_canon(r);  // r = x mod N (x < p < 2N)
  fe_to_words(rw, r);
}

// s = k^-1 (e + r d) mod N as 8 little-endian words: kw the nonce (little-
// endian words, 0 < k < N), r canonical, dm_n = d in Montgomery form mod N,
// e < 2^256 plain.
MBFT_DEV void sign_s(uint32_t (&sw)[8], const uint32_t (&kw)[8], const fe& r, const fe& dm_n, const fe& e) {
  fe k, kinv, t, rd;
  fe_from_words(k, kw);
  fn_to_mont(kinv, k);
  fn_inv(kinv, kinv);
  fn_mul(rd, r, dm_n);  // r d (plain)
  fe_add(t, e, rd);
  fn_canon(t);
  fn_mul(t, t, kinv);
  fn_canon(t);
  fe_to_words(sw, t);
}

// The candidate loop.  Nonces: next(kb) hands out the next candidate (big-
// endian-numeric words, in [1, N)) or returns false when none is left;
// discarded() is told that the last one gave r == 0 or s == 0.  (r, s) of the
// first usable candidate as big-endian-numeric words and true; false (r = s =
// 0) when the source ran out.
template <class Nonces>
MBFT_DEV bool sign_loop(uint32_t (&rb)[8], uint32_t (&sb)[8], Nonces& src, const fe& dm_n, const fe& e,
                        const uint32_t* tab, int W) {
#pragma unroll
  for (int j = 0; j < 8; j++) { rb[j] = 0; sb[j] = 0; }
  bool ok = false;
  uint32_t kb[8];
#pragma unroll 1
  while (src.next(kb)) {
    uint32_t kw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) kw[j] = kb[7 - j];
    jac R;
    sign_comb(R, kw, tab, W);
    fe x;
    uint32_t rw[8], sw[8];
    sign_r(x, rw, R.X, R.Z);
    sign_s(sw, kw, x, dm_n, e);
    if (!words_is_zero(rw) && !words_is_zero(sw)) {
#pragma unroll
      for (int j = 0; j < 8; j++) { rb[j] = rw[7 - j]; sb[j] = sw[7 - j]; }
      ok = true;
      break;
    }
    src.discarded();
  }
  return ok;
}

// The product's nonce source: RFC 6979 over (d, e) with q = N, at most
// kSignTries candidates, the RFC's step h.3 after a discarded one.
struct SignNonces {
  Rfc6979 g;
  uint32_t q[8];
  int left;
  MBFT_DEV void init(const uint32_t (&db)[8], const uint32_t (&eb)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = kNw[7 - j];  // N as big-endian-numeric words
    g.init(db, eb, q);
    left = kSignTries;
  }
  MBFT_DEV bool next(uint32_t (&kb)[8]) { return rfc6979_next(g, q, kb, left); }
  MBFT_DEV void discarded() { g.retry(); }  // RFC 6979 3.2 h.3 for a discarded candidate
};

// The signer both kernels share: (r, s) over the digest input eb
// (big-endian-numeric words) under the 32-byte big-endian key at `key`, the
// values as big-endian-numeric words.  Everything from the key's load on:
// the nonce loop, sign_comb, the two fixed-exponent inversions, the zero
// checks.  false (r = s = 0): none of kSignTries candidates was usable.  The
// callers finish their hashing of public bytes before they call it, so the
// key and what derives from it are live only here.
MBFT_DEV bool sign_rs(uint32_t (&rb)[8], uint32_t (&sb)[8], const uint8_t* key, const uint32_t (&eb)[8],
                      const uint32_t* tab, int W) {
  uint32_t db[8];
  load_be_words(db, key);

  uint32_t dw[8], ew[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { dw[j] = db[7 - j]; ew[j] = eb[7 - j]; }
  fe d, e, dm_n;
  fe_from_words(d, dw);
  fe_from_words(e, ew);
  fn_to_mont(dm_n, d);

  SignNonces src;
  src.init(db, eb);
  return sign_loop(rb, sb, src, dm_n, e, tab, W);
}

// What k_sign_tags writes for one lane after sign_rs: the tag into its
// kTagSlot-byte slot and its length, or the slot zeroed and length 0.
MBFT_DEV void sign_tag_finish(uint8_t* out, uint8_t* len, bool ok, const uint32_t (&rb)[8],
                              const uint32_t (&sb)[8]) {
  if (ok) {
    *len = (uint8_t)der_encode_sig(out, rb, sb);
  } else {
#pragma unroll 1
    for (int j = 0; j < kTagSlot; j++) out[j] = 0;
    *len = 0;
  }
}

// What k_usig_uis writes for one lane after sign_rs: the UI into its
// kUiSlot-byte slot and its length, or the slot zeroed and length 0.
MBFT_DEV void usig_ui_finish(uint8_t* out, uint8_t* len, bool ok, uint64_t counter, uint64_t epoch,
                             const uint32_t (&rb)[8], const uint32_t (&sb)[8]) {
  if (ok) {
    *len = (uint8_t)usig_ui_write(out, counter, epoch, rb, sb);
  } else {
#pragma unroll 1
    for (int j = 0; j < kUiSlot; j++) out[j] = 0;
    *len = 0;
  }
}

}  // namespace mbft
