// The scalar side of the batch signer (sign_kernels.hip, k_sign_tags), one
// signature per lane, in plain C++ that also compiles for the host
// (tests/csrc/sign_check.cpp runs it on the CPU against the oracle):
//  * the RFC 6979 nonce with HMAC-SHA-256 (Rfc6979, rfc6979_next) exactly as
//    oracle/p256.py rfc6979_k states it, so a tag is reproducible from (d, e);
//  * the signed window recoding of the nonce (sign_digit) -- the digits of
//    the comb layout in table_kernels.hip (k_table_fill) -- and
//  * the masked pick of a lane's table entry out of a whole window read at
//    wave-uniform addresses (sign_pick);
//  * the byte format of a software-USIG UI (usig_ui_write; k_usig_uis,
//    tests/csrc/usig_check.cpp).
// Nothing here indexes memory, branches or bounds a loop by a secret; the one
// exception is rfc6979_next's retry, which tells only that a DISCARDED
// candidate was out of range (RFC 6979 3.2 step h.3).
//
// 256-bit values are 8 big-endian-numeric words (b[0] = bytes 0..3 of the 32
// big-endian bytes) on the hash side and 8 little-endian words on the
// recoding side, as in the verifier (words_dev.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "der_enc_dev.h"
#include "sha256.h"

namespace mbft {

// a < b, branch-free (borrow of a - b)
MBFT_HD bool be256_lt(const uint32_t a[8], const uint32_t b[8]) {
  uint64_t borrow = 0;
#pragma unroll
  for (int j = 7; j >= 0; j--) borrow = ((uint64_t)a[j] - b[j] - borrow) >> 63;
  return borrow != 0;
}

MBFT_HD bool be256_is_zero(const uint32_t a[8]) {
  uint32_t x = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) x |= a[j];
  return x == 0;
}

// a mod q for q >= 2^255 (a < 2^256 < 2q): one conditional subtraction, by
// select -- bits2octets of RFC 6979 2.3.4
MBFT_HD void be256_csub(uint32_t o[8], const uint32_t a[8], const uint32_t q[8]) {
  uint32_t d[8];
  uint64_t borrow = 0;
#pragma unroll
  for (int j = 7; j >= 0; j--) {
    const uint64_t t = (uint64_t)a[j] - q[j] - borrow;
    d[j] = (uint32_t)t;
    borrow = t >> 63;
  }
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = borrow ? a[j] : d[j];
}

// HMAC-SHA-256 generator state of RFC 6979 3.2 (x = d, h1 = e; hlen = qlen =
// 256, so one HMAC output is one candidate).  The key K is held as the two
// SHA-256 states after its ipad / opad block.
struct Rfc6979 {
  uint32_t V[8], si[8], so[8];

  MBFT_HD void key(const uint32_t K[8]) {
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = (j < 8 ? K[j] : 0u) ^ 0x36363636u;
    sha256_init(si);
    sha256_block(si, m);
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = (j < 8 ? K[j] : 0u) ^ 0x5c5c5c5cu;
    sha256_init(so);
    sha256_block(so, m);
  }
  // out = outer hash over the inner digest ih
  MBFT_HD void outer(uint32_t out[8], const uint32_t ih[8]) const {
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 8; j++) m[j] = ih[j];
    m[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; j++) m[j] = 0;
    m[15] = (64u + 32u) * 8u;
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = so[j];
    sha256_block(out, m);
  }
  // V = HMAC_K(V)
  MBFT_HD void step_v() {
    uint32_t m[16], ih[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { m[j] = V[j]; ih[j] = si[j]; }
    m[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; j++) m[j] = 0;
    m[15] = (64u + 32u) * 8u;
    sha256_block(ih, m);
    outer(V, ih);
  }
  // K = HMAC_K(V || tag || x || h) (97 bytes: two blocks), then V = HMAC_K(V)
  MBFT_HD void step_k_long(uint32_t tag, const uint32_t x[8], const uint32_t h[8]) {
    uint32_t m[16], ih[8], K[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { m[j] = V[j]; ih[j] = si[j]; }
    m[8] = (tag << 24) | (x[0] >> 8);
#pragma unroll
    for (int j = 1; j < 8; j++) m[8 + j] = (x[j - 1] << 24) | (x[j] >> 8);
    sha256_block(ih, m);
    m[0] = (x[7] << 24) | (h[0] >> 8);
#pragma unroll
    for (int j = 1; j < 8; j++) m[j] = (h[j - 1] << 24) | (h[j] >> 8);
    m[8] = (h[7] << 24) | 0x00800000u;
#pragma unroll
    for (int j = 9; j < 15; j++) m[j] = 0;
    m[15] = (64u + 97u) * 8u;
    sha256_block(ih, m);
    outer(K, ih);
    key(K);
    step_v();
  }
  // the retry step: K = HMAC_K(V || 0x00), V = HMAC_K(V)
  MBFT_HD void retry() {
    uint32_t m[16], ih[8], K[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { m[j] = V[j]; ih[j] = si[j]; }
    m[8] = 0x00800000u;
#pragma unroll
    for (int j = 9; j < 15; j++) m[j] = 0;
    m[15] = (64u + 33u) * 8u;
    sha256_block(ih, m);
    outer(K, ih);
    key(K);
    step_v();
  }
  // steps b .. g: x = the private key, e = the 32-byte hashToInt input, q =
  // the group order (2^255 <= q < 2^256)
  MBFT_HD void init(const uint32_t x[8], const uint32_t e[8], const uint32_t q[8]) {
    uint32_t h[8], K[8];
    be256_csub(h, e, q);
#pragma unroll
    for (int j = 0; j < 8; j++) { V[j] = 0x01010101u; K[j] = 0; }
    key(K);
    step_k_long(0x00u, x, h);
    step_k_long(0x01u, x, h);
  }
};

constexpr int kSignTries = 4;  // candidates per item before it reports failure

// Step h: the next candidate in [1, q), spending at most `left` candidates
// (decremented per candidate drawn).  false: none left.  After a candidate
// that the caller discards (r == 0 or s == 0) the caller runs g.retry().
MBFT_HD bool rfc6979_next(Rfc6979& g, const uint32_t q[8], uint32_t k[8], int& left) {
  while (left > 0) {
    left--;
    g.step_v();
    if (!be256_is_zero(g.V) && be256_lt(g.V, q)) {
#pragma unroll
      for (int j = 0; j < 8; j++) k[j] = g.V[j];
      return true;
    }
    g.retry();
  }
  return false;
}

// ---------------------------------------------------------------------------
// Window recoding, low window first (the signed-digit comb of scalar_dev.h):
// U = the scalar's 8 little-endian words, shifted right by W after each digit.
// x = low W bits + carry; x > 2^(W-1) -> digit x - 2^W, carry 1; the last
// window (top) keeps x: 0 <= digit <= 2^(256 - (S-1) W).  Returns |digit|;
// all by selects.
MBFT_HD uint32_t sign_digit(uint32_t (&U)[8], uint32_t& carry, int W, bool top, bool& neg) {
  const uint32_t x = (U[0] & ((1u << W) - 1u)) + carry;
  neg = !top && x > (1u << (W - 1));
  carry = neg ? 1u : 0u;
  const uint32_t mag = neg ? (1u << W) - x : x;
#pragma unroll
  for (int j = 0; j < 7; j++) U[j] = (U[j] >> W) | (U[j + 1] << (32 - W));
  U[7] >>= W;
  return mag;
}

MBFT_HD int sign_steps(int W) { return (256 + W - 1) / W; }
// entries of window `step`: |digit| = 1 .. count
MBFT_HD int sign_window_entries(int W, int step) {
  const int S = sign_steps(W);
  return step + 1 < S ? 1 << (W - 1) : 1 << (256 - (S - 1) * W);
}

// The lane's entry of one window: EVERY entry of the window is read, at an
// address that depends on the window and the loop counter alone (the same in
// all lanes), and kept where its number equals the lane's |digit|.  win: the
// window's `count` entries of 16 words.  A zero digit keeps entry 1 (a
// dummy operand whose sum the caller discards).
//
// The optimiser must not turn "load, then select" into "load where selected":
// left alone, clang sinks each load under its select and predicates it on the
// lanes whose digit matches (exec mask + s_cbranch_execz), which makes both a
// branch and the set of entries fetched depend on the nonce.  So all 16 words
// of an entry are loaded first and each passes through an empty volatile asm
// (sign_opaque) before any select sees it: the asm cannot be moved under a
// condition, so the loads stay unconditional.  The select itself is written
// as mask arithmetic, not ?:, so that it cannot become control flow either.
#if defined(__HIP_DEVICE_COMPILE__)
#define MBFT_SIGN_OPAQUE(v) asm volatile("" : "+v"(v))
#else
#define MBFT_SIGN_OPAQUE(v) asm volatile("" : "+r"(v))
#endif
MBFT_HD void sign_pick(uint32_t (&w)[16], const uint32_t* win, int count, uint32_t mag) {
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = win[k];
  for (int j = 2; j <= count; j++) {
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = win[16 * (j - 1) + k];
#pragma unroll
    for (int k = 0; k < 16; k++) MBFT_SIGN_OPAQUE(v[k]);
    uint32_t m = 0u - (uint32_t)(mag == (uint32_t)j);  // all ones where the lane takes entry j
    MBFT_SIGN_OPAQUE(m);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = (v[k] & m) | (w[k] & ~m);
  }
}

// ---------------------------------------------------------------------------
// The software USIG's UI (k_usig_uis), as the reference marshals it:
// usig.UI{Counter, Cert} is counter_be64 || cert (usig/usig.go:54-86) and the
// SGX USIG's cert is epoch_be64 || asn1.Marshal{R, S} (usig/sgx/sgx-usig.go:
// 143-168), so a UI is at most 8 + 8 + 72 bytes: one kUiSlot-byte slot per
// item, the bytes after the UI zeroed.  Returns the UI's length.  (The signed
// digest takes epoch and counter little-endian, sha256_usig_chain; the two
// byte orders are checked on the host build, tests/csrc/usig_check.cpp.)
constexpr int kUiSlot = 16 + kTagSlot;

MBFT_HD uint32_t usig_ui_write(uint8_t* slot, uint64_t counter, uint64_t epoch, const uint32_t r[8],
                               const uint32_t s[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    slot[j] = (uint8_t)(counter >> (56 - 8 * j));
    slot[8 + j] = (uint8_t)(epoch >> (56 - 8 * j));
  }
  return 16u + der_encode_sig(slot + 16, r, s);
}

}  // namespace mbft
