// Test-only: runs the batch signer's host-compilable device code on the HOST
// -- the RFC 6979 nonce, the window recoding and masked pick
// (minbft_amd/csrc/sign_dev.h) and the DER encoder
// (minbft_amd/csrc/der_enc_dev.h) -- so the CPU suite can check them against
// the oracle (tests/test_sign_host.py).  Built into tests/libsign_check.so by
// __graft_entry__.build().
#include <string.h>

#include "../../minbft_amd/csrc/der_enc_dev.h"
#include "../../minbft_amd/csrc/sign_dev.h"

namespace {
void be_words(uint32_t w[8], const uint8_t* p) {
  for (int j = 0; j < 8; j++)
    w[j] = ((uint32_t)p[4 * j] << 24) | ((uint32_t)p[4 * j + 1] << 16) |
           ((uint32_t)p[4 * j + 2] << 8) | p[4 * j + 3];
}
}  // namespace

extern "C" {

// n nonces: d, e, k_out n x 32 big-endian bytes, q 32 bytes.  tries[i] = the
// candidates drawn (1 .. kSignTries), or 0 when none of them was in [1, q)
// (k_out then zero).
int sign_check_nonce(const uint8_t* d, const uint8_t* e, const uint8_t* q, int n, uint8_t* k_out,
                     int32_t* tries) {
  uint32_t qw[8];
  be_words(qw, q);
  for (int i = 0; i < n; i++) {
    uint32_t dw[8], ew[8], kw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    be_words(dw, d + 32 * i);
    be_words(ew, e + 32 * i);
    mbft::Rfc6979 g;
    g.init(dw, ew, qw);
    int left = mbft::kSignTries;
    const bool ok = mbft::rfc6979_next(g, qw, kw, left);
    tries[i] = ok ? mbft::kSignTries - left : 0;
    for (int j = 0; j < 8; j++)
      for (int b = 0; b < 4; b++) k_out[32 * i + 4 * j + b] = ok ? (uint8_t)(kw[j] >> (24 - 8 * b)) : 0;
  }
  return 0;
}

// n tags: r, s n x 32 big-endian bytes -> tags n x 72 (prefilled by the
// caller: the encoder writes the whole slot), lens n.
int sign_check_der(const uint8_t* r, const uint8_t* s, int n, uint8_t* tags, uint8_t* lens) {
  for (int i = 0; i < n; i++) {
    uint32_t rw[8], sw[8];
    be_words(rw, r + 32 * i);
    be_words(sw, s + 32 * i);
    lens[i] = (uint8_t)mbft::der_encode_sig(tags + mbft::kTagSlot * i, rw, sw);
  }
  return 0;
}

// Digits of n scalars (k: n x 32 big-endian bytes) for window W: digits[i][j]
// = the signed digit of window j, j < sign_steps(W) (row stride 64).
int sign_check_recode(const uint8_t* k, int n, int W, int32_t* digits) {
  if (W < 4 || W > 6) return -1;
  const int S = mbft::sign_steps(W);
  for (int i = 0; i < n; i++) {
    uint32_t U[8];
    for (int j = 0; j < 8; j++) {
      const uint8_t* p = k + 32 * i + 4 * (7 - j);
      U[j] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    uint32_t carry = 0;
    for (int j = 0; j < S; j++) {
      bool neg;
      const uint32_t mag = mbft::sign_digit(U, carry, W, j + 1 == S, neg);
      if ((int)mag > mbft::sign_window_entries(W, j)) return -2;  // outside the table
      digits[64 * i + j] = neg ? -(int32_t)mag : (int32_t)mag;
    }
    if (carry) return -3;
  }
  return 0;
}

// The masked pick over a caller-made window of `count` entries (16 words
// each) for every |digit| in mags: out n x 16 words.
int sign_check_pick(const uint32_t* win, int count, const uint32_t* mags, int n, uint32_t* out) {
  for (int i = 0; i < n; i++) {
    uint32_t w[16];
    mbft::sign_pick(w, win, count, mags[i]);
    memcpy(out + 16 * i, w, 64);
  }
  return 0;
}

int sign_check_window_entries(int W, int step) { return mbft::sign_window_entries(W, step); }

}  // extern "C"
