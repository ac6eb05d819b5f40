// k_sign_tags: the batch GenerateMessageAuthenTag of the ECDSA roles
// (sample/authentication/crypto.go:57-76 ecdsaSigCipher.Sign, reached from
// authenticator.go GenerateMessageAuthenTag; api/api.go:133-144), one tag per
// lane, fit for a key that protects something -- unlike k_sign (kernels.hip),
// whose comb gathers table entries at nonce-dependent addresses.
//
// Per lane, from the digest input e and the role's private key d:
//   k      RFC 6979 3.2, HMAC-SHA-256 (sign_dev.h), at most kSignTries
//          candidates;
//   R = kG a signed fixed-window comb over a small dedicated generator table
//          (window 4..6: 33 / 52 / 87 KB, the layout of k_table_fill), one
//          mixed addition per window, unconditionally (sign_comb below);
//   r      x(R) mod N, with 1 / Z by the fixed-exponent fe_inv;
//   s      k^-1 (e + r d) mod N, with k^-1 by the fixed-exponent fn_inv;
//   tag    asn1.Marshal(ecdsaSignature{r, s}) (der_enc_dev.h) into the lane's
//          72-byte slot, its length into tag_len.
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
// digits and this property on the host build of sign_digit.)
//
// The steps from the key's load to (r, s) are one device function, sign_rs,
// shared with k_usig_uis (the software USIG's CreateUI, further down; DESIGN.md
// 4.6) and, for the comb alone, with k_sign_pubkey.
//
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "authen_dev.h"
#include "der_enc_dev.h"
#include "ecc.h"
#include "kernels.h"
#include "minbft_gpu.h"
#include "sha256_dev.h"
#include "sign_dev.h"
#include "sign_kernels.h"

using namespace mbft;

namespace {

// SHA256("") as big-endian-numeric words: the tail of the quirk digest
// (crypto.go:114,121: e = (m || SHA256(""))[0:32])
__constant__ uint32_t kEmptyW[8] = {0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u,
                                    0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u};
// N as big-endian-numeric words
__constant__ uint32_t kNbe[8] = {0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                 0xBCE6FAADu, 0xA7179E84u, 0xF3B9CAC2u, 0xFC632551u};

// 32 bytes at p (4-byte aligned) as big-endian-numeric words
MBFT_DEV void load_be_words(uint32_t w[8], const uint8_t* p) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(q[j]);
}

// e = (msg || SHA256(""))[0:32] for a raw message of any length (len < 32
// included), byte loads
MBFT_DEV void quirk_e(uint32_t (&e)[8], const uint8_t* msg, uint32_t len) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint32_t k = 4u * j + b;
      uint32_t byte;
      if (k < len) {
        byte = msg[k];
      } else {
        const uint32_t t = k - len;
        byte = (kEmptyW[t >> 2] >> (24 - 8 * (t & 3))) & 0xFFu;
      }
      w = (w << 8) | byte;
    }
    e[j] = w;
  }
}

// e of one message record (messages/authen.go:27-76 + the quirk digest):
// REQUEST and REPLY through authen_digest, REQ-VIEW-CHANGE = "REQ-VIEW-CHANGE"
// || new_view_be64 || SHA256("")[0:9] (authen.go:40-41,71-72: 23 bytes).
MBFT_DEV void record_e(uint32_t (&e)[8], const mbft_msg_rec& m, const uint8_t* bytes) {
  if (m.type == MBFT_MSG_REQ_VIEW_CHANGE) {
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = 0;
    put_str(e, 0, "REQ-VIEW-CHANGE", 15);
    put_be(e, 15, m.view, 8);
    put_h(e, 23, kEmptyW, 9);
    return;
  }
  uint32_t h[8];
  sha256_msg(h, m.op_len ? bytes + m.op_off : bytes, m.op_len);
  if (m.type == MBFT_MSG_REQUEST)
    authen_digest(e, kAuthenRequest, h, m.seq, m.client_id, 0, 0, 0, 0, 0);
  else
    authen_digest(e, kAuthenReply, h, m.seq, m.client_id, 0, 0, 0, 0, 0);
}

// acc = k G for 1 <= k < N (little-endian words), uniform access: see the
// header of this file.  tab: the signer's generator table for window W.
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

  uint32_t q[8];
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = kNbe[j];
  Rfc6979 g;
  g.init(db, eb, q);
#pragma unroll
  for (int j = 0; j < 8; j++) { rb[j] = 0; sb[j] = 0; }
  bool ok = false;
  int left = kSignTries;
  uint32_t kb[8];
#pragma unroll 1
  while (rfc6979_next(g, q, kb, left)) {
    uint32_t kw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) kw[j] = kb[7 - j];
    jac R;
    sign_comb(R, kw, tab, W);
    fe zi, x;
    fe_inv(zi, R.Z);
    fe_sqr(zi, zi);
    fe_mul(x, R.X, zi);
    fe_from_mont(x, x);
    fe_canon(x);
    fn_canon(x);  // r = x mod N (x < p < 2N)
    uint32_t rw[8];
    fe_to_words(rw, x);
    // s = k^-1 (e + r d) mod N
    fe k, kinv, t, rd;
    fe_from_words(k, kw);
    fn_to_mont(kinv, k);
    fn_inv(kinv, kinv);
    fn_mul(rd, x, dm_n);  // r d (plain)
    fe_add(t, e, rd);
    fn_canon(t);
    fn_mul(t, t, kinv);
    fn_canon(t);
    uint32_t sw[8];
    fe_to_words(sw, t);
    if (!words_is_zero(rw) && !words_is_zero(sw)) {
#pragma unroll
      for (int j = 0; j < 8; j++) { rb[j] = rw[7 - j]; sb[j] = sw[7 - j]; }
      ok = true;
      break;
    }
    g.retry();  // RFC 6979 3.2 h.3 for a discarded candidate
  }
  return ok;
}

}  // namespace

__global__ void __launch_bounds__(256) k_sign_tags(mbft_launch::SignTagArgs A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  // digest input e and the key of the lane's role (public: the message kind)
  uint32_t eb[8];
  const uint8_t* key = A.key0;
  if (A.mode == mbft_launch::kSignPrehashed) {
    load_be_words(eb, A.e + 32 * i);
  } else if (A.mode == mbft_launch::kSignFlat) {
    const uint32_t a = A.msg_off[i], b = A.msg_off[i + 1];
    quirk_e(eb, A.msgs + a, b - a);
  } else {
    const mbft_msg_rec m = A.recs[i];
    record_e(eb, m, A.bytes);
    if (m.type == MBFT_MSG_REQUEST) key = A.key1;
  }
  uint32_t rb[8], sb[8];
  const bool ok = sign_rs(rb, sb, key, eb, A.tab, A.w);
  uint8_t* out = A.tags + (size_t)kTagSlot * i;
  if (ok) {
    A.tag_len[i] = (uint8_t)der_encode_sig(out, rb, sb);
  } else {
#pragma unroll 1
    for (int j = 0; j < kTagSlot; j++) out[j] = 0;
    A.tag_len[i] = 0;
  }
}

// k_usig_uis: the software USIG's CreateUI (usig/sgx/enclave/usig.c:36-76
// ecall_usig_create_ui, reached through usig/sgx/sgx-usig.go:52-64 CreateUI),
// one UI per lane.  Lane i holds counter first + i; epoch, counter, message
// bytes and lengths are public, so the hash side may branch on them:
//   SHA256(m)  given, or of a raw message (sha256_msg), or of the PREPARE /
//              COMMIT AuthenBytes of a record (authen_dev.h: 59 / 70 bytes);
//   e          SHA256(SHA256(m) || epoch_le64 || counter_le64) (sgx-usig.go:
//              99-101, usig-enclave.go:204-214), one compression;
//   (r, s)     sign_rs, the signer of k_sign_tags: the key is loaded only
//              after e is complete, and the uniform-access property stated at
//              the head of this file holds from there on unchanged;
//   UI         counter_be64 || epoch_be64 || asn1.Marshal{R, S} into the lane's
//              88-byte slot (usig_ui_write), its length into ui_len; the whole
//              slot zeroed and length 0 when no candidate was usable.
// The host (sign.cpp) owns the counter: it hands a range to one launch at a
// time and advances only after every UI of the range came back.
__global__ void __launch_bounds__(256) k_usig_uis(mbft_launch::UsigArgs A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint64_t counter = A.first + (uint64_t)i;
  uint32_t eb[8];
  if (A.mode == mbft_launch::kUsigRecords) {
    const mbft_msg_rec m = A.recs[i];
    uint32_t h[8];
    sha256_msg(h, m.op_len ? A.bytes + m.op_off : A.bytes, m.op_len);
    authen_digest(eb, m.type == MBFT_MSG_PREPARE ? kAuthenPrepare : kAuthenCommit, h, m.seq, m.client_id,
                  m.view, m.prep_replica_id, m.prep_ui_counter, A.epoch, counter);
  } else {
    uint32_t dig[8];
    if (A.mode == mbft_launch::kUsigDigests) {
      load_be_words(dig, A.digests + 32 * i);
    } else {
      const uint32_t a = A.msg_off[i], b = A.msg_off[i + 1];
      sha256_msg(dig, A.msgs + a, b - a);
    }
    sha256_usig_chain(eb, dig, A.epoch, counter);
  }
  uint32_t rb[8], sb[8];
  const bool ok = sign_rs(rb, sb, A.key, eb, A.tab, A.w);
  uint8_t* out = A.uis + (size_t)kUiSlot * i;
  if (ok) {
    A.ui_len[i] = (uint8_t)usig_ui_write(out, counter, A.epoch, rb, sb);
  } else {
#pragma unroll 1
    for (int j = 0; j < kUiSlot; j++) out[j] = 0;
    A.ui_len[i] = 0;
  }
}

// k_sign_pubkey: affine d G of the secret d at `key` (0 < d < N, checked by
// the host), X || Y big-endian, for the USIG identity (sgx-usig.go:105-139:
// the enclave's public key).  One lane; d goes through sign_comb like a
// nonce, never through k_sign or a gather table, and 1 / Z is the
// fixed-exponent fe_inv.  d G is finite for 0 < d < N (the comb's argument at
// the head of this file), so Z != 0.
__global__ void __launch_bounds__(64) k_sign_pubkey(const uint8_t* key, const uint32_t* tab, int W,
                                                    uint8_t* xy) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t db[8], dw[8];
  load_be_words(db, key);
#pragma unroll
  for (int j = 0; j < 8; j++) dw[j] = db[7 - j];
  jac R;
  sign_comb(R, dw, tab, W);
  fe zi, zi2, x, y;
  fe_inv(zi, R.Z);
  fe_sqr(zi2, zi);
  fe_mul(x, R.X, zi2);
  fe_mul(zi2, zi2, zi);
  fe_mul(y, R.Y, zi2);
  fe_from_mont(x, x);
  fe_canon(x);
  fe_from_mont(y, y);
  fe_canon(y);
  uint32_t xw[8], yw[8];
  fe_to_words(xw, x);
  fe_to_words(yw, y);
  uint32_t* o = reinterpret_cast<uint32_t*>(xy);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    o[j] = __builtin_bswap32(xw[7 - j]);
    o[8 + j] = __builtin_bswap32(yw[7 - j]);
  }
}

namespace mbft_launch {

hipError_t usig_uis(const UsigArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.w < kSignMinWindow || a.w > kSignMaxWindow) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_usig_uis, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t sign_pubkey(const uint8_t* key, const uint32_t* tab, int w, uint8_t* xy, hipStream_t st) {
  if (w < kSignMinWindow || w > kSignMaxWindow) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sign_pubkey, dim3(1), dim3(64), 0, st, key, tab, w, xy);
  return hipGetLastError();
}

hipError_t sign_tags(const SignTagArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.w < kSignMinWindow || a.w > kSignMaxWindow) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sign_tags, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace mbft_launch
