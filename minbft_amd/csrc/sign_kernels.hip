// k_sign_tags: the batch GenerateMessageAuthenTag of the ECDSA roles
// (sample/authentication/crypto.go:57-76 ecdsaSigCipher.Sign, reached from
// authenticator.go GenerateMessageAuthenTag; api/api.go:133-144), one tag per
// lane, fit for a key that protects something -- unlike k_sign (prep_kernels.hip),
// whose comb gathers table entries at nonce-dependent addresses.
//
// Per lane, from the digest input e and the role's private key d:
//   k      RFC 6979 3.2, HMAC-SHA-256 (sign_dev.h), at most kSignTries
//          candidates;
//   R = kG a signed fixed-window comb over a small dedicated generator table
//          (window 4..6: 33 / 52 / 87 KB, the layout of k_table_fill), one
//          mixed addition per window, unconditionally (sign_comb);
//   r      x(R) mod N, with 1 / Z by the fixed-exponent fe_inv;
//   s      k^-1 (e + r d) mod N, with k^-1 by the fixed-exponent fn_inv;
//   tag    asn1.Marshal(ecdsaSignature{r, s}) (der_enc_dev.h) into the lane's
//          72-byte slot, its length into tag_len.
//
// The signer itself -- everything from the key's load to (r, s) and the bytes
// of a tag or a UI -- is sign_rs_dev.h: sign_rs, shared with k_usig_uis (the
// software USIG's CreateUI, further down) and, for the comb
// alone, with k_sign_pubkey, and the two tails sign_tag_finish /
// usig_ui_finish.  The uniform-access and no-degenerate-addition arguments
// stand there, with the code they describe.  Here: the hashing of public
// bytes into the digest input e, the kernels and their launchers.
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
#include "sign_rs_dev.h"

using namespace mbft;

namespace {

// SHA256("") as big-endian-numeric words: the tail of the quirk digest
// (crypto.go:114,121: e = (m || SHA256(""))[0:32])
__constant__ uint32_t kEmptyW[8] = {0xe3b0c442u, 0x98fc1c14u, 0x9afbf4c8u, 0x996fb924u,
                                    0x27ae41e4u, 0x649b934cu, 0xa495991bu, 0x7852b855u};

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
  sign_tag_finish(A.tags + (size_t)kTagSlot * i, A.tag_len + i, ok, rb, sb);
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
  usig_ui_finish(A.uis + (size_t)kUiSlot * i, A.ui_len + i, ok, counter, A.epoch, rb, sb);
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
