// asn1.Marshal(ecdsaSignature{R, S}) (sample/authentication/crypto.go:57-69)
// for ONE lane: the tag the batch signer (sign_kernels.hip, k_sign_tags)
// writes, and, compiled for the host, the encoder the CPU suite checks
// against oracle.der_encode_sig (tests/csrc/sign_check.cpp).  Byte-identical
// to the host encoder of mbft_generate_message_authen_tag (host.cpp).
//
// R and S are non-negative and below 2^256, so each INTEGER is its minimal
// big-endian bytes (at least one) with a 0x00 in front when the top bit of
// the first is set: at most 33 content bytes, the SEQUENCE body at most 70,
// every length in the short form, the tag at most 72 bytes (MBFT_TAG_SLOT).
//
// The values arrive as 8 big-endian-numeric words (w[0] = bytes 0..3) and are
// read at compile-time positions; only the DESTINATION index depends on the
// value, so on the GPU the encoder is predicated byte stores and needs no
// per-lane array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbft {

#define MBFT_DERE_HD __host__ __device__ __forceinline__

constexpr int kTagSlot = 72;

// leading zero bytes of the 32-byte value, at most 31 (zero encodes as 02 01 00)
MBFT_DERE_HD uint32_t der_enc_lead(const uint32_t w[8]) {
  uint32_t nz = 0;
  bool run = true;
#pragma unroll
  for (int j = 0; j < 31; j++) {
    const uint32_t b = (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu;
    run = run && b == 0;
    nz += run ? 1u : 0u;
  }
  return nz;
}

// 02 len [00] bytes at out[pos..]; returns the new position
MBFT_DERE_HD uint32_t der_enc_int(uint8_t* out, uint32_t pos, const uint32_t w[8]) {
  const uint32_t nz = der_enc_lead(w);
  uint32_t first = 0;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    const uint32_t b = (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu;
    first = (uint32_t)j == nz ? b : first;
  }
  const uint32_t pad = first >> 7;
  out[pos] = 0x02;
  out[pos + 1] = (uint8_t)(32u - nz + pad);
  if (pad) out[pos + 2] = 0x00;
  const uint32_t base = pos + 2 + pad;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    const uint32_t b = (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu;
    if ((uint32_t)j >= nz) out[base + (uint32_t)j - nz] = (uint8_t)b;
  }
  return base + 32u - nz;
}

// The whole tag into the kTagSlot-byte slot `out` (the bytes after the tag
// are zeroed); returns its length, 8 .. 72.
MBFT_DERE_HD uint32_t der_encode_sig(uint8_t* out, const uint32_t r[8], const uint32_t s[8]) {
  uint32_t pos = der_enc_int(out, 2, r);
  pos = der_enc_int(out, pos, s);
  out[0] = 0x30;
  out[1] = (uint8_t)(pos - 2u);
#pragma unroll
  for (int j = 8; j < kTagSlot; j++)
    if ((uint32_t)j >= pos) out[j] = 0;
  return pos;
}

}  // namespace mbft
