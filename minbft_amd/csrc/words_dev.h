// Device code every kernel unit of the P-256 library shares: 256-bit values as
// eight little-endian words or 32 big-endian bytes (load_words8, store_words8,
// load_be256, store_be256, store_point_words), the nine-limb SoA planes
// (plane_load, plane_store), and the curve's generator and b as words (kGxw,
// kGyw, kBw).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecc.h"

namespace mbft {

namespace {

// Generator and curve b as little-endian words (plain, canonical).
__constant__ uint32_t kGxw[8] = {0xD898C296u, 0xF4A13945u, 0x2DEB33A0u, 0x77037D81u,
                                 0x63A440F2u, 0xF8BCE6E5u, 0xE12C4247u, 0x6B17D1F2u};
__constant__ uint32_t kGyw[8] = {0x37BF51F5u, 0xCBB64068u, 0x6B315ECEu, 0x2BCE3357u,
                                 0x7C0F9E16u, 0x8EE7EB4Au, 0xFE1A7F9Bu, 0x4FE342E2u};
__constant__ uint32_t kBw[8] = {0x27D2604Bu, 0x3BCE3C3Eu, 0xCC53B0F6u, 0x651D06B0u,
                                0x769886BCu, 0xB3EBBD55u, 0xAA3A93E7u, 0x5AC635D8u};

MBFT_DEV void load_words8(uint32_t w[8], const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

MBFT_DEV void store_words8(uint32_t* p, const uint32_t w[8]) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// 32 big-endian bytes at p -> little-endian words
MBFT_DEV void load_be256(uint32_t w[8], const uint8_t* p) {
  uint32_t be[8];
  load_words8(be, reinterpret_cast<const uint32_t*>(p));
  be_words_to_le(w, be);
}

MBFT_DEV void store_point_words(uint32_t* dst, const fe& x, const fe& y) {
  uint32_t wx[8], wy[8];
  fe_to_words(wx, x);
  fe_to_words(wy, y);
  store_words8(dst, wx);
  store_words8(dst + 8, wy);
}

}  // namespace

MBFT_DEV void store_be256(uint8_t* p, const uint32_t w[8]) {
  uint32_t be[8];
#pragma unroll
  for (int i = 0; i < 8; i++) be[i] = __builtin_bswap32(w[7 - i]);
  store_words8(reinterpret_cast<uint32_t*>(p), be);
}

// Values as Montgomery-form limbs in 9 planes of n uint32 (SoA, coalesced):
// limb k of item i at planes[k * n + i].
MBFT_DEV void plane_load(fe& a, const uint32_t* planes, long n, long i) {
#pragma unroll
  for (int k = 0; k < NL; k++) a.v[k] = planes[k * n + i];
}

MBFT_DEV void plane_store(uint32_t* planes, long n, long i, const fe& a) {
#pragma unroll
  for (int k = 0; k < NL; k++) planes[k * n + i] = a.v[k];
}

}  // namespace mbft
