// The P-384 class (mbft_verify_prehashed_p384_keys*): ECDSA
// over secp384r1 under keys that stand beside the items.  A translation unit
// of its own: nothing here is shared with the P-256 kernel units but the launch plan.
//
//   k_verify_p384   one item per lane, 256-thread blocks, grid-stride: the
//                   lane validates its key, inverts s itself, runs the joint
//                   double-and-add over the complete formulas (p384_ecc.h) and
//                   writes one status byte.  No LDS, no queue, no second
//                   kernel: the formulas have no degenerate case to hand on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "p384_ecc.h"

namespace mbft {

struct P384Args {
  const uint8_t *e, *r, *s, *xy;  // n x 48, 48, 48, 96 bytes, big-endian, 16-byte aligned
  long n;
  uint8_t* status;
};

// 48 big-endian bytes at a 16-byte aligned address -> 12 little-endian words
__device__ __forceinline__ void load_be48(uint32_t w[12], const uint8_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint4 v = q[k];
    w[11 - 4 * k] = __builtin_bswap32(v.x);
    w[10 - 4 * k] = __builtin_bswap32(v.y);
    w[9 - 4 * k] = __builtin_bswap32(v.z);
    w[8 - 4 * k] = __builtin_bswap32(v.w);
  }
}

__global__ void __launch_bounds__(256) k_verify_p384(P384Args A) {
  const long stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride) {
    uint32_t e[12], r[12], s[12], x[12], y[12];
    load_be48(e, A.e + 48 * i);
    load_be48(r, A.r + 48 * i);
    load_be48(s, A.s + 48 * i);
    load_be48(x, A.xy + 96 * i);
    load_be48(y, A.xy + 96 * i + 48);
    A.status[i] = p384_verify_item(e, r, s, x, y);
  }
}

}  // namespace mbft

namespace mbft_launch {

hipError_t verify_p384(const P384Batch& b, const mbft::P384Plan& plan, hipStream_t st) {
  if (b.n <= 0 || plan.blocks <= 0) return hipSuccess;
  const mbft::P384Args A{b.e, b.r, b.s, b.xy, b.n, b.status};
  hipLaunchKernelGGL(mbft::k_verify_p384, dim3((unsigned)plan.blocks), dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace mbft_launch
