// The verifier's small-batch form, one item per lane pair: k_verify_pairs
// (verify_pair, pair_dev.h) and its launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_dev.h"
#include "verify_launch.h"

using namespace mbft;

// LANE_INV false: s^-1 R from the batched planes (A.winv, stride A.n).
template <bool LANE_INV>
__global__ void __launch_bounds__(256, 2) k_verify_pairs(VerifyArgs A) {
  __shared__ uint4 coop[4][256];  // per wave: 64 lanes x 64 B (per-lane gathers)
  uint4* buf = coop[threadIdx.x >> 6];
  const Spill sp{A.scr, blockIdx.x * blockDim.x + threadIdx.x, A.sstride};
  const long stride = (long)gridDim.x * blockDim.x;
  // the item count: n, or the device's (<= n) when the caller sized the grid
  // for an upper bound; a wave wholly past it leaves (per-wave buffers, no
  // block barrier in verify_pair)
  long n = A.n;
  if (A.ndev && (long)*A.ndev < n) n = (long)*A.ndev;
  const long wave0 = (long)(threadIdx.x & ~63u);
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < 2 * n; base += stride) {
    if (base + wave0 >= 2 * n) break;
    const long t = base + threadIdx.x;
    verify_pair<LANE_INV>(A, t >> 1, (int)(t & 1), (t >> 1) < n, buf, sp);
  }
}

namespace mbft_launch {

void verify_pairs(const VerifyArgs& A, bool lane_inv, dim3 grid, hipStream_t st) {
  if (lane_inv)
    hipLaunchKernelGGL(k_verify_pairs<true>, grid, dim3(256), 0, st, A);
  else
    hipLaunchKernelGGL(k_verify_pairs<false>, grid, dim3(256), 0, st, A);
}

}  // namespace mbft_launch
