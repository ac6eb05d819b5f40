// Per-key use counts (mbft_set_key_accounting): the stage that ends a verify
// batch while accounting is on.  A translation unit of its own: the verify
// kernels (verify_*.hip) are compiled exactly as without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "kernels.h"

using namespace mbft;
using mbft_launch::KeyAccount;

namespace {

__device__ __forceinline__ void account_add(const KeyAccount& A, uint32_t slot, uint32_t uses, uint32_t rejects) {
  __hip_atomic_fetch_add(&A.uses[slot], (uint64_t)uses, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (rejects)
    __hip_atomic_fetch_add(&A.rejects[slot], (uint64_t)rejects, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// One item per lane, grid-stride.  Equal slots are summed in the wave before
// any atomic: the first remaining lane's slot, a ballot of the lanes that hold
// it, the popcounts of that mask and of its rejects -- until no lane remains.
// Every value the loop turns on is wave-uniform (ballots, a read lane), so all
// 64 lanes walk it together.  The sums of the LAST slot a wave met stay in
// (uniform) registers from one grid-stride step to the next and are added to
// while the slot repeats: a wave that meets one signer issues one pair of
// atomics in all, a wave of 64 distinct signers 64 pairs a step.  At the end a
// block's four carries meet in LDS and equal slots go out as one pair.
__global__ void __launch_bounds__(256) k_key_account(KeyAccount A) {
  __shared__ uint32_t c_slot[4], c_uses[4], c_rej[4];
  long n = A.n;
  if (A.ndev) {  // the count on the device: statuses and slots past it are undefined
    const long nd = (long)*A.ndev;
    if (nd < n) n = nd;
  }
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const long stride = (long)gridDim.x * blockDim.x;
  uint32_t cur = 0, cur_uses = 0, cur_rej = 0;  // the wave's carry (cur_uses == 0: none)
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < n; base += stride) {
    const long i = base + threadIdx.x;
    uint32_t sl = 0;
    bool live = false, rej = false;
    if (i < n) {
      sl = A.slot[i];
      if (sl < A.nslots && A.keys[sl].valid != 0u) {  // (host-decided words are >= kHostSlot >= nslots)
        live = true;
        rej = A.status[i] != 0;  // MBFT_ACCEPT is 0
      }
    }
    uint64_t remain = __ballot(live);
    const uint64_t rejm = __ballot(live && rej);
    while (remain) {
      const int first = __ffsll((unsigned long long)remain) - 1;
      const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)sl, first);
      const uint64_t same = __ballot(live && sl == s0);
      const uint32_t u = (uint32_t)__popcll(same), r = (uint32_t)__popcll(same & rejm);
      if (cur_uses != 0 && cur == s0) {
        cur_uses += u;
        cur_rej += r;
      } else {
        if (cur_uses != 0 && lane == 0) account_add(A, cur, cur_uses, cur_rej);
        cur = s0;
        cur_uses = u;
        cur_rej = r;
      }
      remain &= ~same;
    }
  }
  if (lane == 0) {
    c_slot[wave] = cur;
    c_uses[wave] = cur_uses;
    c_rej[wave] = cur_rej;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      uint32_t u = c_uses[w], r = c_rej[w];
      if (u == 0) continue;
      for (int v = w + 1; v < 4; v++)
        if (c_uses[v] != 0 && c_slot[v] == c_slot[w]) {
          u += c_uses[v];
          r += c_rej[v];
          c_uses[v] = 0;
        }
      account_add(A, c_slot[w], u, r);
    }
  }
}

namespace mbft_launch {

hipError_t key_account(const KeyAccount& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (!a.slot || !a.status || !a.keys || !a.uses || !a.rejects) return hipErrorInvalidValue;
  // the CUs of the CURRENT device (engines of one context may sit on different parts), asked once each
  static std::atomic<int> cus_of[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
  int cus = dev >= 0 && dev < 64 ? cus_of[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;
    }
    if (dev >= 0 && dev < 64) cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  const long ncu = cus;
  const long blocks = key_account_blocks(a.n, ncu);
  hipLaunchKernelGGL(k_key_account, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace mbft_launch
