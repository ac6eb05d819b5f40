// The key memory budget's ranking (mbft_rebalance_keys, mbft_cold_keys,
// mbft_age_key_usage): the use counts are aged, binned and
// turned into lists of slots where they are, on the GPU -- the host sees a
// histogram and the slots that move, never the per-slot counters.  A
// translation unit of its own, as key_account.hip: the verify kernels
// (verify_*.hip) are compiled exactly as without it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "kernels.h"
#include "key_plan.h"

using namespace mbft;
using mbft_launch::KeyPickLists;
using mbft_launch::KeyRank;
using mbft_launch::kRankBins;
using mbft_launch::kRankHistOutside;
using mbft_launch::kRankHistWords;
using mbft_launch::kRankLadder;
using mbft_launch::kRankParts;

static_assert(kRankBins == kUseBins && (size_t)kRankLadder == kLadderMax, "kernels.h and key_plan.h agree");

namespace {

// Slot i of the store as the ranking sees it: its summed count, whether it is
// valid, and its rung (-1: its class is not on the ladder).
struct Ranked {
  uint64_t u;
  bool valid;
  int rung;
};
__device__ __forceinline__ Ranked rank_slot(const KeyRank& R, long i) {
  Ranked k{0, false, -1};
  const KeyDesc kd = R.keys[i];
  k.valid = kd.valid != 0u;
  if (!k.valid) return k;
#pragma unroll
  for (int p = 0; p < kRankParts; p++)
    if (p < R.nparts) k.u += R.part[p][i];
#pragma unroll
  for (int j = 0; j < kRankLadder; j++)
    if (j < R.nladder && R.ladder[j] == kd.wbits) k.rung = j;
  return k;
}

// The lanes of `mask` append their slot to list (cap entries): one atomicAdd a
// wave by the mask's first lane, every lane writes at its rank behind it.
// *count goes past cap where more belong on the list; nothing is written there.
// Called by all lanes of the wave together (mask is a ballot).
__device__ __forceinline__ void wave_append(uint64_t mask, bool mine, uint32_t slot, uint32_t* list, uint32_t cap,
                                            uint32_t* count, int lane) {
  if (!mask) return;
  const int first = __ffsll((unsigned long long)mask) - 1;
  uint32_t base = 0;
  if (lane == first)
    base = __hip_atomic_fetch_add(count, (uint32_t)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
  if (mine) {
    const uint32_t pos = base + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1u));
    if (pos < cap) list[pos] = slot;  // (a slot is appended once, so the counter stays below 2^32)
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_key_age(uint64_t* uses, uint64_t* rejects, size_t n, unsigned shift) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uses[i] >>= shift;
    rejects[i] >>= shift;
  }
}

__global__ void __launch_bounds__(256) k_key_add(uint64_t* dst, const uint64_t* src, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] += src[i];
}

// The block's histogram is kept in LDS (8 x 496 cells and the outside count,
// 15.5 KiB).  Equal cells of a wave are combined before the LDS add with
// k_key_account's loop -- the first remaining lane's cell, a ballot of the
// lanes that hold it, its popcount added once -- so a store whose keys all sit
// in one bin (no uses at all) costs a wave one LDS add a step, not 64 in a
// row.  Every value the loop turns on is wave-uniform.  At the end a block
// makes one global add per non-zero cell.
__global__ void __launch_bounds__(256) k_key_hist(KeyRank R, uint32_t* out) {
  __shared__ uint32_t h[kRankHistWords];
  for (int c = (int)threadIdx.x; c < kRankHistWords; c += 256) h[c] = 0;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  const long n = (long)R.nslots, stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < n; base += stride) {
    const long i = base + threadIdx.x;
    bool live = false;
    int cell = 0;
    if (i < n) {
      const Ranked k = rank_slot(R, i);
      live = k.valid;
      cell = k.rung < 0 ? kRankHistOutside : k.rung * kRankBins + key_use_bin(k.u);
    }
    uint64_t remain = __ballot(live);
    while (remain) {
      const int first = __ffsll((unsigned long long)remain) - 1;
      const int c0 = __builtin_amdgcn_readlane(cell, first);
      const uint64_t same = __ballot(live && cell == c0);
      if (lane == first) atomicAdd(&h[c0], (uint32_t)__popcll(same));
      remain &= ~same;
    }
  }
  __syncthreads();
  for (int c = (int)threadIdx.x; c < kRankHistWords; c += 256) {
    const uint32_t v = h[c];
    if (v) __hip_atomic_fetch_add(&out[c], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// rung_of_bin != null: plan mode; else cold mode (the list is L.list[0]).
__global__ void __launch_bounds__(256)
    k_key_pick(KeyRank R, const uint8_t* rung_of_bin, uint64_t max_uses, KeyPickLists L, uint32_t* count) {
  __shared__ uint8_t target_of[kRankBins];
  const bool plan = rung_of_bin != nullptr;
  if (plan)
    for (int b = (int)threadIdx.x; b < kRankBins; b += 256) target_of[b] = rung_of_bin[b];
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  const long n = (long)R.nslots, stride = (long)gridDim.x * blockDim.x;
#pragma unroll 1
  for (long base = (long)blockIdx.x * blockDim.x; base < n; base += stride) {
    const long i = base + threadIdx.x;
    Ranked k{0, false, -1};
    if (i < n) k = rank_slot(R, i);
    if (plan) {
      int target = -1;
      if (k.valid && k.rung >= 0) {
        target = (int)target_of[key_use_bin(k.u)];
        if (target == k.rung) target = -1;
      }
      for (int t = 0; t < R.nladder; t++) {
        const bool mine = target == t;
        wave_append(__ballot(mine), mine, (uint32_t)i, L.list[t], L.cap[t], &count[t], lane);
      }
    } else {
      const bool mine = k.valid && k.u <= max_uses;
      wave_append(__ballot(mine), mine, (uint32_t)i, L.list[0], L.cap[0], count, lane);
    }
  }
}

namespace mbft_launch {

namespace {

// the grid of n slots on the CURRENT device: k_key_account's (verify_plan.h), its CUs asked once each
hipError_t rank_blocks(size_t n, unsigned* blocks) {
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
  *blocks = (unsigned)key_account_blocks((long)n, (long)cus);
  return hipSuccess;
}

bool rank_ok(const KeyRank& r) {
  if (!r.keys || r.nparts < 0 || r.nparts > kRankParts || r.nladder < 0 || r.nladder > kRankLadder) return false;
  for (int p = 0; p < r.nparts; p++)
    if (!r.part[p]) return false;
  return true;
}

}  // namespace

hipError_t key_age(uint64_t* uses, uint64_t* rejects, size_t n, unsigned shift, hipStream_t st) {
  if (n == 0 || shift == 0) return hipSuccess;
  if (!uses || !rejects || shift > 63 || n > (size_t)1 << 40) return hipErrorInvalidValue;
  unsigned blocks = 0;
  if (const hipError_t e = rank_blocks(n, &blocks)) return e;
  hipLaunchKernelGGL(k_key_age, dim3(blocks), dim3(256), 0, st, uses, rejects, n, shift);
  return hipGetLastError();
}

hipError_t key_add(uint64_t* dst, const uint64_t* src, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!dst || !src || n > (size_t)1 << 40) return hipErrorInvalidValue;
  unsigned blocks = 0;
  if (const hipError_t e = rank_blocks(n, &blocks)) return e;
  hipLaunchKernelGGL(k_key_add, dim3(blocks), dim3(256), 0, st, dst, src, n);
  return hipGetLastError();
}

hipError_t key_hist(const KeyRank& r, uint32_t* out, hipStream_t st) {
  if (!out) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(out, 0, sizeof(uint32_t) * kRankHistWords, st)) return e;
  if (r.nslots == 0) return hipSuccess;
  if (!rank_ok(r)) return hipErrorInvalidValue;
  unsigned blocks = 0;
  if (const hipError_t e = rank_blocks(r.nslots, &blocks)) return e;
  hipLaunchKernelGGL(k_key_hist, dim3(blocks), dim3(256), 0, st, r, out);
  return hipGetLastError();
}

hipError_t key_pick_plan(const KeyRank& r, const uint8_t* rung_of_bin, const KeyPickLists& l, uint32_t* count,
                         hipStream_t st) {
  if (!count || !rung_of_bin) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t) * kRankLadder, st)) return e;
  if (r.nslots == 0) return hipSuccess;
  if (!rank_ok(r)) return hipErrorInvalidValue;
  for (int t = 0; t < r.nladder; t++)
    if (l.cap[t] != 0 && !l.list[t]) return hipErrorInvalidValue;
  unsigned blocks = 0;
  if (const hipError_t e = rank_blocks(r.nslots, &blocks)) return e;
  hipLaunchKernelGGL(k_key_pick, dim3(blocks), dim3(256), 0, st, r, rung_of_bin, (uint64_t)0, l, count);
  return hipGetLastError();
}

hipError_t key_pick_cold(const KeyRank& r, uint64_t max_uses, uint32_t* list, uint32_t cap, uint32_t* count,
                         hipStream_t st) {
  if (!count || (cap != 0 && !list)) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), st)) return e;
  if (r.nslots == 0) return hipSuccess;
  if (!rank_ok(r)) return hipErrorInvalidValue;
  KeyPickLists l{};
  l.list[0] = list;
  l.cap[0] = cap;
  unsigned blocks = 0;
  if (const hipError_t e = rank_blocks(r.nslots, &blocks)) return e;
  hipLaunchKernelGGL(k_key_pick, dim3(blocks), dim3(256), 0, st, r, (const uint8_t*)nullptr, max_uses, l, count);
  return hipGetLastError();
}

}  // namespace mbft_launch
