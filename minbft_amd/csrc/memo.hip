// The verified-call memo's two stages (mbft_set_verified_memo; memo_plan.h,
// DESIGN.md §4.12): k_memo_probe in front of a pass's verify, k_memo_commit
// behind it.  A translation unit of its own: the verify kernels (verify_*.hip)
// are compiled exactly as without it.
//
// Passes on different lanes of one device share one table, so a commit may run
// beside another pass's probe.  The two errors that could follow are not equal:
// a probe that does not yet see an entry costs one more verify; a probe that
// saw a ready tag over a payload not yet whole could accept a tuple nobody
// verified.  So the hand-off is the conservative one.  The inserting wave:
// plain payload stores, s_waitcnt vmcnt(0), an agent-scope release fence, the
// wait again in inline assembly (the compiler may drop the fence's own), then
// the ready tag by an agent-scope atomic store.  The probing wave: the tags by
// agent-scope atomic loads; if any lane saw a matching ready tag, ONE
// agent-scope acquire fence, then the payload loads.  No spin, no acquire per
// probe step, a busy tag is a miss.  INVARIANT (memo_plan.h): between two
// clears an entry only goes empty -> busy -> ready; nothing overwrites a ready
// entry, and a clear runs only while no pass is in flight.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "memo_plan.h"
#include "minbft_gpu.h"

using namespace mbft;
using mbft_launch::MemoCommit;
using mbft_launch::MemoProbe;

namespace {

__device__ __forceinline__ int lane_rank(uint64_t mask) {  // the set bits of mask below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ void stat_add(uint64_t* stats, int which, uint64_t v) {
  if (stats && v) __hip_atomic_fetch_add(&stats[which], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 32 bytes of e, r or s as 8 words, as they lie in the batch
__device__ __forceinline__ void load32(const uint8_t* p, uint32_t* w) {
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
__device__ __forceinline__ void store32(uint8_t* p, const uint32_t* w) {
  reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// the exact compare: the entry's words 1 .. 25 against the tuple
__device__ __forceinline__ bool entry_equals(const uint32_t* ent, const uint32_t* w) {
  uint32_t v[28];
#pragma unroll
  for (int q = 0; q < 7; q++) {
    const uint4 x = reinterpret_cast<const uint4*>(ent)[q];
    v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
  }
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < kMemoTupleWords; k++) d |= v[1 + k] ^ w[k];
  return d == 0;
}

}  // namespace

__global__ void __launch_bounds__(256) k_memo_probe(MemoProbe P) {
  long n = P.n;
  if (P.ndev) {  // the count on the device: items past it are undefined
    const long nd = (long)*P.ndev;
    if (nd < n) n = nd;
  }
  const int lane = (int)(threadIdx.x & 63u);
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i - lane >= n) return;  // (the whole wave)
  const bool live = i < n;
  uint32_t w[kMemoTupleWords];
#pragma unroll
  for (int k = 0; k < kMemoTupleWords; k++) w[k] = 0;
  bool real = false;
  if (live) {
    w[0] = P.slot[i];
    load32(P.e + 32 * i, w + 1);
    load32(P.r + 32 * i, w + 9);
    load32(P.s + 32 * i, w + 17);
    real = w[0] < P.nslots && P.keys[w[0]].valid != 0u;  // (host-decided words are >= kHostSlot >= nslots)
  }
  // the tags of both probe sequences, relaxed; bit g * kMemoProbe + j: generation
  // g's step j holds this tuple's ready tag
  uint64_t h = 0;
  uint32_t cand = 0;
  if (real) {
    h = P.force_hash ? P.force_hash[i] : memo_hash(w);
    const uint32_t tag = memo_tag(h);
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const uint32_t* tab = g == 0 ? P.young : P.old;
#pragma unroll
      for (int j = 0; j < kMemoProbe; j++) {
        const uint32_t t = __hip_atomic_load(tab + memo_probe_at(h, j, P.entries) * kMemoEntryWords, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (t == tag) cand |= 1u << (g * kMemoProbe + j);
      }
    }
  }
  bool hit = false;
  if (__ballot(cand != 0u) != 0ull) {  // wave-uniform: ONE acquire in front of every payload load
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    while (cand != 0u && !hit) {
      const int b = __ffs((int)cand) - 1;
      cand &= cand - 1u;
      const uint32_t* tab = b < kMemoProbe ? P.young : P.old;
      hit = entry_equals(tab + memo_probe_at(h, b % kMemoProbe, P.entries) * kMemoEntryWords, w);
    }
  }
  if (hit) P.status[i] = (uint8_t)MBFT_ACCEPT;
  const uint64_t realm = __ballot(real), hitm = __ballot(hit);
  const bool miss = live && !hit;
  const uint64_t missm = __ballot(miss);
  uint32_t base = 0;
  if (lane == 0) {
    stat_add(P.stats, mbft_launch::kMemoStatLookups, (uint64_t)__popcll(realm));
    stat_add(P.stats, mbft_launch::kMemoStatHits, (uint64_t)__popcll(hitm));
    if (missm)
      base = __hip_atomic_fetch_add(P.miss, (uint32_t)__popcll(missm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  if (miss) {  // (at most n misses in all: j < n <= P.n)
    const size_t j = (size_t)base + (size_t)lane_rank(missm);
    P.slot_c[j] = w[0];
    P.origin[j] = (uint32_t)i;
    store32(P.e_c + 32 * j, w + 1);
    store32(P.r_c + 32 * j, w + 9);
    store32(P.s_c + 32 * j, w + 17);
  }
}

__global__ void __launch_bounds__(256) k_memo_commit(MemoCommit C) {
  long n = C.n;
  {
    const long nd = (long)*C.miss;
    if (nd < n) n = nd;
  }
  const int lane = (int)(threadIdx.x & 63u);
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j - lane >= n) return;  // (the whole wave)
  const bool live = j < n;
  uint32_t w[kMemoTupleWords];
#pragma unroll
  for (int k = 0; k < kMemoTupleWords; k++) w[k] = 0;
  bool want = false;
  if (live) {
    const uint8_t stc = C.status_c[j];
    const uint32_t o = C.origin[j];
    if ((long)o < C.n) C.status[o] = stc;
    w[0] = C.slot_c[j];
    want = stc == (uint8_t)MBFT_ACCEPT && w[0] < C.nslots && C.keys[w[0]].valid != 0u;
  }
  uint32_t* ent = nullptr;  // the entry this lane claimed
  uint32_t tag = 0;
  if (want) {
    load32(C.e_c + 32 * j, w + 1);
    load32(C.r_c + 32 * j, w + 9);
    load32(C.s_c + 32 * j, w + 17);
    const uint64_t h = C.force_hash ? C.force_hash[j] : memo_hash(w);
    tag = memo_tag(h);
#pragma unroll 1
    for (int q = 0; q < kMemoProbe && !ent; q++) {
      uint32_t* e = C.young + memo_probe_at(h, q, C.entries) * kMemoEntryWords;
      uint32_t expect = kMemoEmpty;
      if (__hip_atomic_compare_exchange_strong(e, &expect, kMemoBusy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        ent = e;
    }
    if (ent) {  // the payload: words 1 .. 25, then zero padding; word 0 stays busy
      ent[1] = w[0], ent[2] = w[1], ent[3] = w[2];
#pragma unroll
      for (int q = 1; q < 8; q++) {
        const int k = 4 * q - 1;  // entry word 4 q holds tuple word 4 q - 1
        reinterpret_cast<uint4*>(ent)[q] = make_uint4(k < kMemoTupleWords ? w[k] : 0u, k + 1 < kMemoTupleWords ? w[k + 1] : 0u,
                                                      k + 2 < kMemoTupleWords ? w[k + 2] : 0u,
                                                      k + 3 < kMemoTupleWords ? w[k + 3] : 0u);
      }
    }
  }
  const uint64_t insm = __ballot(ent != nullptr);
  if (insm != 0ull) {  // wave-uniform: this wave signals for its own stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (kept: the fence's own wait can be dropped)
    if (ent) __hip_atomic_store(ent, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const uint64_t wantm = __ballot(want);
  if (lane == 0) {
    stat_add(C.stats, mbft_launch::kMemoStatInserts, (uint64_t)__popcll(insm));
    stat_add(C.stats, mbft_launch::kMemoStatDropped, (uint64_t)__popcll(wantm & ~insm));
  }
}

namespace mbft_launch {

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool table_ok(const void* tab, uint64_t entries) {
  return tab && entries >= kMemoMinEntries && (entries & (entries - 1u)) == 0 &&
         (reinterpret_cast<uintptr_t>(tab) & (kMemoEntryBytes - 1u)) == 0;
}
}  // namespace

hipError_t memo_probe(const MemoProbe& p, hipStream_t st) {
  if (p.n <= 0) return hipSuccess;
  if (p.n > (long)0x7FFFFFFF || !p.e || !p.r || !p.s || !p.slot || !p.keys || !p.status || !p.e_c || !p.r_c ||
      !p.s_c || !p.slot_c || !p.origin || !p.miss || !table_ok(p.young, p.entries) || !table_ok(p.old, p.entries) ||
      !aligned16(p.e) || !aligned16(p.r) || !aligned16(p.s) || !aligned16(p.e_c) || !aligned16(p.r_c) ||
      !aligned16(p.s_c))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_memo_probe, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t memo_commit(const MemoCommit& c, hipStream_t st) {
  if (c.n <= 0) return hipSuccess;
  if (c.n > (long)0x7FFFFFFF || !c.e_c || !c.r_c || !c.s_c || !c.slot_c || !c.origin || !c.status_c || !c.miss ||
      !c.keys || !c.status || !table_ok(c.young, c.entries) || !aligned16(c.e_c) || !aligned16(c.r_c) ||
      !aligned16(c.s_c))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_memo_commit, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, st, c);
  return hipGetLastError();
}

}  // namespace mbft_launch
