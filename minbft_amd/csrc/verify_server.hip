// The resident single-call verifier: k_verify_server (a pool of server
// workgroups over the host-mapped mailbox; split_item, split_dev.h) and its
// launcher.  (-DMBFT_SPLIT_TIMING builds compile it inside verify_split.hip,
// which owns the stamps' device global.)
#if !defined(MBFT_SPLIT_TIMING) || defined(MBFT_IN_VERIFY_SPLIT)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "split_dev.h"
#include "verify_launch.h"

using namespace mbft;

// The resident single-call verifier (kernels.h SrvSlot; host side in
// resident.cpp): a POOL of server workgroups for the mailbox slots.  A post
// is 1 or 2 jobs (TWO: one per scalar, u1 G and u2 Q, each on its own
// workgroup and CU; else the whole item).  Wave 0 of every idle server
// polls the doorbell line (one 64-B system-scope read over PCIe: slot b's
// post tag in byte b) and the claim words (device memory, agent scope); a
// job is open when slot b's tag is the successor of its claim (tags step
// 1..255 per post, so a stale read of either never re-opens a job), and the
// server takes it with one compare-and-swap of the claim.  It then copies
// the 256-B slot into LDS (one round trip, after a system-scope acquire: the
// host writes the slot, then its seq, then its tag), runs the job with
// split_item from that copy, and writes (seq << 8) | status to the job's
// done word (system-scope release).  A server count below 2 x slots keeps
// the resident kernel's VGPRs off most CUs: C2 batches beside it lost 16 %
// with one workgroup pair per slot at 32 slots.  Every
// workgroup leaves its loop when the host posts stop_gen == gen, when
// workgroup 0 has told this generation to exit (dexit[0] == gen: no post
// for idle_ticks, or life_ticks since its start; it also writes exited_gen
// so the host relaunches on the next call), or -- a workgroup whose
// workgroup 0 was never scheduled -- past life_ticks plus a grace; so every
// wave reaches an exit.  A claimed job is always finished first.
constexpr uint64_t kSrvGraceTicks = 10000000ull;  // 100 ms at 100 MHz

MBFT_DEV uint32_t sys_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Release at system scope, spelled out: this wave's stores done, the L2
// written back, and the write-back itself waited for.  The compiler's own
// release before a store (__ATOMIC_RELEASE, system scope) emits the L2
// write-back but drops the wait after it when no store of the wave is
// outstanding at that point (the waitcnt pass does not count the write-back):
// with the partial sums' stores already waited for by the barrier before
// thread 0's done word, the done word could reach the host ahead of them --
// measured as 1-7 wrong statuses in 2000 resident calls (tools/resident_probe.py
// gate), none with this sequence.  A vector-memory write-back (no scalar
// cache operation).
MBFT_DEV void sys_release() {
  asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_wbl2 sc0 sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
}

// A word the host polls (done, exited_gen), after sys_release.
MBFT_DEV void sys_store(uint32_t* p, uint32_t v) {
  sys_release();
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The post tag after t (tags 1..255 in turn; kernels.h srv_tag).
MBFT_DEV uint32_t srv_next_tag(uint32_t t) { return t % 255u + 1u; }

// TWO: jobs are scalars (half 0: u1 G, half 1: u2 Q), four waves over the
// scalar's windows, a range of three leaving its last entry as a partial of
// its own (so at G / key windows >= 26 no mixed addition runs: one affine +
// affine addition per wave), done word done[b][8 half] and 8 partial sums
// (part[b][320 half ..]); else one job per item, both scalars, four partial
// sums.
// The server's VGPRs are capped for 3 waves per SIMD (168; ~108 B of
// scratch per lane), so a CU holding a server workgroup still holds two
// k_verify workgroups beside it: uncapped (205 VGPRs) it held one, and 16
// servers cost a C2 batch stream ~2/3 of 16 CUs instead of ~1/3
// (tools/resident_ab.py; build flag -DMBFT_SRV_WAVES=0: uncapped).
#if !defined(MBFT_SRV_WAVES) || MBFT_SRV_WAVES == 3
#define MBFT_SRV_ATTR __attribute__((amdgpu_waves_per_eu(3)))
#else
#define MBFT_SRV_ATTR
#endif
template <bool WIDE, bool TWO>
__global__ void __launch_bounds__(256) MBFT_SRV_ATTR k_verify_server(ServerArgs S) {
  constexpr int NP = TWO ? 8 : 4;
  __shared__ uint32_t part[NP][4 * NL + 1];
  __shared__ uint4 pre[4][4 * kSplitPre];
  __shared__ uint4 item4[sizeof(SrvSlot) / 16];  // the job's slot, copied from the mailbox
  __shared__ uint32_t cmd[3];
  __shared__ uint8_t st_lds[4];  // the item's status (split_item writes it through A.status)
  uint32_t* item = reinterpret_cast<uint32_t*>(item4);
  uint64_t* act = reinterpret_cast<uint64_t*>(S.dexit + 2);
  const uint64_t t0 = wall_clock64();
  const uint32_t lane = threadIdx.x & 63u;
  // idle servers seeing one post take different halves first
  const uint32_t pref = TWO ? (blockIdx.x & 1u) : 0u;
  uint32_t iter = 0;
#pragma unroll 1
  for (;;) {
    if (threadIdx.x < 64) {
      uint32_t c = 0, jb = 0, jh = 0;
#pragma unroll 1
      for (;;) {
        const bool mine = lane < S.nslots;
        const uint32_t w = sys_load(&S.ctl->tag32[lane >> 2]);
        const uint32_t c0 = mine ? __hip_atomic_load(&S.claim[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : 0u;
        const uint32_t c1 = TWO && mine ? __hip_atomic_load(&S.claim[kSrvMaxSlots + lane], __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)
                                        : 0u;
        const uint32_t tg = (w >> (8u * (lane & 3u))) & 0xFFu;
        const bool open0 = mine && tg != 0u && tg == srv_next_tag(c0);
        const bool open1 = TWO && mine && tg != 0u && tg == srv_next_tag(c1);
        const uint64_t m0 = __ballot(open0), m1 = TWO ? __ballot(open1) : 0ull;
        bool got = false;
        if (m0 | m1) {
#pragma unroll 1
          for (uint32_t k = 0; k < (TWO ? 2u : 1u) && !got; k++) {
            const uint32_t h = TWO ? (k == 0 ? pref : 1u - pref) : 0u;
            uint64_t mm = h ? m1 : m0;
#pragma unroll 1
            while (mm && !got) {
              const uint32_t b = (uint32_t)__builtin_ctzll(mm);
              mm &= mm - 1;
              uint32_t ok = 0;
              if (lane == b) {
                uint32_t exp = h ? c1 : c0;
                ok = __hip_atomic_compare_exchange_strong(&S.claim[h * kSrvMaxSlots + b], &exp, tg,
                                                          __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT)
                         ? 1u
                         : 0u;
              }
              if (__builtin_amdgcn_readlane(ok, b)) {
                got = true;
                jb = b;
                jh = h;
              }
            }
          }
        }
        if (got) {
          c = 1;
          break;
        }
        // the stop and exit words and the clock (s_memrealtime: microseconds
        // of latency; read before every poll it cost ~5 us a call) every 8th
        // poll, so a poll is one PCIe read
        if ((++iter & 7u) != 0) {
#pragma unroll 1
          for (uint32_t z = 0; z < S.poll_sleep; z++) __builtin_amdgcn_s_sleep(8);
          continue;
        }
        if (sys_load(&S.ctl->stop_gen) == S.gen ||
            __hip_atomic_load(&S.dexit[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S.gen) {
          c = 2;
          break;
        }
        const uint64_t now = wall_clock64();
        if (blockIdx.x == 0) {
          const uint64_t a = __hip_atomic_load(act, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t since = a > t0 ? a : t0;
          if (now - since > S.idle_ticks || now - t0 > S.life_ticks) {
            if (lane == 0) {
              __hip_atomic_store(&S.dexit[0], S.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              sys_store(&S.ctl->exited_gen, S.gen);
            }
            c = 2;
            break;
          }
        } else if (now - t0 > S.life_ticks + kSrvGraceTicks) {
          c = 2;
          break;
        }
#pragma unroll 1
        for (uint32_t z = 0; z < S.poll_sleep; z++) __builtin_amdgcn_s_sleep(8);
      }
      if (lane == 0) {
        cmd[0] = c;
        cmd[1] = jb;
        cmd[2] = jh;
      }
    }
    __syncthreads();
    const uint32_t c = cmd[0], b = cmd[1], h = cmd[2];
    if (c == 2) break;  // workgroup-uniform
#ifdef MBFT_SRV_TIMING
    const uint64_t ts0 = wall_clock64();
#endif
    // The slot, one word a lane, read only after its tag was seen: the host
    // writes the fields and the seq before the tag, and a read issued after
    // the tag's read completed sees them.
    if (threadIdx.x < 64) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope
      item[threadIdx.x] = reinterpret_cast<const uint32_t*>(S.slots + b)[threadIdx.x];
    }
    __syncthreads();
#ifdef MBFT_SRV_TIMING
    const uint64_t ts1 = wall_clock64();
#endif
    const SrvSlot* it = reinterpret_cast<const SrvSlot*>(item4);
    const uint32_t q = it->seq & 0xFFFFFFu;
    const int dw = TWO ? 8 * (int)h : 0;  // this job's done word in the slot's line
    VerifyArgs A{it->e, it->r, it->s, &it->key0, it->winv, it->tabG, &it->kd, 1u, (int)it->wg, 1,
                 st_lds, nullptr, nullptr, 0u, nullptr, 0u, nullptr};
    if (it->gjoin) {
      // the whole item on its first job, joins and x test included
      // (k_verify_split's path): a final status, no partials -- for posts of
      // many items at once, whose joins would queue on the caller's one
      // thread; the second job only answers
      if (!TWO || h == 0)
        split_item<WIDE, 4, false>(A, 0, *reinterpret_cast<uint32_t(*)[4][4 * NL + 1]>(&part[0][0]), pre, nullptr, -1,
                            it->ugiven ? it->u : nullptr);
      else if (threadIdx.x == 0)
        st_lds[0] = kSrvPartials;
    } else {
      split_item<WIDE, NP, false>(A, 0, part, pre, S.ctl->part[b] + (TWO ? 40 * NP * h : 0), TWO ? (int)h : -1,
                           it->ugiven ? it->u : nullptr);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // the status came from wave 0, this thread's own wave
      const uint32_t st = *static_cast<volatile uint8_t*>(st_lds);
#ifdef MBFT_SRV_TIMING
      // (the done word's cache line has room)
      const uint64_t ts2 = wall_clock64();
      uint32_t* tw = &S.ctl->done[b][dw + 1];
      tw[0] = (uint32_t)(ts1 - ts0);
      tw[1] = (uint32_t)(ts2 - ts1);
#endif
      sys_store(&S.ctl->done[b][dw], (q << 8) | st);
      __hip_atomic_store(act, wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();  // cmd and the LDS item are reused by the next poll
  }
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h and verify_launch.h)
namespace mbft_launch {

hipError_t verify_server(const ServerArgs& a, int servers, bool two, hipStream_t st) {
  if (a.nslots == 0 || a.nslots > (uint32_t)kSrvMaxSlots || servers <= 0 || servers > 2 * kSrvMaxSlots)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)servers), block(256);
  if (two) {
    if (split_wide())
      hipLaunchKernelGGL((k_verify_server<true, true>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((k_verify_server<false, true>), grid, block, 0, st, a);
  } else {
    if (split_wide())
      hipLaunchKernelGGL((k_verify_server<true, false>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((k_verify_server<false, false>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace mbft_launch
#endif
