// The verifier's lowest-latency form, one item per 256-thread workgroup:
// k_verify_split (split_item, split_dev.h) and its launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"
#include "kernels.h"
#include "verify_launch.h"

using namespace mbft;

#ifdef MBFT_SPLIT_TIMING
// Phase timestamps of the last split / resident item of workgroups 0 and 1
// (timing builds only, tools/split_timing.py, tools/resident_timing.py):
// [5 workgroup + wave][phase] wall clock (100 MHz), plus the shader clock at
// phases 0 and 7 of wave 0.  Phase 9: a wave's table entries are in
// (comb_range_uniform).
__device__ unsigned long long g_split_t[10][16];
__device__ unsigned long long g_split_clk[2];
extern "C" int mbft_debug_split_timing(unsigned long long out[162]) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_split_t), sizeof(g_split_t)) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out + 160, HIP_SYMBOL(g_split_clk), sizeof(g_split_clk)) != hipSuccess) return -1;
  return 0;
}
#endif

#include "split_dev.h"

// Small batches at the lowest latency (mbft_launch::verify, n <=
// MBFT_SPLIT_MAX, default 256 -- single calls, coalesced groups): ONE item
// per 256-thread workgroup, its 2 S comb windows split over the 4 waves
// (one per SIMD): wave 0 sums the low half of the G windows, wave 1 the high
// half, waves 2 and 3 the same for Q, at the same time; waves 0 and 2 then
// join the halves (full Chudnovsky additions) and wave 0 the two sums
// (x-only).  An item's latency is s^-1 (every wave inverts s itself with all
// its lanes, modinv_n_var_wave: no barrier) + ceil(S / 2) additions + two
// joins, instead of S additions + a join (k_verify_pairs) or 2 S.
// Degenerate additions or joins (u1 G == +-u2 Q, or crafted partial sums)
// take the exact path (verify_exact).  s^-1 per item (A.winv null), or
// the host's s^-1 R planes (A.winv: the lone calls' host inversion,
// batch.cpp host_winv -- ~2 us on the CPU against ~19 us for one wave).
template <bool WIDE>
__global__ void __launch_bounds__(256) k_verify_split(VerifyArgs A) {
  __shared__ uint32_t part[4][4 * NL + 1];
  __shared__ uint4 pre[4][4 * kSplitPre];  // each wave's prefetched table entries
#ifdef MBFT_SPLIT_TIMING
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0 && blockIdx.x == 0) g_split_clk[0] = clock64();
  SPLIT_T(0);
#endif
  const long i = blockIdx.x;
  if (A.ndev && i >= (long)*A.ndev) return;  // past the device count: block-uniform
  split_item<WIDE>(A, i, part, pre, nullptr, -1, A.uhost ? A.uhost + 16 * i : nullptr);
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h and verify_launch.h)
namespace mbft_launch {

// k_verify_split's additions: lane-group parallel (default) or sequential
// (env MBFT_SPLIT_WIDE=0)
bool split_wide() {
  static const bool w = env_on("MBFT_SPLIT_WIDE", true);
  return w;
}

long split_max_env() {
  static const long v = env_long("MBFT_SPLIT_MAX", 256L);
  return v;
}

template <bool WIDE>
static void launch_split(const VerifyArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_split<WIDE>, dim3((unsigned)A.n), dim3(256), 0, st, A);
}

void verify_split(const VerifyArgs& A, hipStream_t st) {
  if (split_wide())
    launch_split<true>(A, st);
  else
    launch_split<false>(A, st);
}

}  // namespace mbft_launch

// Timing builds: k_verify_server stamps the same g_split_t (split_item), and a
// device global belongs to one unit, so the resident kernels are compiled here.
#ifdef MBFT_SPLIT_TIMING
#define MBFT_IN_VERIFY_SPLIT
#include "verify_server.hip"
#endif
