// Batched scalar inversion s^-1 mod N (Montgomery's trick): the level chain
// (k_ninv_up, k_ninv_top, k_ninv_down) and the one-launch forms per wave
// (k_ninv_local) and per workgroup (k_ninv_block), with their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "ecc.h"
#include "kernels.h"
#include "modinv.h"
#include "scalar_dev.h"
#include "verify_launch.h"
#include "words_dev.h"

using namespace mbft;

// ---------------------------------------------------------------------------
// Batched inversion mod N (Montgomery's trick).  Values are Montgomery-form
// limbs stored as 9 planes of n uint32 (SoA, coalesced).  Level structure:
// thread g of a level with G groups owns items g, g+G, g+2G, ... (strided so
// that each step of the chain is a coalesced access); it writes the running
// prefix products over its chain in place of nothing (prefix array) and the
// chain total into the next level's input.

// The chain kernels run beside the previous batch's verify kernel (DESIGN.md
// §4): s_setprio(3) gives their few waves issue priority on the SIMDs they
// share with verify waves, so the latency-bound chain is not slowed 3-4x by
// round-robin issue; the verify kernel loses only the slots these waves use.
#define MBFT_CHAIN_PRIO() __builtin_amdgcn_s_setprio(3)

// s (32 BE bytes) of item i as a PLAIN value; out-of-range s -> 1 (the
// verifier rejects those items on the range check before using w).
//
// The chains run Montgomery's trick on plain values with Montgomery
// multiplies (x*y/R): prefix p_k = p_(k-1) s_k / R from p_0 = R, and the
// root hands down P^-1 R for its chain total P.  Then in the down-sweep
// r = p_k^-1 R gives mont(p_(k-1), r) = s_k^-1 R -- exactly the Montgomery
// form of w the verifier multiplies e and r by -- and mont(r, s_k) =
// p_(k-1)^-1 R for the next item.  No per-item conversion to Montgomery form.
MBFT_DEV void s_plain(fe& a, const uint8_t* s, long i) {
  uint32_t w[8];
  load_be256(w, s + 32 * i);
  const bool ok = !words_is_zero(w) && words_lt(w, kNw);
  fe_from_words(a, w);
  if (!ok) {
    fe_zero(a);
    a.v[0] = 1;
  }
}

// Level-l up-sweep.  in: x[n] (planes), or the raw s bytes at level 0;
// out: pre[n] (pre[i] = product of the chain items before i), tot[G] =
// product of each chain.  Thread g owns items g, g+G, g+2G, ... (each step
// of the chain is a coalesced access).
template <bool FROM_S>
__global__ void k_ninv_up(const uint32_t* __restrict__ x, const uint8_t* __restrict__ s, long n,
                          long G, uint32_t* __restrict__ pre, uint32_t* __restrict__ tot) {
  MBFT_CHAIN_PRIO();
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  fe acc;
  fe_set(acc, kRN);  // Montgomery one
#pragma unroll 1
  for (long i = g; i < n; i += G) {
    plane_store(pre, n, i, acc);
    fe v;
    if (FROM_S)
      s_plain(v, s, i);
    else
      plane_load(v, x, n, i);
    fn_mul(acc, acc, v);
  }
  plane_store(tot, G, g, acc);
}

// The root of the tree: the m <= kTopMax chain totals x_k of the top level
// (planes, stride m) -> x_k^-1 R mod N, in place (what the down-sweeps hand
// down).  ONE workgroup: 4 values per thread as a chain (p_0 = R, p_j =
// mont(p_(j-1), v_j)), a product tree of the 1024 thread totals in LDS, one
// inversion at the root on lane 0 (divsteps, modinv.h: ~8K dependent ops
// where Fermat needs ~60K), then the tree and the chains walked back:
// inv(a) = mont(inv(a b / R), b) at every node, exactly as in the down-sweeps.
constexpr int kTopThreads = 256, kTopPer = 16;
constexpr long kTopMax = (long)kTopThreads * kTopPer;

// 256 threads (one wave per SIMD of one CU) so that the kernel fits beside
// the previous batch's verify waves (3 per SIMD, 168 VGPRs each): a
// 1024-thread block needs a nearly empty CU and waited for the verify
// kernel's tail.  Prefixes go to `pre` (kTopMax planes), not registers.
// The product tree of the 256 values node[256 + t] (t = thread) and back:
// node[1] = their product, inverted by wave 0 (x^-1 R), then every node
// replaced by the inverse of its value: inv(a) = mont(inv(a b / R), b).  On
// return node[256 + t] = (value of thread t)^-1 R.  All 256 threads call it.
MBFT_DEV void lds_tree_invert(uint32_t (&node)[NL][512], int t) {
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) {
      const int i = w + t;
      fe a, b, c;
#pragma unroll
      for (int k = 0; k < NL; k++) {
        a.v[k] = node[k][2 * i];
        b.v[k] = node[k][2 * i + 1];
      }
      fn_mul(c, a, b);
#pragma unroll
      for (int k = 0; k < NL; k++) node[k][i] = c.v[k];
    }
    __syncthreads();
  }
  // The root inversion runs on ALL lanes of wave 0, each on the same value,
  // passed through an empty asm with VGPR operands so the compiler treats it
  // as divergent: the code is then VALU (one v_mad per 32x32+64 product).
  // Uniform (lane 0 alone, or a uniform LDS read) it is scalarized into
  // multi-instruction SALU 64-bit arithmetic (tools/ubench_inv.hip).
  if (t < 64) {
    fe r;
#pragma unroll
    for (int k = 0; k < NL; k++) r.v[k] = node[k][1];
    fn_canon(r);
    uint32_t w[8], iw[8];
    fe_to_words(w, r);
#pragma unroll
    for (int k = 0; k < 8; k++) asm volatile("" : "+v"(w[k]));  // divergent to the compiler
    if (!modinv_n_var_wave(iw, w)) {
      // not reachable: every leaf is a product of values in [1, N)
#pragma unroll
      for (int k = 0; k < 8; k++) iw[k] = 0;
    }
    fe_from_words(r, iw);
    fn_to_mont(r, r);  // x^-1 R
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < NL; k++) node[k][1] = r.v[k];
    }
  }
  __syncthreads();
  for (int w = 1; w < 256; w <<= 1) {
    if (t < w) {
      const int i = w + t;
      fe a, b, r, ia, ib;
#pragma unroll
      for (int k = 0; k < NL; k++) {
        a.v[k] = node[k][2 * i];
        b.v[k] = node[k][2 * i + 1];
        r.v[k] = node[k][i];
      }
      fn_mul(ia, r, b);
      fn_mul(ib, r, a);
#pragma unroll
      for (int k = 0; k < NL; k++) {
        node[k][2 * i] = ia.v[k];
        node[k][2 * i + 1] = ib.v[k];
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_ninv_top(uint32_t* __restrict__ x, long m,
                                                  uint32_t* __restrict__ pre) {
  MBFT_CHAIN_PRIO();
  __shared__ uint32_t node[NL][2 * kTopThreads];  // node i (1 = root, leaves 256..511), SoA
  const int t = threadIdx.x;
  fe acc;
  fe_set(acc, kRN);  // Montgomery one
#pragma unroll 1
  for (int j = 0; j < kTopPer; j++) {
    const long idx = (long)j * kTopThreads + t;  // strided: coalesced planes
    plane_store(pre, kTopMax, idx, acc);
    if (idx < m) {
      fe v;
      plane_load(v, x, m, idx);
      fn_mul(acc, acc, v);
    }
  }
#pragma unroll
  for (int k = 0; k < NL; k++) node[k][kTopThreads + t] = acc.v[k];
  lds_tree_invert(node, t);
  fe r;
#pragma unroll
  for (int k = 0; k < NL; k++) r.v[k] = node[k][kTopThreads + t];
#pragma unroll 1
  for (int j = kTopPer - 1; j >= 0; j--) {
    const long idx = (long)j * kTopThreads + t;
    if (idx >= m) continue;
    fe v, p, o;
    plane_load(v, x, m, idx);
    plane_load(p, pre, kTopMax, idx);
    fn_mul(o, p, r);  // x_idx^-1 R
    fn_mul(r, r, v);
    plane_store(x, m, idx, o);
  }
}

// The chains of the one-launch batched s^-1 (k_ninv_local, k_ninv_block):
// thread-local Montgomery's trick over PER items b0, b0 + STRIDE, ... (each
// step a coalesced access).  The prefixes go to the w planes themselves
// (each is read back once, on the way down, just before the inverse
// overwrites it), and the raw bytes of the next item -- and of the next
// prefix on the way down -- are loaded one step ahead: the chain is a
// dependent multiply chain, and a load issued at its own step would stall it
// for the memory latency at every step.  Items past the batch (and
// out-of-range s, which the verifier rejects anyway) take the value 1;
// Montgomery's trick is consistent for it and nothing is stored.
template <int STRIDE>
MBFT_DEV void ninv_load_raw(const uint8_t* s, long n, long b0, int k, uint32_t* w) {
  const long i = b0 + (long)STRIDE * k;
  load_be256(w, s + 32 * (i < n ? i : 0));
}
template <int STRIDE>
MBFT_DEV void ninv_to_plain(long n, long b0, int k, const uint32_t* w, fe& v) {
  const long i = b0 + (long)STRIDE * k;
  const bool ok = i < n && !words_is_zero(w) && words_lt(w, kNw);
  fe_from_words(v, w);
  if (!ok) {
    fe_zero(v);
    v.v[0] = 1;
  }
}
// acc (Montgomery one on entry) -> the chain's product; prefix k to the planes
template <int PER, int STRIDE>
MBFT_DEV void ninv_chain_up(const uint8_t* s, long n, long b0, uint32_t* winv, fe& acc) {
  uint32_t nxt[8];
  ninv_load_raw<STRIDE>(s, n, b0, 0, nxt);
#pragma unroll 1
  for (int k = 0; k < PER; k++) {
    const long i = b0 + (long)STRIDE * k;
    uint32_t cur[8];
#pragma unroll
    for (int j = 0; j < 8; j++) cur[j] = nxt[j];
    if (k + 1 < PER) ninv_load_raw<STRIDE>(s, n, b0, k + 1, nxt);
    fe v;
    ninv_to_plain<STRIDE>(n, b0, k, cur, v);
    if (i < n) plane_store(winv, n, i, acc);  // prefix before item k
    fn_mul(acc, acc, v);
  }
}
// r = (the chain's product)^-1 R -> every item's s^-1 R in the planes
template <int PER, int STRIDE>
MBFT_DEV void ninv_chain_down(const uint8_t* s, long n, long b0, uint32_t* winv, fe& r) {
  uint32_t nxt[8];
  fe pn;
  {
    const long i = b0 + (long)STRIDE * (PER - 1);
    if (i < n) plane_load(pn, winv, n, i);
  }
  ninv_load_raw<STRIDE>(s, n, b0, PER - 1, nxt);
#pragma unroll 1
  for (int k = PER - 1; k >= 0; k--) {
    const long i = b0 + (long)STRIDE * k;
    const fe p = pn;
    uint32_t cur[8];
#pragma unroll
    for (int j = 0; j < 8; j++) cur[j] = nxt[j];
    if (k > 0) {
      const long ip = i - STRIDE;
      if (ip < n) plane_load(pn, winv, n, ip);
      if (k > 1) ninv_load_raw<STRIDE>(s, n, b0, k - 1, nxt);
    }
    fe o;
    fn_mul(o, p, r);  // s_i^-1 R
    if (k > 0) {
      fe v;
      ninv_to_plain<STRIDE>(n, b0, k, cur, v);
      fn_mul(r, r, v);
    }
    if (i < n) plane_store(winv, n, i, o);
  }
}

// Batched s^-1 of a batch issued while the GPU is idle (one batch at a time:
// its latency is what counts): ONE launch, every WAVE independent (no LDS,
// no barrier).  Wave v owns items [64 PER v, 64 PER (v + 1)); lane l the
// strided chain l, l + 64, ... (PER items, coalesced, prefixes in
// registers).  The 64 chain totals meet in a butterfly over the lanes
// (__shfl_xor at distance 1, 2, .., 32: after it every lane holds the
// wave's product, and sib[j] the product of the block it met at level j),
// the whole wave inverts that product together (modinv_n_var_wave), and the
// butterfly and the chain are walked back: inv(a) = mont(inv(a b / R), b),
// w = s^-1 R written to the planes -- the arithmetic of the level chain
// (k_ninv_up / k_ninv_top / k_ninv_down), so the same w.  fn_mul is
// symmetric bit for bit (the same products in the same columns), so both
// partners of a level compute the same value and all lanes pass the same
// root.  One inversion per 64 PER items.  The pipelined C2 loop's form
// (PER 16, batch_inverse_s_pipelined): with no barrier its waves interleave
// with the previous batch's verify waves (host.cpp verify_device).  Block 0
// also zeroes the exact-path queue counter the verify kernel that follows
// on the same stream appends to (saves a memset launch on the critical path).
// PROBE (tools/ubench_ninv.hip only): lane 0 of each wave writes
// s_memrealtime stamps after each phase to probe[6 wave ..].
template <int PER, bool PROBE = false>
__global__ void __launch_bounds__(256) k_ninv_local(const uint8_t* __restrict__ s, long n,
                                                    uint32_t* __restrict__ winv,
                                                    uint32_t* __restrict__ zero_word,
                                                    uint64_t* __restrict__ probe = nullptr,
                                                    const uint32_t* __restrict__ ndev = nullptr) {
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  uint64_t stamp[6];
  auto mark = [&](int k, const fe& dep) {
    if (PROBE) {
      asm volatile("s_nop 0" ::"v"(dep.v[0]), "v"(dep.v[8]) : "memory");
      stamp[k] = __builtin_amdgcn_s_memrealtime();
    }
  };
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long b0 = wave * 64 * PER + __lane_id();
  if (wave * 64 * PER >= n) return;  // wave-uniform
  // (ndev: n is an upper bound -- the planes' stride -- and the item count is
  // on the device; items past it in a live wave are garbage, harmless to
  // Montgomery's trick, and never read)
  if (ndev && wave * 64 * PER >= (long)*ndev) return;
  fe acc;
  fe_set(acc, kRN);  // Montgomery one
  mark(0, acc);
  ninv_chain_up<PER, 64>(s, n, b0, winv, acc);
  mark(1, acc);
  fe sib[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
#pragma unroll
    for (int k = 0; k < NL; k++) sib[j].v[k] = __shfl_xor(acc.v[k], 1 << j);
    fn_mul(acc, acc, sib[j]);
  }
  mark(2, acc);
  // the wave's product (the same on every lane) -> its inverse x^-1 R
  fe r = acc;
  fn_canon(r);
  uint32_t w[8], iw[8];
  fe_to_words(w, r);
  if (!modinv_n_var_wave(iw, w)) {
    // not reachable: every leaf is a value in [1, N)
#pragma unroll
    for (int k = 0; k < 8; k++) iw[k] = 0;
  }
  fe_from_words(r, iw);
  fn_to_mont(r, r);
  mark(3, r);
#pragma unroll
  for (int j = 5; j >= 0; j--) fn_mul(r, r, sib[j]);  // inverse of this lane's block at level j
  mark(4, r);
  ninv_chain_down<PER, 64>(s, n, b0, winv, r);
  mark(5, r);
  if (PROBE && __lane_id() == 0)
    for (int k = 0; k < 6; k++) probe[6 * wave + k] = stamp[k];
}

// The same one-launch s^-1 with ONE inversion per WORKGROUP (256 threads x
// PER items) instead of per wave: the 256 chain products meet in
// k_ninv_top's LDS product tree (lds_tree_invert: 8 levels up, the root
// inverted by wave 0, 8 levels down; a wave butterfly + 4-leaf tree instead
// had to hold 6 sibling products across the inversion and spilled: slower,
// tools/ubench_ninv.hip).  The chains issue their loads all at
// once (ninv_block_chains), so a launch waits on memory twice, not once per
// chain step -- the per-wave form's chains (k_ninv_local) stall on a load at
// every step and took ~2/3 of its launch.  PER = 8 (249 VGPRs, no spills):
// one inversion per 2,048 items, 2 blocks per CU, all resident at once for a
// 1M batch.  Block 0 zeroes the verify's queue counter.
// (The steps are expanded over an index sequence, so every array index is a
// compile-time constant and the arrays live in registers: a `#pragma unroll`
// loop left them in scratch.)  Prefixes go to the w planes on the way up (as
// in ninv_chain_up) and come back all at once, with the raw values, before the
// way down: two memory waits per launch instead of one per step.
template <int PER, bool PROBE, size_t... K>
MBFT_DEV void ninv_block_chains(const uint8_t* s, long n, long b0, uint32_t* winv,
                                uint32_t (&node)[NL][2 * kTopThreads], int t, uint64_t* probe,
                                std::index_sequence<K...>) {
  uint64_t stamp[5];
  auto mark = [&](int k, const fe& dep) {
    if (PROBE) {
      asm volatile("s_nop 0" ::"v"(dep.v[0]), "v"(dep.v[8]) : "memory");
      stamp[k] = __builtin_amdgcn_s_memrealtime();
    }
  };
  fe acc;
  fe_set(acc, kRN);
  mark(0, acc);
  {
    uint32_t raw[PER][8];
    (ninv_load_raw<256>(s, n, b0, (int)K, raw[K]), ...);  // every load in flight at once
    auto up = [&](auto kc) {
      constexpr int k = decltype(kc)::value;
      const long i = b0 + 256L * k;
      if (i < n) plane_store(winv, n, i, acc);  // the product of the items before k
      fe v;
      ninv_to_plain<256>(n, b0, k, raw[k], v);
      fn_mul(acc, acc, v);
    };
    (up(std::integral_constant<int, (int)K>{}), ...);
  }
  mark(1, acc);
#pragma unroll
  for (int j = 0; j < NL; j++) node[j][kTopThreads + t] = acc.v[j];
  lds_tree_invert(node, t);
  fe r;
#pragma unroll
  for (int j = 0; j < NL; j++) r.v[j] = node[j][kTopThreads + t];
  mark(2, r);
  uint32_t raw[PER][8];
  fe pre[PER];
  auto fetch = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const long i = b0 + 256L * k;
    if (i < n) plane_load(pre[k], winv, n, i);
    if (k > 0) ninv_load_raw<256>(s, n, b0, k, raw[k]);
  };
  (fetch(std::integral_constant<int, (int)K>{}), ...);
  mark(3, pre[PER - 1]);
  auto down = [&](auto kc) {
    constexpr int k = PER - 1 - decltype(kc)::value;
    fe o;
    fn_mul(o, pre[k], r);  // s_k^-1 R
    if (k > 0) {
      fe v;
      ninv_to_plain<256>(n, b0, k, raw[k], v);
      fn_mul(r, r, v);  // (the product of the items before k)^-1 R
    }
    const long i = b0 + 256L * k;
    if (i < n) plane_store(winv, n, i, o);
  };
  (down(std::integral_constant<int, (int)K>{}), ...);
  mark(4, r);
  if (PROBE && t == 0)
    for (int k = 0; k < 5; k++) probe[5 * blockIdx.x + k] = stamp[k];
}

// PROBE (tools/ubench_ninv.hip only): thread 0 of each block writes
// s_memrealtime stamps after each phase to probe[5 block ..].
template <int PER, bool PROBE = false>
__global__ void __launch_bounds__(256, (PER >= 16 ? 1 : 16 / PER))
    k_ninv_block(const uint8_t* __restrict__ s, long n, uint32_t* __restrict__ winv,
                 uint32_t* __restrict__ zero_word, uint64_t* __restrict__ probe = nullptr) {
  __shared__ uint32_t node[NL][2 * kTopThreads];  // node i (1 = root, leaves 256..511), SoA
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  const int t = threadIdx.x;
  const long b0 = (long)blockIdx.x * 256 * PER + t;  // the grid covers n: every block has items
  ninv_block_chains<PER, PROBE>(s, n, b0, winv, node, t, probe, std::make_index_sequence<PER>{});
}

// Level-l down-sweep.  in: x[n] (or s bytes at level 0, recomputed: one
// multiply instead of storing and re-reading 36 B per item), pre[n],
// inv_tot[G]; out: inv[n] = x_i^-1, written straight into its final buffer.
// zero_word (level 0, optional): zeroed by block 0 -- the exact-path queue
// counter of the verify that waits for this chain (no memset launch on the
// verify's stream, where it would queue behind other batches' kernels).
template <bool FROM_S>
__global__ void k_ninv_down(const uint32_t* __restrict__ x, const uint8_t* __restrict__ s,
                            const uint32_t* __restrict__ pre, long n, long G,
                            const uint32_t* __restrict__ inv_tot, uint32_t* __restrict__ inv,
                            uint32_t* __restrict__ zero_word) {
  MBFT_CHAIN_PRIO();
  if (zero_word && blockIdx.x == 0 && threadIdx.x == 0) *zero_word = 0;
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G || g >= n) return;
  fe r;
  plane_load(r, inv_tot, G, g);  // (prod of chain)^-1
  const long last = g + ((n - 1 - g) / G) * G;
#pragma unroll 1
  for (long i = last; i >= g; i -= G) {
    fe p, v, t;
    plane_load(p, pre, n, i);
    if (FROM_S)
      s_plain(v, s, i);
    else
      plane_load(v, x, n, i);
    fn_mul(t, r, p);   // x_i^-1 = (prefix_i) * (prod through i)^-1
    fn_mul(r, r, v);   // (prod through i-1)^-1
    plane_store(inv, n, i, t);
  }
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h and verify_launch.h)
namespace mbft_launch {

// Batched s^-1 (Montgomery's trick) as a tree of strided chains of 16:
// n -> ceil(n/16) -> ... until <= kTopMax (4096) totals, which k_ninv_top
// inverts with one workgroup and one divsteps inversion.
// Workspace per level l with m_l inputs and G_l chains: pre (m_l planes),
// tot (G_l planes) and, below the top level, inv_tot (G_l planes).
namespace {
constexpr long kChain = 16, kMaxRoots = kTopMax;
long ninv_groups(long m) { return (m + kChain - 1) / kChain; }
}  // namespace

size_t ninv_workspace_words(long n) {
  size_t words = (size_t)NL * kTopMax;  // k_ninv_top's prefixes
  long m = n;
  do {
    const long G = ninv_groups(m);
    words += (size_t)NL * (m + 2 * G);
    m = G;
  } while (m > kMaxRoots);
  return words + 64;
}

// w planes (9 x n) <- (s_i)^-1 * R mod N for each item (invalid s -> 1^-1)
hipError_t batch_inverse_s(const uint8_t* s, long n, uint32_t* ws, uint32_t* winv,
                           uint32_t* zero_word, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  struct Level { long m, G; uint32_t *pre, *tot, *itot; };
  Level lv[16];
  int nl = 0;
  uint32_t* top_pre = ws;
  uint32_t* wp = ws + (size_t)NL * kTopMax;
  long m = n;
  do {
    Level L;
    L.m = m;
    L.G = ninv_groups(m);
    L.pre = wp;  wp += (size_t)NL * L.m;
    L.tot = wp;  wp += (size_t)NL * L.G;
    L.itot = wp; wp += (size_t)NL * L.G;
    lv[nl++] = L;
    m = L.G;
  } while (m > kMaxRoots && nl < 16);
  // up-sweeps: level 0 reads s directly, level l > 0 reads level l-1's totals
  for (int l = 0; l < nl; l++) {
    const Level& L = lv[l];
    const dim3 grid((unsigned)((L.G + 255) / 256)), block(256);
    if (l == 0)
      hipLaunchKernelGGL(k_ninv_up<true>, grid, block, 0, st, nullptr, s, L.m, L.G, L.pre, L.tot);
    else
      hipLaunchKernelGGL(k_ninv_up<false>, grid, block, 0, st, lv[l - 1].tot, nullptr, L.m, L.G,
                         L.pre, L.tot);
  }
  // the top level's totals (<= kTopMax), inverted in place by one workgroup
  // (they are its inv_tot)
  Level& top = lv[nl - 1];
  hipLaunchKernelGGL(k_ninv_top, dim3(1), dim3(kTopThreads), 0, st, top.tot, top.G, top_pre);
  top.itot = top.tot;
  // down-sweeps: level l writes the inverses of its inputs, i.e. level
  // l-1's inv_tot (or winv at level 0)
  for (int l = nl - 1; l >= 0; l--) {
    const Level& L = lv[l];
    const dim3 grid((unsigned)((L.G + 255) / 256)), block(256);
    if (l == 0)
      hipLaunchKernelGGL(k_ninv_down<true>, grid, block, 0, st, nullptr, s, L.pre, L.m, L.G,
                         L.itot, winv, zero_word);
    else
      hipLaunchKernelGGL(k_ninv_down<false>, grid, block, 0, st, lv[l - 1].tot, nullptr, L.pre,
                         L.m, L.G, L.itot, lv[l - 1].itot, nullptr);
  }
  return hipGetLastError();
}

// The one-launch forms: chains of PER per wave (k_ninv_local) or per
// workgroup (k_ninv_block).
template <int PER>
hipError_t launch_ninv_local(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                             hipStream_t st, const uint32_t* ndev = nullptr) {
  const long per_block = 256L * PER;
  hipLaunchKernelGGL(k_ninv_local<PER>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256),
                     0, st, s, n, winv, zero_word, nullptr, ndev);
  return hipGetLastError();
}

template <int PER>
hipError_t launch_ninv_block(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                             hipStream_t st) {
  const long per_block = 256L * PER;
  hipLaunchKernelGGL(k_ninv_block<PER>, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256),
                     0, st, s, n, winv, zero_word);
  return hipGetLastError();
}

// The s^-1 of a batch on an idle GPU: the per-workgroup form, chains of 8.
hipError_t batch_inverse_s_local(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                                 hipStream_t st) {
  if (n <= 0) return hipSuccess;
  return launch_ninv_block<8>(s, n, winv, zero_word, st);
}

// The s^-1 of a batch issued while earlier batches are in flight (the
// pipelined C2 loop): the per-wave one-launch form, chains of 16, on the
// caller's stream -- no barrier, so its waves interleave with the previous
// batch's verify waves wave by wave.  Same-box A/B in the C2 loop (3 caller
// streams, tools/steady_ab.py, profiles/round6_ninv_forms.jsonl): 0.954 ms a
// step against 0.969 (per-block form) and 1.048 (the level chain on the
// high-priority stream, round 5's default).
hipError_t batch_inverse_s_pipelined(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                                     hipStream_t st) {
  if (n <= 0) return hipSuccess;
  return launch_ninv_local<16>(s, n, winv, zero_word, st, nullptr);
}

// The s^-1 of a small batch ahead of its verify kernel (verify(), where the
// plan says so): one item per lane, the item count on the device where given.
hipError_t batch_inverse_s_small(const uint8_t* s, long n, uint32_t* winv, const uint32_t* ndev, hipStream_t st) {
  return launch_ninv_local<1>(s, n, winv, nullptr, st, ndev);
}

}  // namespace mbft_launch
