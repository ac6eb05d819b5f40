// What runs before and beside the verifier: the SHA-256 digest kernels
// (k_sha256_var, k_usig_e, k_request_e, k_request_e_tiled, k_authen_e), the
// device-side decode of raw calls (k_prepare) and the plain bulk signer
// (k_sign), with their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "arena_dev.h"
#include "authen_dev.h"
#include "der_dev.h"
#include "ecc.h"
#include "kernels.h"
#include "scalar_dev.h"
#include "sha256.h"
#include "sha256_dev.h"
#include "verify_dev.h"
#include "words_dev.h"

using namespace mbft;

// acc += sum_i d_i * T[i][d_i] over the S = ceil(256/W) windows of scalar U
// (low window first): unchecked mixed additions, next entry prefetched one
// step ahead.  A degenerate addition (acc == +-entry) leaves Z == 0 for good,
// which the caller detects.  W is a runtime value (per table): the digit
// arithmetic is a handful of scalar-shift ops against ~1,800 VALU ops of the
// mixed addition, so one kernel serves every window size.
MBFT_DEV void comb_fast(jac& acc, bool& inf, uint32_t (&U)[8], const uint32_t* tab, int W) {
  const int S = (256 + W - 1) / W;
  uint32_t carry = 0;
  bool neg, zero;
  uint32_t idx = comb_digit(U[0], carry, W, S == 1, neg, zero);
  const uint4* p = comb_entry(tab, W, 0, idx);
  uint4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3];
#pragma unroll 1
  for (int step = 0; step < S; step++) {
    shr_words(U, W);
    bool nneg, nzero;
    const uint32_t in = comb_digit(U[0], carry, W, step + 2 >= S, nneg, nzero);
    const uint4* pn = comb_entry(tab, W, step + 1 < S ? step + 1 : step, in);
    const uint4 n0 = pn[0], n1 = pn[1], n2 = pn[2], n3 = pn[3];
    fe px, py;
    {
      uint32_t wx[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      uint32_t wy[8] = {c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
      fe_from_words(px, wx);
      fe_from_words(py, wy);
    }
    fe_cneg(py, neg);
    // Branches, not selects: a zero digit has probability 2^-(W-1) and `inf`
    // is wave-uniform after the first nonzero digit, so the common path is
    // the in-place mixed addition with no extra live registers.
    if (!zero) {
      if (inf) {
        acc.X = px;
        acc.Y = py;
        fe_one_mont(acc.Z);
        inf = false;
      } else {
        ec_madd(acc, acc, px, py);
      }
    }
    neg = nneg;
    zero = nzero;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
  }
}

// ---------------------------------------------------------------------------
// Bulk ECDSA signing (generation side: GenerateMessageAuthenTag for the
// ECDSA roles, crypto.go:63-76, and synthetic load generation).  R = k*G by
// the same 8-bit comb over the G table (no degenerate cases possible: the
// partial sums are distinct multiples < N of G).  Deterministic nonce
// k = SHA256(d || e || ctr) mod N.
struct SignArgs {
  const uint8_t* priv;      // nkeys x 32 B big-endian
  const uint32_t* key_idx;  // n (or null: key 0)
  const uint8_t* e;         // n x 32 B big-endian
  long n;
  const uint32_t* tabG;
  int wg;
  uint8_t* r_out;           // n x 32 B big-endian
  uint8_t* s_out;
  const uint8_t* k_in;      // optional n x 32 B big-endian nonces (crafted load)
};

__global__ void __launch_bounds__(256) k_sign(SignArgs A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t kid = A.key_idx ? A.key_idx[i] : 0u;
  uint32_t dbe[8], ebe[8], dw[8], ew[8];
  load_words8(dbe, reinterpret_cast<const uint32_t*>(A.priv + 32 * (size_t)kid));
  load_words8(ebe, reinterpret_cast<const uint32_t*>(A.e + 32 * i));
  // byte-order: sha256 consumes big-endian words == the raw bytes loaded
  // little-endian then byte-swapped
  uint32_t dm[8], em[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dm[j] = __builtin_bswap32(dbe[j]);
    em[j] = __builtin_bswap32(ebe[j]);
  }
  be_words_to_le(dw, dbe);
  be_words_to_le(ew, ebe);
  fe d, e, dm_n;
  fe_from_words(d, dw);
  fe_from_words(e, ew);
  fn_to_mont(dm_n, d);
  uint32_t rw_out[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sw_out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (uint32_t ctr = 0; ctr < 4; ctr++) {
    uint32_t h[8], m[16];
    uint32_t kw[8];
    if (A.k_in) {
      // a given nonce (generation of crafted inputs): one attempt
      uint32_t kbe[8];
      load_words8(kbe, reinterpret_cast<const uint32_t*>(A.k_in + 32 * i));
      be_words_to_le(kw, kbe);
      ctr = 3;
    } else {
      sha256_init(h);
#pragma unroll
      for (int j = 0; j < 8; j++) { m[j] = dm[j]; m[8 + j] = em[j]; }
      sha256_block(h, m);
#pragma unroll
      for (int j = 0; j < 16; j++) m[j] = 0;
      m[0] = ctr;
      m[1] = 0x80000000u;
      m[15] = 68u * 8u;
      sha256_block(h, m);
#pragma unroll
      for (int j = 0; j < 8; j++) kw[7 - j] = h[j];
    }
    fe k;
    fe_from_words(k, kw);
    fn_canon(k);
    uint32_t kc[8];
    fe_to_words(kc, k);
    if (words_is_zero(kc)) continue;
    // R = k G
    uint32_t U[8];
#pragma unroll
    for (int j = 0; j < 8; j++) U[j] = kc[j];
    jac acc;
    fe_zero(acc.X); fe_zero(acc.Y); fe_zero(acc.Z);
    bool inf = true;
    comb_fast(acc, inf, U, A.tabG, A.wg);
    fe zi, x;
    fe_inv(zi, acc.Z);
    fe_sqr(zi, zi);
    fe_mul(x, acc.X, zi);
    fe_from_mont(x, x);
    fe_canon(x);
    fn_canon(x);  // r = x mod N (x < p < 2N)
    uint32_t rw[8];
    fe_to_words(rw, x);
    if (words_is_zero(rw)) continue;
    // s = k^-1 (e + r d) mod N
    fe kinv, t, rd;
    fn_to_mont(kinv, k);
    fn_inv(kinv, kinv);
    fn_mul(rd, x, dm_n);   // r d (plain)
    fe_add(t, e, rd);
    fn_canon(t);
    fn_mul(t, t, kinv);
    fn_canon(t);
    uint32_t sw[8];
    fe_to_words(sw, t);
    if (words_is_zero(sw)) continue;
#pragma unroll
    for (int j = 0; j < 8; j++) { rw_out[j] = rw[j]; sw_out[j] = sw[j]; }
    break;
  }
  store_be256(A.r_out + 32 * i, rw_out);
  store_be256(A.s_out + 32 * i, sw_out);
}


// ---------------------------------------------------------------------------
// SHA-256 stage (messages/authen.go:78-82 hashsum; the USIG digest chain
// usig/sgx/sgx-usig.go:99-101 + usig-enclave.go:204-214).  One message per
// lane; digests are written as 32 big-endian bytes.

MBFT_DEV void store_digest(uint8_t* dst, const uint32_t h[8]) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(h[j]);
  store_words8(reinterpret_cast<uint32_t*>(dst), w);
}

// out[i] = SHA256(data[off[i] .. off[i+1]))
__global__ void k_sha256_var(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                             long n, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = off[i], b = off[i + 1];
  uint32_t h[8];
  sha256_msg(h, data + a, (uint32_t)(b - a));
  store_digest(out + 32 * i, h);
}

// e[dst_i] = SHA256(SHA256(m_i) || epoch_le || counter_le), dst_i = idx[i]
// (or i when idx is null: the batch path scatters into its item-indexed e)
__global__ void k_usig_e(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                         const uint64_t* __restrict__ epoch, const uint64_t* __restrict__ counter,
                         const uint32_t* __restrict__ idx, long n, uint8_t* __restrict__ e) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = off[i], b = off[i + 1];
  uint32_t d[8], h[8];
  sha256_msg(d, data + a, (uint32_t)(b - a));
  sha256_usig_chain(h, d, epoch[i], counter[i]);
  store_digest(e + 32 * (idx ? (long)idx[i] : i), h);
}

// REQUEST pipeline front end: AuthenBytes = "REQUEST" || seq_be64 ||
// SHA256(op) (messages/authen.go:33,54-56), and the ECDSA-role digest input
// e = (AuthenBytes || SHA256(""))[0:32] = "REQUEST" || seq || SHA256(op)[0:17]
// (sample/authentication/crypto.go:121).  ops: n x op_len bytes.
__global__ void k_request_e(const uint64_t* __restrict__ seq, const uint8_t* __restrict__ ops,
                            uint32_t op_len, long n, uint8_t* __restrict__ e) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h[8];
  sha256_msg(h, ops + (size_t)op_len * i, op_len);
  const uint64_t q = seq[i];
  uint32_t W[8];
  W[0] = 0x52455155u;                                   // "REQU"
  W[1] = 0x45535400u | (uint32_t)(q >> 56);             // "EST" seq0
  W[2] = (uint32_t)(q >> 24);                           // seq1..4
  W[3] = ((uint32_t)q << 8) | (h[0] >> 24);             // seq5..7 H0
#pragma unroll
  for (int k = 1; k <= 4; k++) W[3 + k] = (h[k - 1] << 8) | (h[k] >> 24);
  store_digest(e + 32 * i, W);
}

// Same digest for fixed-length operations (op_len % 16 == 0, ops 16-byte
// aligned, op_len <= kReqTileMax): one wave per 64 messages.  The wave's
// 64 x op_len contiguous bytes are loaded with fully coalesced dwordx4 loads
// (each wave-instruction reads 1 KiB in one piece) into an LDS tile whose rows
// are padded to an odd word stride (conflict-free row-per-lane reads), then
// each lane hashes its row from LDS with the state in VGPRs.
constexpr int kReqTileMax = 512;

__global__ void __launch_bounds__(64) k_request_e_tiled(const uint64_t* __restrict__ seq,
                                                        const uint8_t* __restrict__ ops,
                                                        uint32_t op_len, long n,
                                                        uint8_t* __restrict__ e) {
  extern __shared__ uint32_t tile[];
  const int lane = threadIdx.x;
  const long base = (long)blockIdx.x * 64;
  const int cnt = n - base < 64 ? (int)(n - base) : 64;
  const uint32_t wpr = op_len / 4, stride = wpr + 1, cpr = op_len / 16;
  const uint4* src = reinterpret_cast<const uint4*>(ops + (size_t)base * op_len);
  const uint32_t nchunks = (uint32_t)cnt * cpr;
#pragma unroll 4
  for (uint32_t c = lane; c < nchunks; c += 64) {
    const uint4 v = src[c];
    const uint32_t msg = c / cpr, w = (c - msg * cpr) * 4;
    uint32_t* row = tile + msg * stride + w;
    row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
  }
  __syncthreads();
  if (lane >= cnt) return;
  const uint32_t* row = tile + lane * stride;
  uint32_t h[8];
  sha256_init(h);
  const uint32_t nblk = (op_len + 9 + 63) / 64;
  const uint64_t bits = (uint64_t)op_len * 8u;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; b++) {
    uint32_t m[16];
    const bool last = b + 1 == nblk;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t wi = 16 * b + j;
      m[j] = wi < wpr ? __builtin_bswap32(row[wi]) : (wi == wpr ? 0x80000000u : 0u);
    }
    if (last) {
      m[14] = (uint32_t)(bits >> 32);
      m[15] = (uint32_t)bits;
    }
    sha256_block(h, m);
  }
  const uint64_t q = seq[base + lane];
  uint32_t W[8];
  W[0] = 0x52455155u;
  W[1] = 0x45535400u | (uint32_t)(q >> 56);
  W[2] = (uint32_t)(q >> 24);
  W[3] = ((uint32_t)q << 8) | (h[0] >> 24);
#pragma unroll
  for (int k = 1; k <= 4; k++) W[3 + k] = (h[k - 1] << 8) | (h[k] >> 24);
  store_digest(e + 32 * (base + lane), W);
}

// AuthenBytes + digest input e of every PREPARE / COMMIT / REPLY call from
// the message's raw fields and H(op) (authen_dev.h; H(op) computed by
// k_sha256_var over the operations).  One call per thread.
__global__ void k_authen_e(const uint8_t* __restrict__ H, const AuthenDesc* __restrict__ D, long n,
                           uint8_t* __restrict__ e) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AuthenDesc d = D[i];
  uint32_t hw[8], hb[8];
  load_words8(hb, reinterpret_cast<const uint32_t*>(H + 32 * (size_t)d.msg));
#pragma unroll
  for (int k = 0; k < 8; k++) hw[k] = __builtin_bswap32(hb[k]);  // big-endian-numeric words
  uint32_t out[8];
  authen_digest(out, d.kind, hw, d.seq, d.client, d.view, d.primary, d.prep_ctr, d.epoch, d.counter);
  store_digest(e + 32 * (size_t)d.item, out);
}

// ---------------------------------------------------------------------------
// Device-side decode of raw VerifyMessageAuthenTag calls (k_prepare): the
// byte-level part of batch.cpp's prepare_item, one call per lane, in the
// reference's check order (sample/authentication/authenticator.go:121-134,
// keymanager.go:100, crypto.go:79-89 for the ECDSA roles, crypto.go:186-239
// + usig.go:75-80 + sgx-usig.go:159-168 + usig-enclave.go:217-222 for USIG).
// The USIG epoch step stays on the host (it is ordered state); a USIG call
// whose DER fails, or has trailing bytes, is left to it (kHostSlot |
// MBFT_BAD_KEY, the host's kDeadSlot).
__constant__ uint8_t kEmptySha[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14,
                                      0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
                                      0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c,
                                      0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};

namespace {
constexpr uint32_t kStMalformedDer = 2, kStUnknownKey = 4, kStBadKey = 5, kStBadUi = 6,
                   kStBadCert = 7, kStUnknownRole = 10;
constexpr uint32_t kRoleReplica = 1, kRoleUsig = 2, kRoleClient = 3;

MBFT_DEV uint64_t load_be64_bytes(const uint8_t* p) {
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) v = (v << 8) | p[k];
  return v;
}
}  // namespace

__global__ void __launch_bounds__(256) k_prepare(PrepArgs A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  uint32_t role = A.roles8 ? (uint32_t)A.roles8[i] : A.roles[i];
  const uint32_t id = A.ids[i];
  const uint64_t ma = A.moff32 ? A.moff32[i] : A.moff[i], mz = A.moff32 ? A.moff32[i + 1] : A.moff[i + 1];
  const uint64_t ta = A.toff32 ? A.toff32[i] : A.toff[i], tz = A.toff32 ? A.toff32[i + 1] : A.toff[i + 1];
  // the call's fields must lie in its chunk's byte ranges, in order (the
  // host checks no call of a device-decoded batch): else flag the batch
  // (MBFT_ERR_ARG) and read nothing
  const bool in_range = A.mlo <= ma && ma <= mz && mz <= A.mhi && A.tlo <= ta && ta <= tz && tz <= A.thi;
  if (!in_range) {
    atomicOr(A.bad, 1u);
    role = ~0u;  // decided without reading a byte (an unknown role)
  }
  const uint64_t m0 = in_range ? ma - A.mbase : 0, t0 = in_range ? ta - A.tbase : 0;
  const uint32_t mlen = in_range ? (uint32_t)(mz - ma) : 0u;
  const uint32_t tlen = in_range ? (uint32_t)(tz - ta) : 0u;
  const uint8_t* msg = A.msgs + m0;
  uint32_t st = 0xFFu, sl = 0;
  uint32_t ew[8], rw[8], sw[8];
#pragma unroll
  for (int j = 0; j < 8; j++) ew[j] = rw[j] = sw[j] = 0;
  // the tag's covering words staged in this lane's LDS slot (one batch of
  // loads; DER is parsed byte by byte at LDS latency), arena_dev.h
  __shared__ uint32_t tagbuf[256 * kTagWords];
  uint32_t* tw = tagbuf + threadIdx.x * kTagWords;
  const bool staged = stage_field(tw, A.tags, t0, tlen);
  if (role > 3u || ((A.map.role_ok >> role) & 1u) == 0) {
    st = kStUnknownRole;
  } else {
    const uint64_t key = ((uint64_t)role << 32) | id;
    bool known = false;
    for (uint32_t h = keymap_hash(key) & A.map.mask, probe = 0; probe <= A.map.mask;
         probe++, h = (h + 1) & A.map.mask) {
      const uint64_t k = A.map.keys[h];
      if (k == key) {
        known = true;
        sl = A.map.slots[h];
        break;
      }
      if (k == ~0ull) break;
    }
    const bool valid = known && sl < A.nslots && A.keys[sl].valid != 0;
    auto parse = [&](const uint8_t* tag) __attribute__((always_inline)) {
      if (role != kRoleUsig) {
        // DER first: Go panics on a decode error before looking at the key
        uint32_t used;
        if (!der_sig(tag, tlen, rw, sw, used)) {
          st = kStMalformedDer;
        } else if (!known) {
          st = kStUnknownKey;
        } else if (!valid) {
          st = kStBadKey;
        } else if (mlen >= 32) {
          // md = msg || SHA256("") (crypto.go:121): e = md[0:32]
          const ArenaField f = arena_field(A.msgs, m0, 32);
          arena_block(f, 0, ew);
        } else {
#pragma unroll
          for (int k = 0; k < 32; k++) {
            const uint32_t b = (uint32_t)k < mlen ? (uint32_t)msg[k] : (uint32_t)kEmptySha[k - mlen];
            ew[k >> 2] |= b << (8 * (k & 3));
          }
        }
      } else if (tlen < 8) {
        st = kStBadUi;
      } else if (!known) {
        st = kStUnknownKey;
      } else if (!valid) {
        st = kStBadKey;
      } else if (tlen - 8 < 8) {
        st = kStBadCert;
      } else {
        const uint64_t counter = load_be64_bytes(tag), epoch = load_be64_bytes(tag + 8);
        uint32_t used;
        if (!der_sig(tag + 16, tlen - 16, rw, sw, used) || used != tlen - 16) {
          st = kStBadKey;  // the host's epoch step decides (MALFORMED_DER / DER_TRAILING)
        } else {
          uint32_t d[8], h[8];
          sha256_arena(d, A.msgs, m0, mlen);
          sha256_usig_chain(h, d, epoch, counter);
#pragma unroll
          for (int j = 0; j < 8; j++) ew[j] = __builtin_bswap32(h[j]);
        }
      }
    };
    if (staged)
      parse(reinterpret_cast<const uint8_t*>(tw) + (t0 & 3u));
    else
      parse(A.tags + t0);
  }
  store_words8(reinterpret_cast<uint32_t*>(A.e + 32 * i), ew);
  store_words8(reinterpret_cast<uint32_t*>(A.r + 32 * i), rw);
  store_words8(reinterpret_cast<uint32_t*>(A.s + 32 * i), sw);
  A.slot[i] = st == 0xFFu ? sl : (kHostSlot | st);
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h)
namespace mbft_launch {

hipError_t sha256_var(const uint8_t* data, const uint64_t* off, long n, uint8_t* out,
                      hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sha256_var, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, data, off,
                     n, out);
  return hipGetLastError();
}

hipError_t usig_e(const uint8_t* data, const uint64_t* off, const uint64_t* epoch,
                  const uint64_t* counter, const uint32_t* idx, long n, uint8_t* e,
                  hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_usig_e, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, data, off,
                     epoch, counter, idx, n, e);
  return hipGetLastError();
}

hipError_t request_e(const uint64_t* seq, const uint8_t* ops, uint32_t op_len, long n, uint8_t* e,
                     hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (op_len > 0 && op_len % 16 == 0 && op_len <= (uint32_t)kReqTileMax &&
      ((uintptr_t)ops & 15u) == 0) {
    const size_t lds = (size_t)64 * (op_len / 4 + 1) * 4;
    hipLaunchKernelGGL(k_request_e_tiled, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, seq,
                       ops, op_len, n, e);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_request_e, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seq, ops,
                     op_len, n, e);
  return hipGetLastError();
}

hipError_t prepare_calls(const PrepArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_prepare, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t authen_e(const uint8_t* H, const AuthenDesc* d, long n, uint8_t* e, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_authen_e, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, H, d, n, e);
  return hipGetLastError();
}

hipError_t sign(const uint8_t* priv, const uint32_t* key_idx, const uint8_t* e, const uint8_t* k_in,
                long n, const uint32_t* tabG, int wg, uint8_t* r_out, uint8_t* s_out,
                hipStream_t st) {
  if (n <= 0) return hipSuccess;
  SignArgs A{priv, key_idx, e, n, tabG, wg, r_out, s_out, k_in};
  hipLaunchKernelGGL(k_sign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace mbft_launch
