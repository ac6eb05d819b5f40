// Test-only harness (tests/test_gpu_field.py): runs the library's P-256
// field and group primitives (minbft_amd/csrc/fe29.h, ecc.h) and the
// verifier's scalar side (scalar_dev.h: mod-N arithmetic, u1 / u2, the comb's
// signed recoding, the whole-wave inversion, the accept test) on caller-given
// limb inputs, one case per lane -- or one case per 64-lane block for the
// wave-uniform forms -- so that Python can check every result against
// big-integer arithmetic and every documented bound.  Built into
// tests/libfield_check.so by __graft_entry__.build(); never part of the
// product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/ecc.h"
#include "../../minbft_amd/csrc/scalar_dev.h"

using namespace mbft;

enum Op : uint32_t {
  OP_MUL = 0, OP_SQR = 1, OP_SUB = 2, OP_NEG = 3, OP_ADD = 4, OP_MUL2 = 5,
  OP_CANON = 6, OP_MULSMALL8 = 7, OP_MADD = 8, OP_DBL = 9, OP_SUB2X = 10,
  OP_MULADD_P5B = 11, OP_MULADD_P2B = 12, OP_SUB5 = 13, OP_FE_INV = 14,
  OP_CHUD_P = 16, OP_CHUD_N = 17, OP_AFF_CHUD_P = 18, OP_AFF_CHUD_N = 19,
  OP_CHUD_LAZY_P = 20, OP_CHUD_LAZY_N = 21, OP_CHUD_LAST_P = 22, OP_CHUD_LAST_N = 23,
  OP_NORM_LAZY = 24,
  OP_FN_MUL = 32, OP_FN_CANON = 33, OP_FN_CSUB1 = 34, OP_FN_TO_MONT = 35, OP_FN_FROM_MONT = 36,
  OP_SCALARS = 37, OP_X_MATCHES = 38, OP_FN_INV = 39
};

// in: per case 6 field elements (9 limbs each): a, b, c, d, e, f
// MADD: (X, Y, Z) = (a, b, c) Jacobian, (x2, y2) = (d, e) affine
// MULADD_P5B: fe_mul_add(a, b, kP5B - c)   (ec_madd_chud's H)
// MULADD_P2B: fe_mul_add(kP2B - a, b, c)   (ec_madd_chud's R' with a negative y2)
// CHUD_P / _N: ec_madd_chud((X, Y, ZZ, ZZZ) = (a, b, c, d), (e, f)), add_s2 = false / true
// AFF_CHUD_P / _N: ec_add_affine_chud((a, b), (e, f)), add_s2 = false / true
// CHUD_LAZY_P / _N: ec_madd_chud<LAZY> (ZZ in and out with lazy low limbs)
// CHUD_LAST_P / _N: ec_madd_chud<LAZY, LAST> (X and ZZ only; Y, ZZZ = inputs)
// NORM_LAZY: fe_norm_lazy(a)
// DBL:  (X, Y, Z) = (a, b, c)
// FE_INV: fe_inv(a); FN_INV: fn_inv(a) (the signer's fixed-exponent inversions, Montgomery in and out)
// FN_MUL: fn_mul(a, b); FN_CANON / FN_CSUB1 / FN_TO_MONT / FN_FROM_MONT: of a
// SCALARS: scalars(U1, U2, e = a, r = b, w = c); U1 -> out 0, U2 -> out 1 (8 words each)
// X_MATCHES: x_matches_r(X = a, ZZ = b, rw = the first 8 words of c) -> out 0, word 0
// out: per case 4 field elements (9 limbs each)
__global__ void k_field(const uint32_t* op, const uint32_t* in, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe v[6];
  for (int k = 0; k < 6; k++)
    for (int l = 0; l < NL; l++) v[k].v[l] = in[(size_t)i * 54 + 9 * k + l];
  fe r0, r1, r2, r3;
  fe_zero(r0); fe_zero(r1); fe_zero(r2); fe_zero(r3);
  switch (op[i]) {
    case OP_MUL: fe_mul(r0, v[0], v[1]); break;
    case OP_SQR: fe_sqr(r0, v[0]); break;
    case OP_SUB: fe_sub(r0, v[0], v[1]); break;
    case OP_NEG: fe_neg(r0, v[0]); break;
    case OP_ADD: fe_add(r0, v[0], v[1]); break;
    case OP_MUL2: fe_mul2(r0, v[0], v[1], v[2], v[3]); break;
    case OP_CANON: r0 = v[0]; fe_canon(r0); break;
    case OP_MULSMALL8: fe_mulsmall(r0, v[0], 8); break;
    case OP_SUB2X: fe_sub_2x(r0, v[0], v[1], v[2]); break;
    case OP_SUB5: fe_sub5(r0, v[0], v[1]); break;
    case OP_MULADD_P5B: {
      fe w;
      for (int l = 0; l < NL; l++) w.v[l] = kP5B[l] - v[2].v[l];
      fe_mul_add(r0, v[0], v[1], w);
      break;
    }
    case OP_MULADD_P2B: {
      fe a;
      for (int l = 0; l < NL; l++) a.v[l] = kP2B[l] - v[0].v[l];
      fe_mul_add(r0, a, v[1], v[2]);
      break;
    }
    case OP_MADD: {
      jac a{v[0], v[1], v[2]};
      ec_madd(a, a, v[3], v[4]);
      r0 = a.X; r1 = a.Y; r2 = a.Z;
      break;
    }
    case OP_CHUD_P:
    case OP_CHUD_N: {
      chud a{v[0], v[1], v[2], v[3]};
      ec_madd_chud(a, a, v[4], v[5], op[i] == OP_CHUD_N);
      r0 = a.X; r1 = a.Y; r2 = a.ZZ; r3 = a.ZZZ;
      break;
    }
    case OP_CHUD_LAZY_P:
    case OP_CHUD_LAZY_N: {
      chud a{v[0], v[1], v[2], v[3]};
      ec_madd_chud<true>(a, a, v[4], v[5], op[i] == OP_CHUD_LAZY_N);
      r0 = a.X; r1 = a.Y; r2 = a.ZZ; r3 = a.ZZZ;
      break;
    }
    case OP_CHUD_LAST_P:
    case OP_CHUD_LAST_N: {
      chud a{v[0], v[1], v[2], v[3]};
      ec_madd_chud<true, true>(a, a, v[4], v[5], op[i] == OP_CHUD_LAST_N);
      r0 = a.X; r1 = a.Y; r2 = a.ZZ; r3 = a.ZZZ;
      break;
    }
    case OP_NORM_LAZY: r0 = v[0]; fe_norm_lazy(r0); break;
    case OP_AFF_CHUD_P:
    case OP_AFF_CHUD_N: {
      chud a;
      ec_add_affine_chud(a, v[0], v[1], v[4], v[5], op[i] == OP_AFF_CHUD_N);
      r0 = a.X; r1 = a.Y; r2 = a.ZZ; r3 = a.ZZZ;
      break;
    }
    case OP_DBL: {
      jac a{v[0], v[1], v[2]};
      ec_dbl(a, a);
      r0 = a.X; r1 = a.Y; r2 = a.Z;
      break;
    }
    case OP_FE_INV: fe_inv(r0, v[0]); break;
    case OP_FN_INV: fn_inv(r0, v[0]); break;
    case OP_FN_MUL: fn_mul(r0, v[0], v[1]); break;
    case OP_FN_CANON: r0 = v[0]; fn_canon(r0); break;
    case OP_FN_CSUB1: r0 = v[0]; fn_csub(r0, 1); break;
    case OP_FN_TO_MONT: fn_to_mont(r0, v[0]); break;
    case OP_FN_FROM_MONT: fn_from_mont(r0, v[0]); break;
    case OP_SCALARS: {
      uint32_t U1[8], U2[8];
      scalars(U1, U2, v[0], v[1], v[2]);
      for (int l = 0; l < 8; l++) { r0.v[l] = U1[l]; r1.v[l] = U2[l]; }
      break;
    }
    case OP_X_MATCHES: {
      uint32_t rw[8];
      for (int l = 0; l < 8; l++) rw[l] = v[2].v[l];
      r0.v[0] = x_matches_r(v[0], v[1], rw) ? 1u : 0u;
      break;
    }
  }
  for (int l = 0; l < NL; l++) {
    out[(size_t)i * 36 + l] = r0.v[l];
    out[(size_t)i * 36 + 9 + l] = r1.v[l];
    out[(size_t)i * 36 + 18 + l] = r2.v[l];
    out[(size_t)i * 36 + 27 + l] = r3.v[l];
  }
}

// The comb's recoding of a whole scalar: in = 8 LE words of u, then W; out =
// 64 words, window k (low first) as index | neg << 30 | zero << 31 -- the
// loop every verify form runs (comb_digit, then shr_words by W).
__global__ void k_comb(const uint32_t* in, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t U[8];
  for (int l = 0; l < 8; l++) U[l] = in[(size_t)i * 9 + l];
  const int W = (int)in[(size_t)i * 9 + 8];
  const int S = (256 + W - 1) / W;
  uint32_t carry = 0;
  for (int k = 0; k < 64; k++) {
    uint32_t o = 0xFFFFFFFFu;
    if (k < S) {
      bool neg, zero;
      const uint32_t idx = comb_digit(U[0], carry, W, k + 1 >= S, neg, zero);
      shr_words(U, W);
      o = idx | (neg ? 1u << 30 : 0u) | (zero ? 1u << 31 : 0u);
    }
    out[(size_t)i * 64 + k] = o;
  }
}

// modinv_n_var_wave: ONE value per 64-lane block (in: 8 LE words a case),
// every lane's result out (8 words, then the return value).
__global__ void k_modinv_wave(const uint32_t* in, uint32_t* out) {
  uint32_t x[8], r[8];
  for (int l = 0; l < 8; l++) {
    x[l] = in[(size_t)blockIdx.x * 8 + l];
    asm volatile("" : "+v"(x[l]));  // per-lane registers, as at the library's call sites
    r[l] = 0;
  }
  const bool ok = modinv_n_var_wave(r, x);
  uint32_t* o = out + ((size_t)blockIdx.x * 64 + threadIdx.x) * 9;
  for (int l = 0; l < 8; l++) o[l] = r[l];
  o[8] = ok ? 1u : 0u;
}

enum GroupOp : uint32_t {
  G_ADD_FULL = 0, G_ADD_X_SAME = 1, G_ADD_X_DIFF = 2, G_MADD_P = 3, G_MADD_N = 4,
  G_AFF_P = 5, G_AFF_N = 6
};

// The joins of two Chudnovsky points and the mixed additions in both forms.
// in: per case 8 field elements: a = (X, Y, ZZ, ZZZ), b = (X, Y, ZZ, ZZZ)
//   ADD_FULL: ec_add_chud_full(a, b); ADD_X_SAME / _DIFF: ec_add_chud_x(a, b, same_sign)
//   MADD_P / _N: ec_madd_chud(a, (x2, y2) = (b.X, b.Y)), add_s2 = false / true
//   AFF_P / _N: ec_add_affine_chud((a.X, a.Y), (b.X, b.Y)), add_s2 = false / true
// out: per THREAD 4 field elements, then the return value (37 words).
// WIDE: one case per 64-lane block, the wave-uniform forms (every lane is
// handed the same inputs and writes its own outputs); else one case per lane,
// the sequential forms.
template <bool WIDE>
__global__ void k_group(const uint32_t* op, const uint32_t* in, uint32_t* out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = WIDE ? (int)blockIdx.x : t;
  if (i >= n) return;
  fe v[8];
  for (int k = 0; k < 8; k++)
    for (int l = 0; l < NL; l++) v[k].v[l] = in[(size_t)i * 72 + 9 * k + l];
  const chud a{v[0], v[1], v[2], v[3]}, b{v[4], v[5], v[6], v[7]};
  chud o;
  fe_zero(o.X); fe_zero(o.Y); fe_zero(o.ZZ); fe_zero(o.ZZZ);
  uint32_t ret = 2;  // no such form
  switch (op[i]) {
    case G_ADD_FULL:
      ret = (WIDE ? ec_add_chud_full_wide(o, a, b) : ec_add_chud_full(o, a, b)) ? 1u : 0u;
      break;
    case G_ADD_X_SAME:
    case G_ADD_X_DIFF:
      if (!WIDE) ret = ec_add_chud_x(o.X, o.ZZ, a, b, op[i] == G_ADD_X_SAME) ? 1u : 0u;
      break;
    case G_MADD_P:
    case G_MADD_N:
      if (WIDE) ec_madd_chud_wide(o, a, b.X, b.Y, op[i] == G_MADD_N);
      else ec_madd_chud(o, a, b.X, b.Y, op[i] == G_MADD_N);
      ret = 1;
      break;
    case G_AFF_P:
    case G_AFF_N:
      if (WIDE) ec_add_affine_chud_wide(o, a.X, a.Y, b.X, b.Y, op[i] == G_AFF_N);
      else ec_add_affine_chud(o, a.X, a.Y, b.X, b.Y, op[i] == G_AFF_N);
      ret = 1;
      break;
  }
  uint32_t* w = out + (size_t)t * 37;
  for (int l = 0; l < NL; l++) {
    w[l] = o.X.v[l];
    w[9 + l] = o.Y.v[l];
    w[18 + l] = o.ZZ.v[l];
    w[27 + l] = o.ZZZ.v[l];
  }
  w[36] = ret;
}

namespace {
// host arrays in and out around one launch: op (n words, or null), in (n x
// in_words), out (out_rows x out_words)
template <class Launch>
int run_cases(const uint32_t* h_op, const uint32_t* h_in, size_t in_words, uint32_t* h_out,
              size_t out_rows, size_t out_words, int n, Launch launch) {
  if (n <= 0) return -1;
  uint32_t *d_op = nullptr, *d_in = nullptr, *d_out = nullptr;
  int rc = 0;
  if (hipMalloc(&d_op, 4 * (size_t)n) != hipSuccess ||
      hipMalloc(&d_in, 4 * in_words * (size_t)n) != hipSuccess ||
      hipMalloc(&d_out, 4 * out_words * out_rows) != hipSuccess)
    rc = -1;
  if (!rc && ((h_op && hipMemcpy(d_op, h_op, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) ||
              hipMemcpy(d_in, h_in, 4 * in_words * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemset(d_out, 0xEE, 4 * out_words * out_rows) != hipSuccess))
    rc = -2;
  if (!rc) {
    launch(d_op, d_in, d_out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h_out, d_out, 4 * out_words * out_rows, hipMemcpyDeviceToHost) != hipSuccess)
      rc = -3;
  }
  (void)hipFree(d_op);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return rc;
}
}  // namespace

extern "C" int field_check_run(const uint32_t* h_op, const uint32_t* h_in, uint32_t* h_out,
                               int n) {
  return run_cases(h_op, h_in, 54, h_out, (size_t)n, 36, n,
                   [&](uint32_t* op, uint32_t* in, uint32_t* out) {
                     hipLaunchKernelGGL(k_field, dim3((n + 63) / 64), dim3(64), 0, 0, op, in, out, n);
                   });
}

// in: n x 9 words (u, W); out: n x 64 words
extern "C" int comb_check_run(const uint32_t* h_in, uint32_t* h_out, int n) {
  for (int i = 0; i < n; i++)
    if (h_in[(size_t)i * 9 + 8] < 4 || h_in[(size_t)i * 9 + 8] > 29) return -1;
  return run_cases(nullptr, h_in, 9, h_out, (size_t)n, 64, n,
                   [&](uint32_t*, uint32_t* in, uint32_t* out) {
                     hipLaunchKernelGGL(k_comb, dim3((n + 63) / 64), dim3(64), 0, 0, in, out, n);
                   });
}

// in: n x 8 words; out: n x 64 lanes x 9 words
extern "C" int modinv_wave_check_run(const uint32_t* h_in, uint32_t* h_out, int n) {
  return run_cases(nullptr, h_in, 8, h_out, (size_t)n * 64, 9, n,
                   [&](uint32_t*, uint32_t* in, uint32_t* out) {
                     hipLaunchKernelGGL(k_modinv_wave, dim3(n), dim3(64), 0, 0, in, out);
                   });
}

// in: n x 72 words; out: n x 37 words (wide == 0: the sequential forms, one
// case per lane) or n x 64 lanes x 37 words (wide != 0: one case per block)
extern "C" int group_check_run(const uint32_t* h_op, const uint32_t* h_in, uint32_t* h_out, int n,
                               int wide) {
  if (wide)
    return run_cases(h_op, h_in, 72, h_out, (size_t)n * 64, 37, n,
                     [&](uint32_t* op, uint32_t* in, uint32_t* out) {
                       hipLaunchKernelGGL(k_group<true>, dim3(n), dim3(64), 0, 0, op, in, out, n);
                     });
  return run_cases(h_op, h_in, 72, h_out, (size_t)n, 37, n,
                   [&](uint32_t* op, uint32_t* in, uint32_t* out) {
                     hipLaunchKernelGGL(k_group<false>, dim3((n + 63) / 64), dim3(64), 0, 0, op, in, out, n);
                   });
}
