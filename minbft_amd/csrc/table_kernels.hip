// Key validation and table construction (init time, once per key):
// k_check_points, k_point_entries (a table-free key's one entry), the comb
// tables without doublings (k_table_pow2, k_table_fill) and the compact and
// signed compact keys' small tables (k_teeth_table, k_steeth_table), with
// their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecc.h"
#include "kernels.h"
#include "teeth_dev.h"
#include "words_dev.h"

using namespace mbft;

// ---------------------------------------------------------------------------
// Key validation: x, y < p and y^2 == x^3 - 3x + b.  xy: n x 16 LE words.
// (x509.ParsePKIXPublicKey's on-curve check, keymanager.go:357)
__global__ void k_check_points(const uint32_t* __restrict__ xy, int n,
                               uint32_t* __restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wx[8], wy[8];
  load_words8(wx, xy + 16 * i);
  load_words8(wy, xy + 16 * i + 8);
  const bool in_range = words_lt(wx, kPw) && words_lt(wy, kPw);
  fe x, y, b, t, lhs, rhs;
  fe_from_words(x, wx);
  fe_from_words(y, wy);
  fe_from_words(b, kBw);
  fe_to_mont(x, x);
  fe_to_mont(y, y);
  fe_to_mont(b, b);
  fe_sqr(lhs, y);
  fe_sqr(t, x);
  fe_mul(t, t, x);               // x^3
  fe_mulsmall(rhs, x, 3);
  fe_sub(rhs, t, rhs);           // x^3 - 3x
  fe_add(rhs, rhs, b);
  fe_canon(lhs);
  fe_canon(rhs);
  ok[i] = (in_range && fe_eq_canon(lhs, rhs)) ? 1u : 0u;
}

// A table-free key's whole device state (key window 0): the point as ONE comb
// entry -- x, y as 8 + 8 LE words, canonical Montgomery -- which the ladder
// reads (ladder_dev.h).  xy: n validated plain affine points, 16 LE words each.
__global__ void k_point_entries(const uint32_t* __restrict__ xy, int n, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wx[8], wy[8];
  load_words8(wx, xy + 16 * i);
  load_words8(wy, xy + 16 * i + 8);
  fe x, y;
  fe_from_words(x, wx);
  fe_from_words(y, wy);
  fe_to_mont(x, x);
  fe_to_mont(y, y);
  fe_canon(x);
  fe_canon(y);
  store_point_words(out + 16 * i, x, y);
}

// Comb geometry for window W, SIGNED digits: S = ceil(256 / W) windows.  A
// scalar u < 2^256 is recoded low to high into digits d_i in
// (-2^(W-1), 2^(W-1)] (x = window bits + carry; x > 2^(W-1) -> d = x - 2^W,
// carry 1), except the last window, which holds the top L = 256 - (S-1) W
// bits plus the carry: 0 <= d <= 2^L.  A table stores |d| * 2^(W i) * P for
// |d| >= 1 only (y of a negative digit is negated at use), at index
// (i << (W-1)) + |d| - 1: 2^(W-1) entries per window, 2^L for the last --
// half the entries of an unsigned comb with the same number of windows.
MBFT_DEV int comb_steps(int W) { return (256 + W - 1) / W; }
MBFT_DEV long comb_entries(int W) {
  const int S = comb_steps(W);
  return ((long)(S - 1) << (W - 1)) + (1L << (256 - (S - 1) * W));
}

// B[pt][i] = 2^(W*i) * P_pt for i < S, affine canonical Montgomery (16 words
// each).  xy: plain affine input points (validated).  One thread per (pt, i).
__global__ void k_table_pow2(const uint32_t* __restrict__ xy, int npts, int wbits,
                             uint32_t* __restrict__ bpts) {
  const int nwin = comb_steps(wbits);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npts * nwin) return;
  const int pt = t / nwin, w = t % nwin;
  uint32_t wx[8], wy[8];
  load_words8(wx, xy + 16 * pt);
  load_words8(wy, xy + 16 * pt + 8);
  jac a;
  fe_from_words(a.X, wx);
  fe_from_words(a.Y, wy);
  fe_to_mont(a.X, a.X);
  fe_to_mont(a.Y, a.Y);
  fe_one_mont(a.Z);
#pragma unroll 1
  for (int j = 0; j < wbits * w; j++) ec_dbl(a, a);
  fe x, y;
  ec_to_affine(x, y, a);
  store_point_words(bpts + 16 * t, x, y);
}

// tab[pt] entry (i, d - 1) = d * B[pt][i] (signed-digit layout above); the
// tables of the npts points follow each other (comb_entries(W) entries
// each), 16 words (x, y) per entry.
//
// Run-based fill: thread t owns a run of kFillRun consecutive multiples
// d0 .. d0 + L - 1 of one window's base point B (fewer when the window is
// smaller).  P_d0 = d0 B by double-and-add, then P_d = P_(d-1) + B, one mixed
// addition each (P_2 = 2B by doubling when d0 = 1: the only degenerate
// addition, since c B = +-B needs c = +-1 mod N).  Each Jacobian (X, Y) is
// parked canonical in its own output slot and the Z ratio H_d (Z_d = Z_(d-1)
// H_d) in scratch planes; ONE inversion per run gives 1/Z_last, and the
// down pass walks back: (x, y) = (X zi^2, Y zi^3), zi <- zi H_d.  About 20
// field multiplies per entry instead of a double-and-add plus an inversion
// per entry (~700).
constexpr int kFillRun = 32;

struct FillGeom {
  int S, L0, L1;      // windows, run length for windows 0..S-2 and for the last
  long R0, R1, runs;  // runs per window (full / last), runs per point
};

MBFT_DEV FillGeom fill_geom(int W) {
  FillGeom g;
  g.S = comb_steps(W);
  const int lastbits = 256 - (g.S - 1) * W;
  const long n0 = 1L << (W - 1), n1 = 1L << lastbits;
  g.L0 = (int)min((long)kFillRun, n0);
  g.L1 = (int)min((long)kFillRun, n1);
  g.R0 = n0 / g.L0;
  g.R1 = n1 / g.L1;
  g.runs = (long)(g.S - 1) * g.R0 + g.R1;
  return g;
}

MBFT_DEV void park_xy(uint32_t* dst, const jac& a) {
  fe x = a.X, y = a.Y;
  fe_canon(x);
  fe_canon(y);
  store_point_words(dst, x, y);
}

// runs [first, first + count) of the npts points' tables; scratch: 9 x L
// planes of `count` words (H of run-local entry j, limb k at (j*9+k)*count + t)
__global__ void __launch_bounds__(256) k_table_fill(const uint32_t* __restrict__ bpts, int npts,
                                                    int wbits, long first, long count,
                                                    uint32_t* __restrict__ scratch,
                                                    uint32_t* __restrict__ tab) {
  const FillGeom g = fill_geom(wbits);
  const long tl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long t = first + tl;
  if (tl >= count || t >= (long)npts * g.runs) return;
  const long pt = t / g.runs, rr = t - pt * g.runs;
  long win, run;
  int L;
  if (rr < (long)(g.S - 1) * g.R0) {
    win = rr / g.R0;
    run = rr - win * g.R0;
    L = g.L0;
  } else {
    win = g.S - 1;
    run = rr - (long)(g.S - 1) * g.R0;
    L = g.L1;
  }
  const long d0 = run * L + 1;  // first multiple of this run
  const long ent = comb_entries(wbits);
  uint32_t* dst = tab + 16 * (pt * ent + (win << (wbits - 1)) + (d0 - 1));
  fe bx, by;
  load_point(bx, by, reinterpret_cast<const uint4*>(bpts + 16 * (pt * g.S + win)));

  // P = d0 B (left-to-right double-and-add; partial sums c B with 1 < c < N
  // are never +-B)
  jac a;
  a.X = bx;
  a.Y = by;
  fe_one_mont(a.Z);
  const int top = 63 - __builtin_clzl((unsigned long)d0);
#pragma unroll 1
  for (int b = top - 1; b >= 0; b--) {
    ec_dbl(a, a);
    if ((d0 >> b) & 1) ec_madd(a, a, bx, by);
  }
  park_xy(dst, a);
  // chain: P_j = P_(j-1) + B, H_j parked in scratch
#pragma unroll 1
  for (int j = 1; j < L; j++) {
    fe h;
    if (d0 == 1 && j == 1) {
      ec_dbl(a, a);  // 2B from B (Z_0 = 1): the ratio is Z_1 itself
      h = a.Z;
    } else {
      ec_madd(a, a, bx, by, &h);
    }
#pragma unroll
    for (int k = 0; k < NL; k++) scratch[((long)j * NL + k) * count + tl] = h.v[k];
    park_xy(dst + 16 * j, a);
  }
  // 1/Z_(L-1), then walk back
  fe zi;
  fe_inv(zi, a.Z);
#pragma unroll 1
  for (int j = L - 1; j >= 0; j--) {
    fe X, Y, z2, z3, x, y;
    load_point(X, Y, reinterpret_cast<const uint4*>(dst + 16 * j));
    fe_sqr(z2, zi);
    fe_mul(z3, z2, zi);
    fe_mul(x, X, z2);
    fe_mul(y, Y, z3);
    fe_canon(x);
    fe_canon(y);
    store_point_words(dst + 16 * j, x, y);
    if (j > 0) {
      fe h;
#pragma unroll
      for (int k = 0; k < NL; k++) h.v[k] = scratch[((long)j * NL + k) * count + tl];
      fe_mul(zi, zi, h);  // 1/Z_(j-1)
    }
  }
}

// A compact key's table (teeth_dev.h): 2^t entries of 16 words, entry v =
// val(v) Q with val(v) = sum_j bit_j(v) 2^(j d), d = ceil(256 / t); entry 0 is
// never read (zeroed).  One lane per key, keys [first, first + count):
//  1. the t base points B_j = 2^(j d) Q by (t - 1) d dependent doublings,
//     parked Jacobian and made affine with ONE inversion (Montgomery's trick
//     over their t - 1 values of Z);
//  2. the subset sums in ascending v, one mixed addition each: the entry
//     without its lowest set bit (Jacobian, parked) plus that bit's base
//     point (affine) -- a single-tooth entry is its base point, Z = 1;
//  3. every entry made affine with ONE more inversion (Montgomery's trick
//     over the 2^t - 1 values of Z).
// The additions of step 2 are never degenerate: the addend is 2^(j d) Q, the
// other operand val(v') Q with v' = v minus its lowest bit j, so val(v') has
// its bits above j d -- the two differ, both lie in [1, 2^225), and so does
// their sum val(v): none of val(v') -+ 2^(j d) is 0 (mod N).  No doubling
// meets order 2 and no base point is infinity (N is prime, 2^(j d) < N).
// (X, Y) are parked canonical in the entry's own slot; scratch holds two
// planes of 8 words per entry and lane -- Z and the running product before
// it -- word k of entry v at ((plane 2^t + v) 8 + k) count + lane.
MBFT_DEV void teeth_park(uint32_t* scr, long count, long tl, long idx, const fe& a) {
  fe c = a;
  fe_canon(c);
  uint32_t w[8];
  fe_to_words(w, c);
#pragma unroll
  for (int k = 0; k < 8; k++) scr[(idx * 8 + k) * count + tl] = w[k];
}

MBFT_DEV void teeth_unpark(fe& a, const uint32_t* scr, long count, long tl, long idx) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = scr[(idx * 8 + k) * count + tl];
  fe_from_words(a, w);
}

// scr planes [lo, hi]: entries lo .. hi (step `by`: x2 for the base points)
// of this lane hold Z in plane 0; their (X, Y), parked in `dst`, become affine.
template <bool POW2>
MBFT_DEV void teeth_affine(uint32_t* dst, uint32_t* scr, long count, long tl, long ne, long lo, long hi) {
  fe prod;
  fe_one_mont(prod);
#pragma unroll 1
  for (long v = lo; v <= hi; v = POW2 ? 2 * v : v + 1) {
    teeth_park(scr, count, tl, ne + v, prod);  // the product before v
    fe z;
    teeth_unpark(z, scr, count, tl, v);
    fe_mul(prod, prod, z);
  }
  fe inv;
  fe_inv(inv, prod);
#pragma unroll 1
  for (long v = hi; v >= lo; v = POW2 ? v / 2 : v - 1) {
    fe pre, z, zi, z2, z3, X, Y, x, y;
    teeth_unpark(pre, scr, count, tl, ne + v);
    teeth_unpark(z, scr, count, tl, v);
    fe_mul(zi, inv, pre);  // 1 / Z_v
    fe_mul(inv, inv, z);   // 1 / (the product before v)
    load_point(X, Y, reinterpret_cast<const uint4*>(dst + 16 * v));
    fe_sqr(z2, zi);
    fe_mul(z3, z2, zi);
    fe_mul(x, X, z2);
    fe_mul(y, Y, z3);
    fe_canon(x);
    fe_canon(y);
    store_point_words(dst + 16 * v, x, y);
  }
}

__global__ void __launch_bounds__(64) k_teeth_table(const uint32_t* __restrict__ xy, long first, long count,
                                                    int t, uint32_t* __restrict__ scr,
                                                    uint32_t* __restrict__ tab) {
  const long tl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tl >= count) return;
  const long pt = first + tl;
  const int d = teeth_columns(t);
  const long ne = 1L << t;
  uint32_t* dst = tab + 16 * (pt * ne);
  uint32_t wx[8], wy[8];
  load_words8(wx, xy + 16 * pt);
  load_words8(wy, xy + 16 * pt + 8);
  jac a;
  fe_from_words(a.X, wx);
  fe_from_words(a.Y, wy);
  fe_to_mont(a.X, a.X);
  fe_to_mont(a.Y, a.Y);
  fe_one_mont(a.Z);
#pragma unroll
  for (int k = 0; k < 16; k++) dst[k] = 0u;  // entry 0
  park_xy(dst + 16, a);                       // B_0 = Q
  teeth_park(scr, count, tl, 1, a.Z);
  // 1. base points
#pragma unroll 1
  for (int j = 1; j < t; j++) {
#pragma unroll 1
    for (int k = 0; k < d; k++) ec_dbl(a, a);
    park_xy(dst + 16 * (1L << j), a);
    teeth_park(scr, count, tl, 1L << j, a.Z);
  }
  teeth_affine<true>(dst, scr, count, tl, ne, 2, ne / 2);
  {
    fe one;
    fe_one_mont(one);
#pragma unroll 1
    for (int j = 1; j < t; j++) teeth_park(scr, count, tl, 1L << j, one);
  }
  // 2. subset sums
#pragma unroll 1
  for (long v = 3; v < ne; v++) {
    const long low = v & -v;
    if (low == v) continue;  // a base point
    jac s;
    load_point(s.X, s.Y, reinterpret_cast<const uint4*>(dst + 16 * (v - low)));
    teeth_unpark(s.Z, scr, count, tl, v - low);
    fe bx, by;
    load_point(bx, by, reinterpret_cast<const uint4*>(dst + 16 * low));
    ec_madd(s, s, bx, by);
    park_xy(dst + 16 * v, s);
    teeth_park(scr, count, tl, v, s.Z);
  }
  // 3. affine
  teeth_affine<false>(dst, scr, count, tl, ne, 1, ne - 1);
}

// A signed compact key's table (teeth_dev.h): 2^(t-1) entries, entry idx =
// (2^((t-1) d) + sum_(j < t-1) sigma_j 2^(j d)) Q with sigma_j = +1 iff bit j
// of idx is set.  One lane per key, with k_teeth_table's parked Z and
// Montgomery's trick; scratch as there, two planes of 8 words per entry and
// lane (as large as the tables):
//  1. ONE chain of (t - 1) d dependent doublings from Q passes D_j = 2 B_j
//     (j < t - 1) and B_(j+1) = 2^((j+1) d) Q: these 2 t - 2 <= 2^(t-1) points
//     are parked in the entry slots 0 .. 2 t - 3 (D_j at j, B_j at t - 2 + j)
//     and made affine with one inversion;
//  2. the D_j move to the scratch's second plane (unused until step 4: 2^(t-2)
//     >= t - 1 points fit), entry 0 = B_(t-1) - B_(t-2) - .. - B_0 is summed in
//     registers (B_0 = Q) and only then written over slot 0;
//  3. every other entry in ascending idx is the entry without idx's lowest
//     set bit j, plus D_j;
//  4. every entry made affine with one more inversion.
// No addition is degenerate.  Step 2 adds -2^(j d) Q to a Q with a = 2^((t-1)
// d) - sum_(j < j' < t-1) 2^(j' d): a is a positive multiple of 2^((j+1) d),
// so a > 2^(j d) and a - 2^(j d) > 0; step 3 adds the EVEN 2^(j d + 1) Q to m Q
// with m an ODD entry multiplier, so m != +-2^(j d + 1).  All of these and
// their sums lie in [1, 2^234) and N > 2^255 is prime: none of a -+ b is 0
// (mod N), no operand is infinity, and no doubling meets order 2.
__global__ void __launch_bounds__(64) k_steeth_table(const uint32_t* __restrict__ xy, long first, long count,
                                                     int t, uint32_t* __restrict__ scr,
                                                     uint32_t* __restrict__ tab) {
  const long tl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tl >= count) return;
  const long pt = first + tl;
  const int d = teeth_columns(t);
  const long ne = 1L << (t - 1);
  uint32_t* dst = tab + 16 * (pt * ne);
  uint32_t wx[8], wy[8];
  load_words8(wx, xy + 16 * pt);
  load_words8(wy, xy + 16 * pt + 8);
  fe qx, qy;
  fe_from_words(qx, wx);
  fe_from_words(qy, wy);
  fe_to_mont(qx, qx);
  fe_to_mont(qy, qy);
  fe_canon(qx);
  fe_canon(qy);
  // 1. the doubling chain
  {
    jac a;
    a.X = qx;
    a.Y = qy;
    fe_one_mont(a.Z);
#pragma unroll 1
    for (int j = 0; j < t - 1; j++) {
      ec_dbl(a, a);
      park_xy(dst + 16 * (long)j, a);  // D_j
      teeth_park(scr, count, tl, j, a.Z);
#pragma unroll 1
      for (int k = 1; k < d; k++) ec_dbl(a, a);
      park_xy(dst + 16 * (long)(t - 1 + j), a);  // B_(j+1)
      teeth_park(scr, count, tl, t - 1 + j, a.Z);
    }
  }
  teeth_affine<false>(dst, scr, count, tl, ne, 0, 2 * t - 3);
  // 2. D_j to the second plane, entry 0
#pragma unroll 1
  for (int j = 0; j < t - 1; j++) {
    fe x, y;
    load_point(x, y, reinterpret_cast<const uint4*>(dst + 16 * (long)j));
    teeth_park(scr, count, tl, ne + 2 * j, x);
    teeth_park(scr, count, tl, ne + 2 * j + 1, y);
  }
  {
    jac s;
    load_point(s.X, s.Y, reinterpret_cast<const uint4*>(dst + 16 * (long)(2 * t - 3)));  // B_(t-1)
    fe_one_mont(s.Z);
#pragma unroll 1
    for (int j = t - 2; j >= 0; j--) {
      fe bx, by;
      if (j > 0) {
        load_point(bx, by, reinterpret_cast<const uint4*>(dst + 16 * (long)(t - 2 + j)));
      } else {
        bx = qx;
        by = qy;
      }
      fe_neg(by, by);
      ec_madd(s, s, bx, by);
    }
    park_xy(dst, s);
    teeth_park(scr, count, tl, 0, s.Z);
  }
  // 3. the other entries
#pragma unroll 1
  for (long v = 1; v < ne; v++) {
    const long low = v & -v;
    const int j = __ffsll((long long)low) - 1;
    jac s;
    load_point(s.X, s.Y, reinterpret_cast<const uint4*>(dst + 16 * (v - low)));
    teeth_unpark(s.Z, scr, count, tl, v - low);
    fe bx, by;
    teeth_unpark(bx, scr, count, tl, ne + 2 * j);
    teeth_unpark(by, scr, count, tl, ne + 2 * j + 1);
    ec_madd(s, s, bx, by);
    park_xy(dst + 16 * v, s);
    teeth_park(scr, count, tl, v, s.Z);
  }
  // 4. affine
  teeth_affine<false>(dst, scr, count, tl, ne, 0, ne - 1);
}

// ---------------------------------------------------------------------------
// host-side launchers (declared in kernels.h)
namespace mbft_launch {

hipError_t check_points(const uint32_t* xy, int n, uint32_t* ok, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_check_points, dim3((n + 63) / 64), dim3(64), 0, st, xy, n, ok);
  return hipGetLastError();
}

hipError_t point_entries(const uint32_t* xy, int n, uint32_t* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_point_entries, dim3((n + 127) / 128), dim3(128), 0, st, xy, n, out);
  return hipGetLastError();
}

size_t table_entries(int wbits) {
  const int S = (256 + wbits - 1) / wbits;
  return ((size_t)(S - 1) << (wbits - 1)) + ((size_t)1 << (256 - (S - 1) * wbits));
}
size_t table_words(int wbits) { return table_entries(wbits) * 16u; }
int table_steps(int wbits) { return (256 + wbits - 1) / wbits; }

hipError_t build_tables(const uint32_t* xy, int npts, int wbits, uint32_t* bpts, uint32_t* tab,
                        hipStream_t st) {
  if (npts <= 0) return hipSuccess;
  if (wbits < kMinWindow || wbits > kMaxWindow) return hipErrorInvalidValue;
  const int t1 = npts * table_steps(wbits);
  hipLaunchKernelGGL(k_table_pow2, dim3((t1 + 63) / 64), dim3(64), 0, st, xy, npts, wbits, bpts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // runs (k_table_fill) in launches of at most 2^19 threads, each with its
  // own H scratch (9 x kFillRun words per thread)
  const int S = table_steps(wbits);
  const int lastbits = 256 - (S - 1) * wbits;
  const long n0 = 1L << (wbits - 1), n1 = 1L << lastbits;
  const long L0 = n0 < kFillRun ? n0 : kFillRun, L1 = n1 < kFillRun ? n1 : kFillRun;
  const long runs = (long)(S - 1) * (n0 / L0) + n1 / L1;
  const long total = (long)npts * runs;
  const long chunk = total < (1L << 19) ? total : (1L << 19);
  uint32_t* scratch = nullptr;
  e = hipMalloc(reinterpret_cast<void**>(&scratch), (size_t)chunk * NL * kFillRun * 4);
  if (e != hipSuccess) return e;
  for (long first = 0; first < total; first += chunk) {
    const long cnt = total - first < chunk ? total - first : chunk;
    hipLaunchKernelGGL(k_table_fill, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st,
                       bpts, npts, wbits, first, cnt, scratch, tab);
    e = hipGetLastError();
    if (e != hipSuccess) break;
  }
  // the launches read the scratch until they finish
  const hipError_t es = hipStreamSynchronize(st);
  const hipError_t ef = hipFree(scratch);
  return e != hipSuccess ? e : (es != hipSuccess ? es : ef);
}

// The compact and the signed compact keys' tables (k_teeth_table,
// k_steeth_table): one lane per key, in launches whose scratch (as large as
// their tables: two planes of 8 words per entry) stays within 64 MiB.
// teeth in [lo, hi]; a key's table is words_of(teeth) words.
using TeethKernel = void (*)(const uint32_t*, long, long, int, uint32_t*, uint32_t*);
template <TeethKernel KERNEL>
static hipError_t build_lane_tables(int lo, int hi, size_t (*words_of)(int), const uint32_t* xy, int npts, int teeth,
                                    uint32_t* tab, hipStream_t st) {
  if (npts <= 0) return hipSuccess;
  if (teeth < lo || teeth > hi) return hipErrorInvalidValue;
  const size_t per_key = words_of(teeth) * 4;
  long chunk = (long)(((size_t)64 << 20) / per_key);
  if (chunk > npts) chunk = npts;
  uint32_t* scratch = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&scratch), (size_t)chunk * per_key);
  if (e != hipSuccess) return e;
  for (long first = 0; first < npts; first += chunk) {
    const long cnt = npts - first < chunk ? npts - first : chunk;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, xy, first, cnt, teeth, scratch,
                       tab);
    e = hipGetLastError();
    if (e != hipSuccess) break;
  }
  // the launches read the scratch until they finish
  const hipError_t es = hipStreamSynchronize(st);
  const hipError_t ef = hipFree(scratch);
  return e != hipSuccess ? e : (es != hipSuccess ? es : ef);
}

size_t teeth_table_words(int teeth) { return ((size_t)1 << teeth) * 16u; }

hipError_t build_teeth_tables(const uint32_t* xy, int npts, int teeth, uint32_t* tab, hipStream_t st) {
  return build_lane_tables<k_teeth_table>(kTeethMin, kTeethMax, teeth_table_words, xy, npts, teeth, tab, st);
}

size_t steeth_table_words(int teeth) { return ((size_t)1 << (teeth - 1)) * 16u; }

hipError_t build_steeth_tables(const uint32_t* xy, int npts, int teeth, uint32_t* tab, hipStream_t st) {
  return build_lane_tables<k_steeth_table>(kSteethMin, kSteethMax, steeth_table_words, xy, npts, teeth, tab, st);
}

hipError_t generator_xy(uint32_t* xy16, hipStream_t st) {
  uint32_t h[16];
  hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(kGxw), 32, 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  e = hipMemcpyFromSymbol(h + 8, HIP_SYMBOL(kGyw), 32, 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(xy16, h, 64, hipMemcpyHostToDevice, st);
}

}  // namespace mbft_launch
