// Test-only harness (tests/test_gpu_sign_dev.py): runs the batch signer's
// device functions (minbft_amd/csrc/sign_rs_dev.h, sign_dev.h, der_enc_dev.h)
// on caller-given inputs, one case per lane, so that Python can hand them the
// nonces, points and candidate lists that never come out of HMAC and check
// every result against big integers.  The functions are the product's own,
// called, not restated; only the list-backed nonce source of the `loop` op is
// the harness's.  Host arrays go in and out around one launch, every output
// is pre-filled with a marker, every HIP call's status is checked.  Built
// into tests/libsign_dev_check.so by __graft_entry__.build(); never part of
// the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/sign_rs_dev.h"

using namespace mbft;

namespace {

constexpr int kMaxList = kSignTries + 1;  // candidates a `loop` case may carry
constexpr int kMark = 0xAA;               // every output byte before the launch

// A device buffer around one launch: in() copies a host array, out() fills
// with the marker; back() copies to the host.  ok stays false after the first
// HIP call that fails.
struct Bufs {
  static constexpr int kMax = 16;
  void* p[kMax];
  int n = 0;
  bool ok = true;
  ~Bufs() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  void* raw(size_t bytes) {
    void* d = nullptr;
    if (!ok || n == kMax || hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    p[n++] = d;
    return d;
  }
  template <class T> T* in(const T* h, size_t count) {
    T* d = static_cast<T*>(raw(sizeof(T) * count));
    if (d && count && hipMemcpy(d, h, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  template <class T> T* out(size_t count) {
    T* d = static_cast<T*>(raw(sizeof(T) * count));
    if (d && hipMemset(d, kMark, sizeof(T) * (count ? count : 1)) != hipSuccess) ok = false;
    return d;
  }
  template <class T> void back(T* h, const T* d, size_t count) {
    if (ok && count && hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  }
  // after the launch
  void sync() {
    if (ok && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) ok = false;
  }
};

// entries of the signer's table for window W (the layout of k_table_fill)
size_t table_entries(int W) {
  const int S = sign_steps(W);
  return ((size_t)(S - 1) << (W - 1)) + ((size_t)1 << (256 - (S - 1) * W));
}

bool table_ok(int W, size_t tab_words) {
  return W >= 4 && W <= 6 && tab_words == 16 * table_entries(W);
}

dim3 grid(int n) { return dim3((unsigned)((n + 63) / 64)); }

MBFT_DEV void put_fe(uint32_t* o, const fe& a) {
  for (int l = 0; l < NL; l++) o[l] = a.v[l];
}

MBFT_DEV void get_fe(fe& a, const uint32_t* p) {
  for (int l = 0; l < NL; l++) a.v[l] = p[l];
}

// d (Montgomery form mod N) and e as limbs, from little-endian words
MBFT_DEV void load_de(fe& dm_n, fe& e, const uint32_t* dw, const uint32_t* ew) {
  uint32_t a[8], b[8];
  for (int j = 0; j < 8; j++) { a[j] = dw[j]; b[j] = ew[j]; }
  fe d;
  fe_from_words(d, a);
  fe_from_words(e, b);
  fn_to_mont(dm_n, d);
}

// The `loop` op's nonce source: the lane's list of candidates (little-endian
// words each), at most kSignTries of them handed out, like the product's.
struct ListNonces {
  const uint32_t* list;
  int count, left = kSignTries;
  uint32_t drawn = 0, discards = 0;
  MBFT_DEV bool next(uint32_t (&kb)[8]) {
    if (left <= 0 || (int)drawn >= count) return false;
    left--;
    for (int j = 0; j < 8; j++) kb[j] = list[8 * drawn + 7 - j];
    drawn++;
    return true;
  }
  MBFT_DEV void discarded() { discards++; }
};

}  // namespace

// comb: k n x 8 little-endian words -> X, Y, Z limbs of sign_comb's result
__global__ void k_comb(const uint32_t* k, const uint32_t* tab, int W, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kw[8];
  for (int j = 0; j < 8; j++) kw[j] = k[(size_t)8 * i + j];
  jac R;
  sign_comb(R, kw, tab, W);
  put_fe(out + (size_t)27 * i, R.X);
  put_fe(out + (size_t)27 * i + 9, R.Y);
  put_fe(out + (size_t)27 * i + 18, R.Z);
}

// r_of_point: X, Z limbs (n x 18) -> r as 8 little-endian words
__global__ void k_r_of_point(const uint32_t* xz, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe X, Z, r;
  get_fe(X, xz + (size_t)18 * i);
  get_fe(Z, xz + (size_t)18 * i + 9);
  uint32_t rw[8];
  sign_r(r, rw, X, Z);
  for (int j = 0; j < 8; j++) out[(size_t)8 * i + j] = rw[j];
}

// rs_of_k: k, d, e (n x 24 little-endian words) -> r, s (n x 16 words)
__global__ void k_rs_of_k(const uint32_t* kde, const uint32_t* tab, int W, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kw[8];
  for (int j = 0; j < 8; j++) kw[j] = kde[(size_t)24 * i + j];
  fe dm_n, e, r;
  load_de(dm_n, e, kde + (size_t)24 * i + 8, kde + (size_t)24 * i + 16);
  jac R;
  sign_comb(R, kw, tab, W);
  uint32_t rw[8], sw[8];
  sign_r(r, rw, R.X, R.Z);
  sign_s(sw, kw, r, dm_n, e);
  for (int j = 0; j < 8; j++) {
    out[(size_t)16 * i + j] = rw[j];
    out[(size_t)16 * i + 8 + j] = sw[j];
  }
}

// loop: per lane a list of kMaxList candidates (count[i] of them valid), d, e
// (n x 16 little-endian words); lane i's UI carries counter first + i.
// res: n x 20 words: the return value, candidates drawn, discards, 0, then r
// and s as little-endian words.
__global__ void k_loop(const uint32_t* cand, const uint32_t* count, const uint32_t* de, const uint32_t* tab,
                       int W, uint64_t first, uint64_t epoch, uint32_t* res, uint8_t* tags, uint8_t* tag_len,
                       uint8_t* uis, uint8_t* ui_len, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe dm_n, e;
  load_de(dm_n, e, de + (size_t)16 * i, de + (size_t)16 * i + 8);
  ListNonces src;
  src.list = cand + (size_t)8 * kMaxList * i;
  src.count = (int)count[i];
  uint32_t rb[8], sb[8];
  const bool ok = sign_loop(rb, sb, src, dm_n, e, tab, W);
  uint32_t* o = res + (size_t)20 * i;
  o[0] = ok ? 1u : 0u;
  o[1] = src.drawn;
  o[2] = src.discards;
  o[3] = 0;
  for (int j = 0; j < 8; j++) {
    o[4 + j] = rb[7 - j];
    o[12 + j] = sb[7 - j];
  }
  sign_tag_finish(tags + (size_t)kTagSlot * i, tag_len + i, ok, rb, sb);
  usig_ui_finish(uis + (size_t)kUiSlot * i, ui_len + i, ok, first + (uint64_t)i, epoch, rb, sb);
}

// nonce: the device twin of sign_check_nonce (tests/csrc/sign_check.cpp)
__global__ void k_nonce(const uint8_t* d, const uint8_t* e, const uint8_t* q, uint8_t* k_out, int32_t* tries,
                        int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t qw[8], dw[8], ew[8], kw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  load_be_words(qw, q);
  load_be_words(dw, d + (size_t)32 * i);
  load_be_words(ew, e + (size_t)32 * i);
  Rfc6979 g;
  g.init(dw, ew, qw);
  int left = kSignTries;
  const bool ok = rfc6979_next(g, qw, kw, left);
  tries[i] = ok ? kSignTries - left : 0;
  uint32_t* o = reinterpret_cast<uint32_t*>(k_out + (size_t)32 * i);
  for (int j = 0; j < 8; j++) o[j] = ok ? __builtin_bswap32(kw[j]) : 0u;
}

// der: the device twin of sign_check_der
__global__ void k_der(const uint8_t* r, const uint8_t* s, uint8_t* tags, uint8_t* lens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rw[8], sw[8];
  load_be_words(rw, r + (size_t)32 * i);
  load_be_words(sw, s + (size_t)32 * i);
  lens[i] = (uint8_t)der_encode_sig(tags + (size_t)kTagSlot * i, rw, sw);
}

// pick: the device twin of sign_check_pick, one |digit| per lane
__global__ void k_pick(const uint32_t* win, int count, const uint32_t* mags, uint32_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[16];
  sign_pick(w, win, count, mags[i]);
  for (int j = 0; j < 16; j++) out[(size_t)16 * i + j] = w[j];
}

extern "C" {

int sign_dev_tries() { return kSignTries; }
uint64_t sign_dev_table_entries(int W) { return W >= 4 && W <= 6 ? table_entries(W) : 0; }

// k: n x 8 words; tab: tab_words words; out: n x 27 words
int sign_dev_comb(const uint32_t* k, int n, const uint32_t* tab, uint64_t tab_words, int W, uint32_t* out) {
  if (n <= 0 || !table_ok(W, tab_words)) return -1;
  Bufs b;
  const uint32_t* d_k = b.in(k, (size_t)8 * n);
  const uint32_t* d_tab = b.in(tab, tab_words);
  uint32_t* d_out = b.out<uint32_t>((size_t)27 * n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_comb, grid(n), dim3(64), 0, 0, d_k, d_tab, W, d_out, n);
  b.sync();
  b.back(out, d_out, (size_t)27 * n);
  return b.ok ? 0 : -3;
}

// xz: n x 18 limbs; out: n x 8 words
int sign_dev_r_of_point(const uint32_t* xz, int n, uint32_t* out) {
  if (n <= 0) return -1;
  Bufs b;
  const uint32_t* d_in = b.in(xz, (size_t)18 * n);
  uint32_t* d_out = b.out<uint32_t>((size_t)8 * n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_r_of_point, grid(n), dim3(64), 0, 0, d_in, d_out, n);
  b.sync();
  b.back(out, d_out, (size_t)8 * n);
  return b.ok ? 0 : -3;
}

// kde: n x 24 words; out: n x 16 words
int sign_dev_rs_of_k(const uint32_t* kde, int n, const uint32_t* tab, uint64_t tab_words, int W, uint32_t* out) {
  if (n <= 0 || !table_ok(W, tab_words)) return -1;
  Bufs b;
  const uint32_t* d_in = b.in(kde, (size_t)24 * n);
  const uint32_t* d_tab = b.in(tab, tab_words);
  uint32_t* d_out = b.out<uint32_t>((size_t)16 * n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_rs_of_k, grid(n), dim3(64), 0, 0, d_in, d_tab, W, d_out, n);
  b.sync();
  b.back(out, d_out, (size_t)16 * n);
  return b.ok ? 0 : -3;
}

// cand: n x (kSignTries + 1) x 8 words; count: n (each <= kSignTries + 1);
// de: n x 16 words; res: n x 20 words; tags: n x 72; uis: n x 88 bytes
int sign_dev_loop(const uint32_t* cand, const uint32_t* count, const uint32_t* de, int n, const uint32_t* tab,
                  uint64_t tab_words, int W, uint64_t first, uint64_t epoch, uint32_t* res, uint8_t* tags,
                  uint8_t* tag_len, uint8_t* uis, uint8_t* ui_len) {
  if (n <= 0 || !table_ok(W, tab_words)) return -1;
  for (int i = 0; i < n; i++)
    if (count[i] > (uint32_t)kMaxList) return -1;
  Bufs b;
  const uint32_t* d_cand = b.in(cand, (size_t)8 * kMaxList * n);
  const uint32_t* d_count = b.in(count, (size_t)n);
  const uint32_t* d_de = b.in(de, (size_t)16 * n);
  const uint32_t* d_tab = b.in(tab, tab_words);
  uint32_t* d_res = b.out<uint32_t>((size_t)20 * n);
  uint8_t* d_tags = b.out<uint8_t>((size_t)kTagSlot * n);
  uint8_t* d_tl = b.out<uint8_t>((size_t)n);
  uint8_t* d_uis = b.out<uint8_t>((size_t)kUiSlot * n);
  uint8_t* d_ul = b.out<uint8_t>((size_t)n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_loop, grid(n), dim3(64), 0, 0, d_cand, d_count, d_de, d_tab, W, first, epoch, d_res,
                     d_tags, d_tl, d_uis, d_ul, n);
  b.sync();
  b.back(res, d_res, (size_t)20 * n);
  b.back(tags, d_tags, (size_t)kTagSlot * n);
  b.back(tag_len, d_tl, (size_t)n);
  b.back(uis, d_uis, (size_t)kUiSlot * n);
  b.back(ui_len, d_ul, (size_t)n);
  return b.ok ? 0 : -3;
}

// d, e, k_out: n x 32 big-endian bytes; q: 32 bytes; tries: n
int sign_dev_nonce(const uint8_t* d, const uint8_t* e, const uint8_t* q, int n, uint8_t* k_out, int32_t* tries) {
  if (n <= 0) return -1;
  Bufs b;
  const uint8_t* d_d = b.in(d, (size_t)32 * n);
  const uint8_t* d_e = b.in(e, (size_t)32 * n);
  const uint8_t* d_q = b.in(q, 32);
  uint8_t* d_k = b.out<uint8_t>((size_t)32 * n);
  int32_t* d_t = b.out<int32_t>((size_t)n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_nonce, grid(n), dim3(64), 0, 0, d_d, d_e, d_q, d_k, d_t, n);
  b.sync();
  b.back(k_out, d_k, (size_t)32 * n);
  b.back(tries, d_t, (size_t)n);
  return b.ok ? 0 : -3;
}

// r, s: n x 32 big-endian bytes; tags: n x 72 (0xAA before the launch); lens: n
int sign_dev_der(const uint8_t* r, const uint8_t* s, int n, uint8_t* tags, uint8_t* lens) {
  if (n <= 0) return -1;
  Bufs b;
  const uint8_t* d_r = b.in(r, (size_t)32 * n);
  const uint8_t* d_s = b.in(s, (size_t)32 * n);
  uint8_t* d_tags = b.out<uint8_t>((size_t)kTagSlot * n);
  uint8_t* d_lens = b.out<uint8_t>((size_t)n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_der, grid(n), dim3(64), 0, 0, d_r, d_s, d_tags, d_lens, n);
  b.sync();
  b.back(tags, d_tags, (size_t)kTagSlot * n);
  b.back(lens, d_lens, (size_t)n);
  return b.ok ? 0 : -3;
}

// win: count x 16 words (1 <= count <= 32); mags: n; out: n x 16 words
int sign_dev_pick(const uint32_t* win, int count, const uint32_t* mags, int n, uint32_t* out) {
  if (n <= 0 || count < 1 || count > 32) return -1;
  Bufs b;
  const uint32_t* d_win = b.in(win, (size_t)16 * count);
  const uint32_t* d_mags = b.in(mags, (size_t)n);
  uint32_t* d_out = b.out<uint32_t>((size_t)16 * n);
  if (!b.ok) return -2;
  hipLaunchKernelGGL(k_pick, grid(n), dim3(64), 0, 0, d_win, count, d_mags, d_out, n);
  b.sync();
  b.back(out, d_out, (size_t)16 * n);
  return b.ok ? 0 : -3;
}

}  // extern "C"
