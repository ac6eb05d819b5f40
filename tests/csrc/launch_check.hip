// Test-only harness (tests/test_gpu_tables.py, tests/test_gpu_ninv.py): calls
// the library's own host-side launchers (minbft_amd/csrc/kernels.h, linked
// from libminbft_amd.so) on caller-given host arrays and hands their raw
// device results back, so that Python can check every comb-table entry and
// every s^-1 plane against big-integer arithmetic.  Built into
// tests/liblaunch_check.so by __graft_entry__.build(); never part of the
// product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/kernels.h"

namespace {
constexpr int kLimbs = 9;  // fe29.h NL: limbs (planes) per value

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess; }
  template <class T> T* as() { return static_cast<T*>(p); }
};
}  // namespace

extern "C" {

uint64_t table_check_entries(int wbits) { return mbft_launch::table_entries(wbits); }
uint64_t table_check_words(int wbits) { return mbft_launch::table_words(wbits); }
int table_check_steps(int wbits) { return mbft_launch::table_steps(wbits); }

// xy: npts x 16 LE words (plain affine x, y).  Builds the npts comb tables
// for window wbits (mbft_launch::build_tables) and copies back either every
// entry (idx null: out holds npts * table_entries * 16 words) or the nidx
// entries at the given global indices (out: nidx * 16 words).
int table_check_run(const uint32_t* xy, int npts, int wbits, const uint64_t* idx, long nidx,
                    uint32_t* out) {
  if (npts <= 0 || wbits < mbft_launch::kMinWindow || wbits > mbft_launch::kMaxWindow) return -1;
  const size_t ent = mbft_launch::table_entries(wbits);
  const size_t total = ent * (size_t)npts;
  if (idx)
    for (long k = 0; k < nidx; k++)
      if (idx[k] >= total) return -1;
  DevBuf d_xy, d_b, d_tab;
  if (!d_xy.alloc(64 * (size_t)npts) ||
      !d_b.alloc(64 * (size_t)npts * (size_t)mbft_launch::table_steps(wbits)) ||
      !d_tab.alloc(64 * total))
    return -2;
  if (hipMemcpy(d_xy.p, xy, 64 * (size_t)npts, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_tab.p, 0xEE, 64 * total) != hipSuccess)
    return -3;
  if (mbft_launch::build_tables(d_xy.as<uint32_t>(), npts, wbits, d_b.as<uint32_t>(),
                                d_tab.as<uint32_t>(), nullptr) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return -4;
  if (!idx)
    return hipMemcpy(out, d_tab.p, 64 * total, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
  for (long k = 0; k < nidx; k++)
    if (hipMemcpy(out + 16 * k, d_tab.as<uint32_t>() + 16 * idx[k], 64, hipMemcpyDeviceToHost) !=
        hipSuccess)
      return -5;
  return 0;
}

// s: n x 32 big-endian bytes.  planes_out: 9 x n words, limb k of item i at
// k * n + i: the s^-1 planes of form 0 (the level chain, batch_inverse_s with
// a workspace of ninv_workspace_words(n)), 1 (batch_inverse_s_local) or 2
// (batch_inverse_s_pipelined).
int ninv_check_run(int form, const uint8_t* s, long n, uint32_t* planes_out) {
  if (n <= 0 || form < 0 || form > 2) return -1;
  DevBuf d_s, d_w, d_ws, d_zero;
  const size_t pbytes = 4 * (size_t)kLimbs * (size_t)n;
  if (!d_s.alloc(32 * (size_t)n) || !d_w.alloc(pbytes) || !d_zero.alloc(4) ||
      !d_ws.alloc(form == 0 ? 4 * mbft_launch::ninv_workspace_words(n) : 4))
    return -2;
  if (hipMemcpy(d_s.p, s, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_w.p, 0xEE, pbytes) != hipSuccess || hipMemset(d_zero.p, 0xEE, 4) != hipSuccess)
    return -3;
  hipError_t e;
  if (form == 0)
    e = mbft_launch::batch_inverse_s(d_s.as<uint8_t>(), n, d_ws.as<uint32_t>(), d_w.as<uint32_t>(),
                                     d_zero.as<uint32_t>(), nullptr);
  else if (form == 1)
    e = mbft_launch::batch_inverse_s_local(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(),
                                           d_zero.as<uint32_t>(), nullptr);
  else
    e = mbft_launch::batch_inverse_s_pipelined(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(),
                                               d_zero.as<uint32_t>(), nullptr);
  if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -4;
  uint32_t zero = 1;
  if (hipMemcpy(planes_out, d_w.p, pbytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&zero, d_zero.p, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return -5;
  return zero == 0 ? 0 : -6;  // every form zeroes the word it is handed
}

}  // extern "C"
