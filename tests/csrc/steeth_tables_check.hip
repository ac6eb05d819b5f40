// Test-only harness (tests/test_gpu_steeth_tables.py): calls the library's own
// launcher of the signed compact key class's table build
// (mbft_launch::build_steeth_tables, minbft_amd/csrc/kernels.h, linked from
// libminbft_amd.so) on caller-given points and hands the raw tables back, so
// that Python can compare entries with the oracle's scalar multiples byte
// for byte.  Built into tests/libsteeth_tables_check.so by
// __graft_entry__.build(); never part of the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/kernels.h"

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess; }
  template <class T> T* as() { return static_cast<T*>(p); }
};
}  // namespace

extern "C" {

uint64_t steeth_tables_check_words(int teeth) { return mbft_launch::steeth_table_words(teeth); }

// xy: npts x 16 LE words (plain affine x, y).  Builds the npts tables for
// `teeth` and copies every entry back (out: npts * 2^(teeth - 1) * 16 words).
int steeth_tables_check_run(const uint32_t* xy, int npts, int teeth, uint32_t* out) {
  if (npts <= 0 || teeth < mbft_launch::kSteethMin || teeth > mbft_launch::kSteethMax) return -1;
  const size_t bytes = 4 * mbft_launch::steeth_table_words(teeth) * (size_t)npts;
  DevBuf d_xy, d_tab;
  if (!d_xy.alloc(64 * (size_t)npts) || !d_tab.alloc(bytes)) return -2;
  if (hipMemcpy(d_xy.p, xy, 64 * (size_t)npts, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_tab.p, 0xEE, bytes) != hipSuccess)
    return -3;
  if (mbft_launch::build_steeth_tables(d_xy.as<uint32_t>(), npts, teeth, d_tab.as<uint32_t>(), nullptr) !=
          hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return -4;
  return hipMemcpy(out, d_tab.p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
}

}  // extern "C"
