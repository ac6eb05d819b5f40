// Test-only harness (tests/test_gpu_key_account.py): the use-count stage
// k_key_account through the library's own launcher (mbft_launch::key_account,
// linked from libminbft_amd.so) on INJECTED slot words, statuses, descriptors
// and device count -- no context, no signature -- and the counters handed back.
// Every HIP call is checked; nothing is launched after a failure.  Built into
// tests/libkey_account_check.so by __graft_entry__.build(); never part of the
// product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../minbft_amd/csrc/kernels.h"

namespace {
struct Bufs {
  std::vector<void*> dev;
  bool ok = true;
  ~Bufs() {
    for (void* p : dev) (void)hipFree(p);
  }
  template <class T> T* up(const T* h, size_t count) {
    void* d = nullptr;
    if (!ok || hipMalloc(&d, sizeof(T) * (count ? count : 1)) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    dev.push_back(d);
    if (count && hipMemcpy(d, h, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return static_cast<T*>(d);
  }
};
}  // namespace

extern "C" {

// slot / status: `cap` entries each (cap >= n: what lies past the count the
// kernel is given must not be read).  valid: nslots bytes, the descriptors'
// valid words.  count < 0: no device count; else *ndev = count.  uses /
// rejects: nslots + 1 counters in and out (the last one a guard the kernel
// must not touch).  `launches` launches into the same counters.  Returns 0, or
// -1 after a HIP failure, -2 for arguments that would read out of bounds.
int key_account_run(const uint32_t* slot, const uint8_t* status, long n, long cap, long count,
                    const uint8_t* valid, uint32_t nslots, int launches, uint64_t* uses, uint64_t* rejects) {
  if (n < 0 || cap < n || launches < 1 || launches > 8 || !slot || !status || !valid || !uses || !rejects) return -2;
  if (count > cap) return -2;
  std::vector<mbft::KeyDesc> kd(nslots);
  for (uint32_t k = 0; k < nslots; k++) kd[k] = mbft::KeyDesc{nullptr, 16u, valid[k] ? 1u : 0u};
  Bufs b;
  const uint32_t cnt = count < 0 ? 0u : (uint32_t)count;
  uint32_t* d_slot = b.up(slot, (size_t)cap);
  uint8_t* d_status = b.up(status, (size_t)cap);
  mbft::KeyDesc* d_kd = b.up(kd.data(), kd.size());
  uint32_t* d_cnt = b.up(&cnt, 1);
  uint64_t* d_uses = b.up(uses, (size_t)nslots + 1);
  uint64_t* d_rej = b.up(rejects, (size_t)nslots + 1);
  if (!b.ok) return -1;
  for (int l = 0; l < launches; l++) {
    const mbft_launch::KeyAccount a{d_slot, d_status, n, count < 0 ? nullptr : d_cnt, d_kd, nslots, d_uses, d_rej};
    if (mbft_launch::key_account(a, nullptr) != hipSuccess) return -1;
  }
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(uses, d_uses, sizeof(uint64_t) * ((size_t)nslots + 1), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(rejects, d_rej, sizeof(uint64_t) * ((size_t)nslots + 1), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}

}  // extern "C"
