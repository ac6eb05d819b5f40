// Test-only harness (tests/test_gpu_memo_stage.py): the verified-call memo's
// two stages, k_memo_probe and k_memo_commit, through the library's own
// launchers (mbft_launch::memo_probe / memo_commit, linked from
// libminbft_amd.so) on INJECTED items, slot words, descriptors, device count,
// table image and, optionally, a forced hash per item -- no context, no
// signature -- and every output handed back.  Every HIP call is checked;
// nothing is launched after a failure.  Built into tests/libmemo_check.so by
// __graft_entry__.build(); never part of the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../minbft_amd/csrc/kernels.h"
#include "../../minbft_amd/csrc/memo_plan.h"

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
  template <class T> bool down(T* h, const T* d, size_t count) {
    return count == 0 || hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess;
  }
};
}  // namespace

extern "C" {

int memo_check_probe_steps(void) { return mbft::kMemoProbe; }

// One run over a table of two generations of `entries` entries (image: 2 *
// entries * 32 words, generation 0 the young one, in and out).
//   e, r, s (32 B an item), slot, status: `cap` items each, cap >= n; count < 0:
//     no device count, else *ndev = count (<= cap).  valid: nslots bytes.
//   hash: null, or `cap` forced hashes of the items.
//   do_probe: k_memo_probe over the items.  The compacted outputs e_c, r_c, s_c,
//     slot_c, origin, each `cap` items and in AND out (guard patterns survive where
//     the kernel must not write), and *miss.
//   do_commit: k_memo_commit over the compacted items.  After a probe they are the
//     probe's (the forced hashes follow the items through origin); without one they
//     are e_c .. origin and *miss as given.  status_c (`cap` bytes, in): the
//     verifier's statuses of the compacted items.
//   stats: 4 counters, in and out.
// Returns 0, -1 after a HIP failure, -2 for arguments that would read out of bounds.
int memo_check_run(const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint32_t* slot, uint8_t* status,
                   long n, long cap, long count, const uint8_t* valid, uint32_t nslots, const uint64_t* hash,
                   uint32_t* image, uint64_t entries, int do_probe, int do_commit, uint8_t* e_c, uint8_t* r_c,
                   uint8_t* s_c, uint32_t* slot_c, uint32_t* origin, uint32_t* miss, const uint8_t* status_c,
                   uint64_t* stats) {
  if (n < 0 || cap < n || cap < 1 || count > cap || !e || !r || !s || !slot || !status || !valid || !image || !e_c ||
      !r_c || !s_c || !slot_c || !origin || !miss || !status_c || !stats)
    return -2;
  if (entries < mbft::kMemoMinEntries || (entries & (entries - 1)) != 0) return -2;
  if (!do_probe && (long)*miss > cap) return -2;
  std::vector<mbft::KeyDesc> kd(nslots);
  for (uint32_t k = 0; k < nslots; k++) kd[k] = mbft::KeyDesc{nullptr, 16u, valid[k] ? 1u : 0u};
  Bufs b;
  const size_t C = (size_t)cap, tab_words = (size_t)(2 * entries) * mbft::kMemoEntryWords;
  const uint32_t cnt = count < 0 ? 0u : (uint32_t)count;
  uint8_t* d_e = b.up(e, 32 * C);
  uint8_t* d_r = b.up(r, 32 * C);
  uint8_t* d_s = b.up(s, 32 * C);
  uint32_t* d_slot = b.up(slot, C);
  uint8_t* d_status = b.up(status, C);
  mbft::KeyDesc* d_kd = b.up(kd.data(), kd.size());
  uint32_t* d_cnt = b.up(&cnt, 1);
  uint64_t* d_hash = hash ? b.up(hash, C) : nullptr;
  uint32_t* d_tab = b.up(image, tab_words);
  uint8_t* d_ec = b.up(e_c, 32 * C);
  uint8_t* d_rc = b.up(r_c, 32 * C);
  uint8_t* d_sc = b.up(s_c, 32 * C);
  uint32_t* d_slotc = b.up(slot_c, C);
  uint32_t* d_origin = b.up(origin, C);
  const uint32_t miss0 = do_probe ? 0u : *miss;
  uint32_t* d_miss = b.up(&miss0, 1);
  uint8_t* d_statusc = b.up(status_c, C);
  uint64_t* d_stats = b.up(stats, (size_t)mbft_launch::kMemoStats);
  std::vector<uint64_t> hash_c(C, 0);
  uint64_t* d_hashc = hash ? b.up(hash_c.data(), C) : nullptr;
  if (!b.ok) return -1;
  uint32_t* young = d_tab;
  uint32_t* old = d_tab + (size_t)entries * mbft::kMemoEntryWords;
  if (do_probe) {
    const mbft_launch::MemoProbe p{d_e, d_r, d_s, d_slot, n, count < 0 ? nullptr : d_cnt, d_kd, nslots, young, old,
                                   entries, d_status, d_ec, d_rc, d_sc, d_slotc, d_origin, d_miss, d_stats, d_hash};
    if (mbft_launch::memo_probe(p, nullptr) != hipSuccess) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (!b.down(miss, d_miss, 1) || !b.down(origin, d_origin, C)) return -1;
    if ((long)*miss > n) return -1;
    if (hash) {  // the forced hashes follow the items
      for (uint32_t j = 0; j < *miss; j++) {
        if ((long)origin[j] >= n) return -1;
        hash_c[j] = hash[origin[j]];
      }
      if (hipMemcpy(d_hashc, hash_c.data(), 8 * C, hipMemcpyHostToDevice) != hipSuccess) return -1;
    }
  } else if (hash) {
    if (hipMemcpy(d_hashc, hash, 8 * C, hipMemcpyHostToDevice) != hipSuccess) return -1;
  }
  if (do_commit) {
    const mbft_launch::MemoCommit c{d_ec, d_rc, d_sc, d_slotc, d_origin, d_statusc, n, d_miss, d_kd, nslots, young,
                                    entries, d_status, d_stats, hash ? d_hashc : nullptr};
    if (mbft_launch::memo_commit(c, nullptr) != hipSuccess) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
  }
  if (!b.down(status, d_status, C) || !b.down(e_c, d_ec, 32 * C) || !b.down(r_c, d_rc, 32 * C) ||
      !b.down(s_c, d_sc, 32 * C) || !b.down(slot_c, d_slotc, C) || !b.down(origin, d_origin, C) ||
      !b.down(miss, d_miss, 1) || !b.down(image, d_tab, tab_words) ||
      !b.down(stats, d_stats, (size_t)mbft_launch::kMemoStats))
    return -1;
  return 0;
}

}  // extern "C"
