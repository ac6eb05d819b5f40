// Test-only harness (tests/test_gpu_key_rank.py): the key memory budget's
// ranking kernels k_key_age, k_key_hist and k_key_pick through the library's
// own launchers (mbft_launch::key_age / key_hist / key_pick_plan /
// key_pick_cold, linked from libminbft_amd.so) on INJECTED descriptors and
// counter arrays -- no context, no signature -- and the results handed back.
// Every output buffer carries one guard element past its end, uploaded from
// the caller and handed back, which the kernels must not touch.  Every HIP
// call is checked; nothing is launched after a failure.  Built into
// tests/libkey_rank_check.so by __graft_entry__.build(); never part of the
// product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../minbft_amd/csrc/kernels.h"

using namespace mbft_launch;

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
template <class T> bool down(T* h, const T* d, size_t count) {
  return hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) == hipSuccess;
}

// The store as the kernels read it: descriptors from cls / valid, the parts
// (nparts arrays of nslots counters, one after the other) and the ladder.
bool make_rank(Bufs& b, const uint32_t* cls, const uint8_t* valid, uint32_t nslots, const uint64_t* parts, int nparts,
               const uint32_t* ladder, int nladder, KeyRank* r) {
  if (!cls || !valid || nparts < 0 || nparts > kRankParts || nladder < 0 || nladder > kRankLadder) return false;
  if ((nparts && !parts) || (nladder && !ladder)) return false;
  std::vector<mbft::KeyDesc> kd(nslots);
  for (uint32_t k = 0; k < nslots; k++) kd[k] = mbft::KeyDesc{nullptr, cls[k], valid[k] ? 1u : 0u};
  *r = KeyRank{};
  r->keys = b.up(kd.data(), kd.size());
  r->nslots = nslots;
  r->nparts = nparts;
  for (int p = 0; p < nparts; p++) r->part[p] = b.up(parts + (size_t)p * nslots, nslots);
  r->nladder = nladder;
  for (int j = 0; j < nladder; j++) r->ladder[j] = ladder[j];
  return true;
}
}  // namespace

extern "C" {

// All return 0, or -1 after a HIP failure, -2 for arguments out of range.

// uses / rejects: n + 1 counters in and out (the last one the guard).
int key_rank_age(uint64_t* uses, uint64_t* rejects, size_t n, unsigned shift) {
  if (!uses || !rejects || shift < 1 || shift > 63) return -2;
  Bufs b;
  uint64_t* du = b.up(uses, n + 1);
  uint64_t* dr = b.up(rejects, n + 1);
  if (!b.ok) return -1;
  if (key_age(du, dr, n, shift, nullptr) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return down(uses, du, n + 1) && down(rejects, dr, n + 1) ? 0 : -1;
}

// dst: n + 1 counters in and out; src: n.
int key_rank_add(uint64_t* dst, const uint64_t* src, size_t n) {
  if (!dst || !src) return -2;
  Bufs b;
  uint64_t* dd = b.up(dst, n + 1);
  uint64_t* ds = b.up(src, n);
  if (!b.ok) return -1;
  if (key_add(dd, ds, n, nullptr) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return down(dst, dd, n + 1) ? 0 : -1;
}

// out: kRankHistWords + 1 words in (anything: the launcher zeroes them) and out.
int key_rank_hist(const uint32_t* cls, const uint8_t* valid, uint32_t nslots, const uint64_t* parts, int nparts,
                  const uint32_t* ladder, int nladder, uint32_t* out) {
  Bufs b;
  KeyRank r;
  if (!out || !make_rank(b, cls, valid, nslots, parts, nparts, ladder, nladder, &r)) return -2;
  uint32_t* d_out = b.up(out, (size_t)kRankHistWords + 1);
  if (!b.ok) return -1;
  if (key_hist(r, d_out, nullptr) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return down(out, d_out, (size_t)kRankHistWords + 1) ? 0 : -1;
}

// rung_of_bin: kRankBins bytes.  cap[t]: list t's capacity; lists: the lists one
// after the other, cap[t] + 1 words each (the last one a guard), in and out.
// count: kRankLadder + 1 words in and out.
int key_rank_pick_plan(const uint32_t* cls, const uint8_t* valid, uint32_t nslots, const uint64_t* parts, int nparts,
                       const uint32_t* ladder, int nladder, const uint8_t* rung_of_bin, const uint32_t* cap,
                       uint32_t* lists, uint32_t* count) {
  Bufs b;
  KeyRank r;
  if (!rung_of_bin || !cap || !lists || !count ||
      !make_rank(b, cls, valid, nslots, parts, nparts, ladder, nladder, &r))
    return -2;
  size_t total = 0;
  for (int t = 0; t < nladder; t++) total += (size_t)cap[t] + 1;
  uint32_t* d_lists = b.up(lists, total);
  uint32_t* d_count = b.up(count, (size_t)kRankLadder + 1);
  uint8_t* d_rob = b.up(rung_of_bin, (size_t)kRankBins);
  if (!b.ok) return -1;
  KeyPickLists l{};
  size_t off = 0;
  for (int t = 0; t < nladder; t++) {
    l.list[t] = d_lists + off;
    l.cap[t] = cap[t];
    off += (size_t)cap[t] + 1;
  }
  if (key_pick_plan(r, d_rob, l, d_count, nullptr) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return down(lists, d_lists, total) && down(count, d_count, (size_t)kRankLadder + 1) ? 0 : -1;
}

// list: cap + 1 words in and out; count: 2 words in and out (the second the guard).
int key_rank_pick_cold(const uint32_t* cls, const uint8_t* valid, uint32_t nslots, const uint64_t* parts, int nparts,
                       uint64_t max_uses, uint32_t cap, uint32_t* list, uint32_t* count) {
  Bufs b;
  KeyRank r;
  if (!list || !count || !make_rank(b, cls, valid, nslots, parts, nparts, nullptr, 0, &r)) return -2;
  uint32_t* d_list = b.up(list, (size_t)cap + 1);
  uint32_t* d_count = b.up(count, 2);
  if (!b.ok) return -1;
  if (key_pick_cold(r, max_uses, d_list, cap, d_count, nullptr) != hipSuccess) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return down(list, d_list, (size_t)cap + 1) && down(count, d_count, 2) ? 0 : -1;
}

}  // extern "C"
