// The key store's bookkeeping after registration: key class codes and their
// cost, the free list of released slot numbers, the per-class lists of
// released storage pieces, the dirty ranges of the descriptor upload and the
// choice of the keys a promotion re-classes, and the memory budget's plan (the
// modelled cost of a class, the use-count bins, the ladder rule,
// rebalance_plan).  Plain C++, no HIP: host.cpp and keys.cpp act on what these
// decide (tests/csrc/key_plan_check.cpp and key_budget_check.cpp drive them
// on the CPU); key_rank.hip shares the bin map.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace mbft {

// A key class as KeyDesc.wbits carries it (the public code of
// mbft_set_key_class): a comb window 4 .. 29, 0 (table-free), or
// 0x100 | t for a compact key of t = 2 .. 8 teeth, or 0x200 | t for a signed
// compact key of t = 2 .. 9 teeth.
constexpr uint32_t kClassTeeth = 0x100u;
constexpr uint32_t kClassSignedTeeth = 0x200u;
constexpr bool key_class_known(uint32_t cls) {
  return cls == 0u || (cls >= 4u && cls <= 29u) || (cls >= (kClassTeeth | 2u) && cls <= (kClassTeeth | 8u)) ||
         (cls >= (kClassSignedTeeth | 2u) && cls <= (kClassSignedTeeth | 9u));
}
// Bytes of one key's verification data in class cls (64 B an entry): the
// order of the classes wherever one is "cheaper" than another.
constexpr uint64_t key_class_bytes(uint32_t cls) {
  if (cls == 0u) return 64u;
  if (cls >= kClassSignedTeeth) return (uint64_t)64u << ((cls & 0xFFu) - 1u);  // 2^(t-1) entries
  if (cls >= kClassTeeth) return (uint64_t)64u << (cls & 0xFFu);
  const uint32_t w = cls, S = (256u + w - 1u) / w;
  return 64u * (((uint64_t)(S - 1u) << (w - 1u)) + ((uint64_t)1u << (256u - (S - 1u) * w)));
}

// Released slot numbers: the next registration takes them first, lowest first.
class SlotList {
 public:
  void release(uint32_t slot) { free_.insert(slot); }
  bool empty() const { return free_.empty(); }
  size_t size() const { return free_.size(); }
  bool holds(uint32_t slot) const { return free_.count(slot) != 0; }
  // the m lowest free numbers (all of them if fewer), ascending, without taking them
  std::vector<uint32_t> lowest(size_t m) const {
    std::vector<uint32_t> v;
    for (auto it = free_.begin(); it != free_.end() && v.size() < m; ++it) v.push_back(*it);
    return v;
  }
  uint32_t take() {
    const uint32_t s = *free_.begin();
    free_.erase(free_.begin());
    return s;
  }
  void clear() { free_.clear(); }

 private:
  std::set<uint32_t> free_;
};

// Released storage, one list of pieces per class: a piece is the address of
// one key's data (a 64-B entry, a table of 2^t entries, a comb table), every
// piece of a class the same size.  take() hands out the piece released last
// (its lines are the likeliest to be mapped still), 0 when the class has none.
class PieceLists {
 public:
  void release(uint32_t cls, uintptr_t piece) {
    lists_[cls].push_back(piece);
    bytes_ += key_class_bytes(cls);
  }
  uintptr_t take(uint32_t cls) {
    auto it = lists_.find(cls);
    if (it == lists_.end() || it->second.empty()) return 0;
    const uintptr_t p = it->second.back();
    it->second.pop_back();
    bytes_ -= key_class_bytes(cls);
    return p;
  }
  size_t count(uint32_t cls) const {
    auto it = lists_.find(cls);
    return it == lists_.end() ? 0 : it->second.size();
  }
  uint64_t bytes() const { return bytes_; }
  void clear() {
    lists_.clear();
    bytes_ = 0;
  }

 private:
  std::map<uint32_t, std::vector<uintptr_t>> lists_;
  uint64_t bytes_ = 0;
};

// The descriptor entries changed since the last upload, as sorted disjoint
// half-open ranges [lo, hi): touching or overlapping marks are merged, so a
// run of neighbours goes up as one copy.
class DirtyRanges {
 public:
  void mark(size_t lo, size_t hi) {
    if (lo >= hi) return;
    auto it = r_.lower_bound(lo);
    if (it != r_.begin()) {
      auto pv = std::prev(it);
      if (pv->second >= lo) it = pv;
    }
    while (it != r_.end() && it->first <= hi) {
      lo = std::min(lo, it->first);
      hi = std::max(hi, it->second);
      it = r_.erase(it);
    }
    r_[lo] = hi;
  }
  void mark(size_t i) { mark(i, i + 1); }
  bool empty() const { return r_.empty(); }
  std::vector<std::pair<size_t, size_t>> ranges() const {
    return std::vector<std::pair<size_t, size_t>>(r_.begin(), r_.end());
  }
  void clear() { r_.clear(); }

 private:
  std::map<size_t, size_t> r_;
};

// The keys mbft_promote_hot_keys re-classes into cls: valid slots whose class
// is cheaper in memory than cls and whose uses are >= min_uses, the max_keys
// of them with the most uses (ties: the lower slot first), returned in that
// order.
inline std::vector<uint32_t> promotion_choice(const uint64_t* uses, const uint32_t* cls_of, const uint8_t* valid,
                                              size_t nslots, uint32_t cls, size_t max_keys, uint64_t min_uses) {
  std::vector<uint32_t> pick;
  const uint64_t target = key_class_bytes(cls);
  for (size_t i = 0; i < nslots; i++)
    if (valid[i] && uses[i] >= min_uses && key_class_bytes(cls_of[i]) < target) pick.push_back((uint32_t)i);
  std::stable_sort(pick.begin(), pick.end(), [&](uint32_t a, uint32_t b) { return uses[a] > uses[b]; });
  if (pick.size() > max_keys) pick.resize(max_keys);
  return pick;
}

// ---------------------------------------------------------------------------
// The memory budget (mbft_rebalance_keys): what a class costs
// a verify, the bins the use counts are ranked in, and the plan that gives
// every bin a class.

// The MODELLED field reductions of u2 Q in class cls -- a model from the
// headers' own counts (doubling 8, mixed addition 10), NOT a measurement: a
// comb window W adds once per window, 10 ceil(256 / W); the table-free ladder
// is 256 doublings and 86 additions, 2,908; a compact key of t teeth, signed or
// not, walks d = ceil(256 / t) columns at a doubling and an addition each but
// for the first, 18 d - 8 (§4.10: a compact key's time follows its columns).
// 0 for an unknown code.
constexpr uint32_t key_class_cost(uint32_t cls) {
  if (!key_class_known(cls)) return 0u;
  if (cls == 0u) return 256u * 8u + 86u * 10u;
  if (cls >= kClassTeeth) return 18u * ((256u + (cls & 0xFFu) - 1u) / (cls & 0xFFu)) - 8u;
  return 10u * ((256u + cls - 1u) / cls);
}

// One definition for the host and the device (key_rank.hip), as teeth_dev.h's
// recoding: in a HIP translation unit the functions carry both attributes.
#ifdef __HIP__
#define MBFT_PLAN_HD __host__ __device__ inline
#else
#define MBFT_PLAN_HD inline
#endif

// A use count's bin: monotone, exact below 16, then eight bins an octave (the
// top three bits under the leading one) up to 2^64 - 1 in bin 495.
constexpr int kUseBins = 496;
MBFT_PLAN_HD int key_use_bin(uint64_t u) {
  if (u < 16u) return (int)u;
  const int e = 63 - __builtin_clzll(u);
  return 16 + 8 * (e - 4) + (int)((u >> (e - 3)) & 7u);
}
// the smallest count of a bin
MBFT_PLAN_HD uint64_t key_use_bin_low(int bin) {
  if (bin < 16) return (uint64_t)bin;
  const int e = 4 + (bin - 16) / 8;
  return (uint64_t)(8 + (bin - 16) % 8) << (e - 3);
}

// A ladder is the classes a rebalance may give a key, cheapest in memory
// first: 1 .. kLadderMax known codes, bytes strictly ascending, cost strictly
// descending, and the gain per byte of each step, g_j = (c_j - c_(j+1)) /
// (b_(j+1) - b_j), strictly decreasing (compared by cross-multiplication; the
// products stay below 2^50).  A rung that costs more than a smaller one is
// dominated and refused: a comb window 4 above signed 9 teeth.
constexpr size_t kLadderMax = 8;
inline bool rebalance_ladder_ok(const uint32_t* classes, size_t L) {
  if (!classes || L < 1 || L > kLadderMax) return false;
  for (size_t j = 0; j < L; j++)
    if (!key_class_known(classes[j])) return false;
  for (size_t j = 0; j + 1 < L; j++)
    if (key_class_bytes(classes[j]) >= key_class_bytes(classes[j + 1]) ||
        key_class_cost(classes[j]) <= key_class_cost(classes[j + 1]))
      return false;
  for (size_t j = 0; j + 2 < L; j++) {
    const uint64_t dc0 = key_class_cost(classes[j]) - key_class_cost(classes[j + 1]);
    const uint64_t dc1 = key_class_cost(classes[j + 1]) - key_class_cost(classes[j + 2]);
    const uint64_t db0 = key_class_bytes(classes[j + 1]) - key_class_bytes(classes[j]);
    const uint64_t db1 = key_class_bytes(classes[j + 2]) - key_class_bytes(classes[j + 1]);
    if (dc0 * db1 <= dc1 * db0) return false;  // g_j > g_(j+1)
  }
  return true;
}

// The plan: hist[bin] ladder keys have a use count in bin, avail_bytes is what
// they may take in all.  Every key starts at rung 0; a STEP moves one bin's keys
// from rung j to j + 1, weighs key_use_bin_low(bin) g_j -- the modelled
// reductions saved per byte spent, at the bin's least count -- and costs
// hist[bin] (b_(j+1) - b_j) bytes.  Only non-empty bins whose least count is >=
// max(min_uses, 1) step.  Steps are taken in descending weight (exact, 128-bit
// cross-multiplication; ties: the higher bin, then the lower j) while the bytes
// stay <= avail_bytes, and the walk STOPS at the first step that does not fit: a
// prefix, not a knapsack.  g falls with j and the least count rises with the
// bin, so every prefix holds (bin, j - 1) before (bin, j) and (bin + 1, j)
// before (bin, j): rung_of_bin is non-decreasing in the bin, and the plan reads
// "a key goes to the rung of its use bin".  All keys of a bin get one rung, so
// `bytes` computed from the histogram is exact; the budget is left unused by
// less than the blocked step's bytes.  If rung 0 alone exceeds avail_bytes the
// plan is all rung 0 and `excess` is by how much.
struct RebalancePlan {
  uint8_t rung_of_bin[kUseBins];
  uint64_t bytes;           // the ladder keys' bytes under the plan
  uint64_t excess;          // bytes - avail_bytes where rung 0 does not fit, else 0
  int blocked_bin, blocked_rung;  // the step that did not fit (from blocked_rung up), -1: none was left
};
inline RebalancePlan rebalance_plan(const uint64_t* hist, const uint32_t* classes, size_t L, uint64_t avail_bytes,
                                    uint64_t min_uses) {
  typedef unsigned __int128 u128;
  RebalancePlan p{};
  p.blocked_bin = p.blocked_rung = -1;
  u128 total = 0;
  for (int b = 0; b < kUseBins; b++) total += (u128)hist[b] * key_class_bytes(classes[0]);
  if (total > avail_bytes) {
    p.bytes = (uint64_t)total;
    p.excess = (uint64_t)(total - avail_bytes);
    return p;
  }
  struct Step {
    int bin, j;
  };
  std::vector<Step> steps;
  const uint64_t floor_uses = min_uses > 1u ? min_uses : 1u;
  for (int b = 0; b < kUseBins; b++)
    if (hist[b] != 0 && key_use_bin_low(b) >= floor_uses)
      for (size_t j = 0; j + 1 < L; j++) steps.push_back(Step{b, (int)j});
  auto dc = [&](int j) { return (u128)(key_class_cost(classes[j]) - key_class_cost(classes[j + 1])); };
  auto db = [&](int j) { return (u128)(key_class_bytes(classes[j + 1]) - key_class_bytes(classes[j])); };
  std::sort(steps.begin(), steps.end(), [&](const Step& x, const Step& y) {
    // low dc / db, both sides times db_x db_y: below 2^64 2^12 2^38
    const u128 wx = (u128)key_use_bin_low(x.bin) * dc(x.j) * db(y.j);
    const u128 wy = (u128)key_use_bin_low(y.bin) * dc(y.j) * db(x.j);
    if (wx != wy) return wx > wy;
    if (x.bin != y.bin) return x.bin > y.bin;
    return x.j < y.j;
  });
  for (const Step& s : steps) {
    const u128 more = (u128)hist[s.bin] * db(s.j);
    if (total + more > avail_bytes) {
      p.blocked_bin = s.bin;
      p.blocked_rung = s.j;
      break;
    }
    total += more;
    p.rung_of_bin[s.bin] = (uint8_t)(s.j + 1);
  }
  p.bytes = (uint64_t)total;
  return p;
}

}  // namespace mbft
