// The key store's bookkeeping after registration: key class codes and their
// cost, the free list of released slot numbers, the per-class lists of
// released storage pieces, the dirty ranges of the descriptor upload and the
// choice of the keys a promotion re-classes.  Plain C++, no HIP: host.cpp
// acts on what these decide (tests/csrc/key_plan_check.cpp drives them on the
// CPU).
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

}  // namespace mbft
