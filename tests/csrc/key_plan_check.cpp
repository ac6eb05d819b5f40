// Test-only: the key store's bookkeeping (minbft_amd/csrc/key_plan.h) and the
// use-count stage's grid (verify_plan.h) on the HOST, as a stand-alone program
// (tests/test_key_plan.py).  It reads commands, one a line, from standard
// input and answers each on standard output; the test compares the answers
// with a Python model.  Built into tests/key_plan_check by
// __graft_entry__.build(); the test may build it again with
// AddressSanitizer and UBSan (host code only) and run it as a program.
//
//   bytes CLS                  -> key_class_bytes, or -1 for an unknown code
//   srel SLOT | stake          -> release a slot number | take one (-1: none)
//   slow M                     -> the M lowest free slot numbers, not taken
//   reg KEY CLS                -> key KEY gets a piece of class CLS: its address
//   rec KEY CLS                -> re-class: the new piece first, then the old one released
//   rem KEY                    -> the key's piece released
//   pstat                      -> pieces listed, bytes listed, fresh pieces made
//   mark LO HI | dirty         -> mark [LO, HI) | print and clear the ranges
//   promote N CLS MAX MIN      -> then N lines "USES CLASS VALID": the chosen slots
//   blocks N NCU               -> key_account_blocks
//   plan N ACC                 -> account flag of a large batch's plan
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>

#include "../../minbft_amd/csrc/key_plan.h"
#include "../../minbft_amd/csrc/verify_plan.h"

int main() {
  mbft::SlotList slots;
  mbft::PieceLists pieces;
  mbft::DirtyRanges dirty;
  std::map<long, std::pair<uint32_t, uintptr_t>> keys;  // key -> class, piece
  std::set<uintptr_t> live;                             // pieces a key holds now
  uintptr_t next = 0x1000;                              // fresh pieces: a bump allocator
  unsigned long fresh = 0;
  auto piece_for = [&](uint32_t cls) {
    uintptr_t p = pieces.take(cls);
    if (!p) {
      p = next;
      next += (uintptr_t)mbft::key_class_bytes(cls);
      fresh++;
    }
    if (!live.insert(p).second) {
      fprintf(stderr, "piece %" PRIxPTR " handed out twice\n", p);
      exit(2);
    }
    return p;
  };
  auto give_back = [&](uint32_t cls, uintptr_t p) {
    live.erase(p);
    pieces.release(cls, p);
  };
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "bytes")) {
      unsigned cls;
      if (scanf("%u", &cls) != 1) return 1;
      if (mbft::key_class_known(cls))
        printf("%" PRIu64 "\n", mbft::key_class_bytes(cls));
      else
        printf("-1\n");
    } else if (!strcmp(cmd, "srel")) {
      unsigned s;
      if (scanf("%u", &s) != 1) return 1;
      slots.release(s);
      printf("%zu\n", slots.size());
    } else if (!strcmp(cmd, "stake")) {
      if (slots.empty())
        printf("-1\n");
      else
        printf("%u\n", slots.take());
    } else if (!strcmp(cmd, "slow")) {
      size_t m;
      if (scanf("%zu", &m) != 1) return 1;
      for (uint32_t v : slots.lowest(m)) printf("%u ", v);
      printf("\n");
    } else if (!strcmp(cmd, "reg") || !strcmp(cmd, "rec")) {
      long k;
      unsigned cls;
      if (scanf("%ld %u", &k, &cls) != 2) return 1;
      const bool re = cmd[2] == 'c';
      if (re != (keys.count(k) != 0)) return 3;
      const uintptr_t p = piece_for(cls);  // the new data first ...
      if (re) give_back(keys[k].first, keys[k].second);  // ... then the old storage
      keys[k] = {cls, p};
      printf("%" PRIuPTR "\n", p);
    } else if (!strcmp(cmd, "rem")) {
      long k;
      if (scanf("%ld", &k) != 1) return 1;
      auto it = keys.find(k);
      if (it == keys.end()) return 3;
      give_back(it->second.first, it->second.second);
      printf("%" PRIuPTR "\n", it->second.second);
      keys.erase(it);
    } else if (!strcmp(cmd, "pstat")) {
      size_t listed = 0;
      for (uint32_t c = 0; c <= (mbft::kClassTeeth | 8u); c++) listed += pieces.count(c);
      printf("%zu %" PRIu64 " %lu %zu\n", listed, pieces.bytes(), fresh, live.size());
    } else if (!strcmp(cmd, "mark")) {
      size_t lo, hi;
      if (scanf("%zu %zu", &lo, &hi) != 2) return 1;
      dirty.mark(lo, hi);
      printf("ok\n");
    } else if (!strcmp(cmd, "dirty")) {
      for (auto& r : dirty.ranges()) printf("%zu-%zu ", r.first, r.second);
      printf("\n");
      dirty.clear();
    } else if (!strcmp(cmd, "promote")) {
      size_t n, maxk;
      unsigned cls;
      uint64_t minu;
      if (scanf("%zu %u %zu %" SCNu64, &n, &cls, &maxk, &minu) != 4) return 1;
      std::vector<uint64_t> uses(n);
      std::vector<uint32_t> co(n);
      std::vector<uint8_t> valid(n);
      for (size_t i = 0; i < n; i++) {
        unsigned c, v;
        if (scanf("%" SCNu64 " %u %u", &uses[i], &c, &v) != 3) return 1;
        co[i] = c;
        valid[i] = (uint8_t)v;
      }
      for (uint32_t s : mbft::promotion_choice(uses.data(), co.data(), valid.data(), n, cls, maxk, minu))
        printf("%u ", s);
      printf("\n");
    } else if (!strcmp(cmd, "blocks")) {
      long n, ncu;
      if (scanf("%ld %ld", &n, &ncu) != 2) return 1;
      printf("%ld\n", mbft::key_account_blocks(n, ncu));
    } else if (!strcmp(cmd, "plan")) {
      long n;
      int acc;
      if (scanf("%ld %d", &n, &acc) != 2) return 1;
      const mbft::VerifyPlan base = mbft::verify_plan(n, mbft::InvSource::kBatch, false, true, 256, 2);
      const mbft::VerifyPlan p = mbft::verify_plan_account(base, acc != 0);
      printf("%d %d %d %ld\n", (int)base.account, (int)p.account, (int)(p.form == base.form), p.threads);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 1;
    }
  }
  return 0;
}
