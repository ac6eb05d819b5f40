// Stand-alone HOST program (its own main) over the verified-call memo's plan
// (minbft_amd/csrc/memo_plan.h) and the memo flag of the launch plan
// (verify_plan.h), driven by tests/test_memo_plan.py with commands on stdin,
// one a line, answers on stdout, one line each:
//   geometry BYTES              -> entries bytes            (0 0: below the minimum)
//   consts                      -> entry_bytes entry_words probe min_entries tuple_words empty busy
//   hash W0 .. W24              -> the 64-bit hash (decimal)
//   bucket ENTRIES W0 .. W24    -> bucket tag
//   probe ENTRIES HASH          -> the kMemoProbe entries of the sequence
//   rotate ENTRIES C1 C2 ...    -> per pass "due young rotations" (a due rotation is performed at once)
//   scratch N                   -> count e r s slot origin status bytes
//   plan N HAS_COUNT ACCOUNT MEMO -> form account memo
// Built by __graft_entry__.build_memo_check_host(); never part of the library.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../minbft_amd/csrc/memo_plan.h"
#include "../../minbft_amd/csrc/verify_plan.h"

using namespace mbft;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "geometry") {
      uint64_t b = 0;
      in >> b;
      const MemoGeometry g = memo_geometry(b);
      printf("%" PRIu64 " %" PRIu64 "\n", g.entries, g.bytes);
    } else if (cmd == "consts") {
      printf("%zu %zu %d %" PRIu64 " %d %u %u\n", kMemoEntryBytes, kMemoEntryWords, kMemoProbe, kMemoMinEntries,
             kMemoTupleWords, kMemoEmpty, kMemoBusy);
    } else if (cmd == "hash" || cmd == "bucket") {
      uint64_t entries = 0;
      if (cmd == "bucket") in >> entries;
      std::vector<uint32_t> w(kMemoTupleWords, 0u);
      for (int i = 0; i < kMemoTupleWords; i++) in >> w[i];
      if (!in || (cmd == "bucket" && (entries == 0 || (entries & (entries - 1)) != 0))) {
        printf("error\n");
        continue;
      }
      const uint64_t h = memo_hash(w.data());
      if (cmd == "hash")
        printf("%" PRIu64 "\n", h);
      else
        printf("%" PRIu64 " %u\n", memo_bucket(h, entries), memo_tag(h));
    } else if (cmd == "probe") {
      uint64_t entries = 0, h = 0;
      in >> entries >> h;
      if (!in || entries == 0 || (entries & (entries - 1)) != 0) {
        printf("error\n");
        continue;
      }
      for (int j = 0; j < kMemoProbe; j++) printf("%s%" PRIu64, j ? " " : "", memo_probe_at(h, j, entries));
      printf("\n");
    } else if (cmd == "rotate") {
      MemoRotation r;
      in >> r.entries;
      uint64_t calls = 0;
      bool first = true;
      while (in >> calls) {
        const bool due = r.add(calls);
        if (due) r.rotate();
        printf("%s%d %d %" PRIu64, first ? "" : " ", due ? 1 : 0, r.young, r.rotations);
        first = false;
      }
      printf("\n");
    } else if (cmd == "scratch") {
      size_t n = 0;
      in >> n;
      const MemoScratch m = memo_scratch(n);
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", m.count, m.e, m.r, m.s, m.slot, m.origin, m.status, m.bytes);
    } else if (cmd == "plan") {
      long n = 0;
      int has_count = 0, account = 0, memo = 0;
      in >> n >> has_count >> account >> memo;
      const InvSource src = verify_inv_source(n, 4096, false, has_count != 0);
      const VerifyPlan base = verify_plan(n, src, has_count != 0, true, 256, 2);
      const VerifyPlan p = verify_plan_memo(verify_plan_account(base, account != 0), memo != 0);
      printf("%d %d %d %d\n", (int)p.form, p.account ? 1 : 0, p.memo ? 1 : 0, base.memo ? 1 : 0);
    } else {
      printf("error\n");
    }
  }
  return 0;
}
