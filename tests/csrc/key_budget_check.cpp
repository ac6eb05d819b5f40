// Test-only: the key memory budget's plan (minbft_amd/csrc/key_plan.h: class
// cost, use bins, ladder rule, rebalance_plan) on the HOST, as a stand-alone
// program (tests/test_key_budget.py).  It reads commands, one a line, from
// standard input and answers each on standard output; the test compares the
// answers with a Python model.  Built into tests/key_budget_check by
// __graft_entry__.build(); the test may build it again with AddressSanitizer
// and UBSan (host code only) and run it as a program.
//
//   bin U                      -> key_use_bin
//   low BIN                    -> key_use_bin_low
//   cost CLS                   -> key_class_cost (0: unknown code)
//   ladder L C0 .. C(L-1)      -> rebalance_ladder_ok as 0 / 1 (L may be 0 .. 16)
//   plan L C0 .. AVAIL MIN NB  -> then NB lines "BIN COUNT": "BYTES EXCESS
//                                 BLOCKED_BIN BLOCKED_RUNG" and the 496 rungs as digits
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../minbft_amd/csrc/key_plan.h"

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "bin")) {
      uint64_t u;
      if (scanf("%" SCNu64, &u) != 1) return 1;
      printf("%d\n", mbft::key_use_bin(u));
    } else if (!strcmp(cmd, "low")) {
      int b;
      if (scanf("%d", &b) != 1 || b < 0 || b >= mbft::kUseBins) return 1;
      printf("%" PRIu64 "\n", mbft::key_use_bin_low(b));
    } else if (!strcmp(cmd, "cost")) {
      unsigned cls;
      if (scanf("%u", &cls) != 1) return 1;
      printf("%u\n", mbft::key_class_cost(cls));
    } else if (!strcmp(cmd, "ladder") || !strcmp(cmd, "plan")) {
      size_t L;
      if (scanf("%zu", &L) != 1 || L > 16) return 1;
      std::vector<uint32_t> cls(L);
      for (size_t j = 0; j < L; j++) {
        unsigned v;
        if (scanf("%u", &v) != 1) return 1;
        cls[j] = v;
      }
      const bool ok = mbft::rebalance_ladder_ok(cls.data(), L);
      if (cmd[0] == 'l') {
        printf("%d\n", ok ? 1 : 0);
        continue;
      }
      uint64_t avail, minu;
      size_t nb;
      if (scanf("%" SCNu64 " %" SCNu64 " %zu", &avail, &minu, &nb) != 3) return 1;
      std::vector<uint64_t> hist(mbft::kUseBins, 0);
      for (size_t k = 0; k < nb; k++) {
        int b;
        uint64_t cnt;
        if (scanf("%d %" SCNu64, &b, &cnt) != 2 || b < 0 || b >= mbft::kUseBins) return 1;
        hist[(size_t)b] = cnt;
      }
      if (!ok) return 3;  // the plan is defined for ladders that pass the rule
      const mbft::RebalancePlan p = mbft::rebalance_plan(hist.data(), cls.data(), L, avail, minu);
      printf("%" PRIu64 " %" PRIu64 " %d %d\n", p.bytes, p.excess, p.blocked_bin, p.blocked_rung);
      for (int b = 0; b < mbft::kUseBins; b++) putchar('0' + p.rung_of_bin[b]);
      putchar('\n');
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 1;
    }
  }
  return 0;
}
