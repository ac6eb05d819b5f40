// Test-only: the inline-key form's launch plan (minbft_amd/csrc/verify_plan.h,
// verify_keys_plan) on the HOST, as a stand-alone program
// (tests/test_inline_keys_plan.py).  It reads commands, one a line, from
// standard input and answers each on standard output; the test compares the
// answers with a Python model.  Built into tests/inline_keys_plan_check by
// __graft_entry__.build(); the test builds it again with AddressSanitizer and
// UBSan (host code only) and runs it as a program.
//
//   plan N LANE_INV_MAX NCU -> "LANE_INV THREADS BLOCKS"
//   bpc                     -> kKeysBpc
#include <stdio.h>
#include <string.h>

#include "../../minbft_amd/csrc/verify_plan.h"

// the plan is a constant expression, as the launcher's callers may need it
static_assert(mbft::verify_keys_plan(4096, 4096, 256).lane_inv && !mbft::verify_keys_plan(4097, 4096, 256).lane_inv,
              "lane inverse up to lane_inv_max, planes above");
static_assert(mbft::verify_keys_plan(1L << 28, 4096, 256).threads == (1L << 28), "no overflow at 2^28");

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "plan")) {
      long n, ncu;
      unsigned long long lim;
      if (scanf("%ld %llu %ld", &n, &lim, &ncu) != 3) return 1;
      const mbft::KeysPlan p = mbft::verify_keys_plan(n, (size_t)lim, ncu);
      printf("%d %ld %ld\n", p.lane_inv ? 1 : 0, p.threads, p.blocks);
    } else if (!strcmp(cmd, "bpc")) {
      printf("%ld\n", mbft::kKeysBpc);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 1;
    }
  }
  return 0;
}
