// Test-only: runs the table-free ladder's recoding (minbft_amd/csrc/ladder_dev.h:
// naf_init, naf_next) on the HOST, so the CPU suite can check its digits
// against Python integers (tests/test_ladder_host.py).  Built into
// tests/libladder_check.so by __graft_entry__.build().
#include "../../minbft_amd/csrc/ladder_dev.h"

extern "C" {

int ladder_check_digits() { return mbft::kNafDigits; }

// Digits of n scalars (u: n x 32 big-endian bytes), from the TOP down as the
// ladder takes them: digits[i][j] = the j-th digit naf_next yields, i.e.
// d_(256 - j), j < kNafDigits (row stride kNafDigits).
int ladder_check_recode(const uint8_t* u, int n, int8_t* digits) {
  for (int i = 0; i < n; i++) {
    uint32_t U[8];
    for (int j = 0; j < 8; j++) {
      const uint8_t* p = u + 32 * i + 4 * (7 - j);
      U[j] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    mbft::NafTop f;
    mbft::naf_init(f, U);
    for (int j = 0; j < mbft::kNafDigits; j++) digits[mbft::kNafDigits * i + j] = (int8_t)mbft::naf_next(f);
  }
  return 0;
}

}  // extern "C"
