// Test-only: runs the compact key class's recoding (minbft_amd/csrc/teeth_dev.h:
// teeth_columns, teeth_column) on the HOST, so the CPU suite can check its
// columns against Python integers (tests/test_teeth_host.py).  Built into
// tests/libteeth_check.so by __graft_entry__.build().
#include "../../minbft_amd/csrc/teeth_dev.h"

extern "C" {

int teeth_check_columns(int t) { return mbft::teeth_columns(t); }

// Columns of n scalars (u: n x 32 big-endian bytes) for t teeth, in the order
// the evaluation takes them: cols[i][k] = v_(d - 1 - k), k < d (row stride d).
int teeth_check_recode(const uint8_t* u, int n, int t, uint8_t* cols) {
  if (t < mbft::kTeethMin || t > mbft::kTeethMax) return -1;
  const int d = mbft::teeth_columns(t);
  for (int i = 0; i < n; i++) {
    uint32_t U[8];
    for (int j = 0; j < 8; j++) {
      const uint8_t* p = u + 32 * i + 4 * (7 - j);
      U[j] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
    for (int k = 0; k < d; k++) cols[(long)d * i + k] = (uint8_t)mbft::teeth_column(U, t, d, d - 1 - k);
  }
  return 0;
}

}  // extern "C"

#ifdef TEETH_CHECK_MAIN
// Stand-alone run for the sanitizers (-fsanitize=address,undefined): every t
// over corner and pseudo-random scalars, each column set checked to rebuild
// its scalar.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main() {
  uint64_t x = 0x9e3779b97f4a7c15ull;
  long bad = 0;
  for (int t = mbft::kTeethMin; t <= mbft::kTeethMax; t++) {
    const int d = teeth_check_columns(t);
    uint8_t* cols = (uint8_t*)malloc((size_t)d);
    for (int it = 0; it < 2000; it++) {
      uint8_t u[32];
      for (int k = 0; k < 32; k++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        u[k] = it == 0 ? 0xFF : it == 1 ? 0x00 : (uint8_t)x;
      }
      if (teeth_check_recode(u, 1, t, cols) != 0) bad++;
      uint8_t back[32];
      memset(back, 0, 32);
      for (int k = 0; k < d; k++) {
        const int c = d - 1 - k;
        for (int j = 0; j < t; j++)
          if ((cols[k] >> j) & 1) {
            const int p = j * d + c;
            if (p >= 256) {
              bad++;
              continue;
            }
            back[31 - p / 8] |= (uint8_t)(1u << (p % 8));
          }
      }
      if (memcmp(back, u, 32) != 0) bad++;
    }
    free(cols);
  }
  printf("teeth_check: %ld mismatches\n", bad);
  return bad != 0;
}
#endif
