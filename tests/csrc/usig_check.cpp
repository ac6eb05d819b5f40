// Test-only: runs the software USIG's host-compilable device code on the HOST
// -- the digest chain SHA256(SHA256(m) || epoch_le64 || counter_le64)
// (minbft_amd/csrc/sha256_dev.h sha256_usig_chain) and the UI assembly
// counter_be64 || epoch_be64 || DER (minbft_amd/csrc/sign_dev.h usig_ui_write)
// -- so the CPU suite can check them against the oracle
// (tests/test_usig_host.py).  Built into tests/libusig_check.so by
// __graft_entry__.build().
#include <string.h>

#include "../../minbft_amd/csrc/sha256_dev.h"
#include "../../minbft_amd/csrc/sign_dev.h"

namespace {
void be_words(uint32_t w[8], const uint8_t* p) {
  for (int j = 0; j < 8; j++)
    w[j] = ((uint32_t)p[4 * j] << 24) | ((uint32_t)p[4 * j + 1] << 16) |
           ((uint32_t)p[4 * j + 2] << 8) | p[4 * j + 3];
}
}  // namespace

extern "C" {

// n signed digests: message i = msgs[off[i] .. off[i+1]), counter first + i.
// e_out: n x 32 bytes.
int usig_check_digest(const uint8_t* msgs, const uint32_t* off, int n, uint64_t epoch, uint64_t first,
                      uint8_t* e_out) {
  for (int i = 0; i < n; i++) {
    uint8_t dig[32];
    mbft::Sha256 h;
    h.init();
    h.update(msgs + off[i], off[i + 1] - off[i]);
    h.final(dig);
    uint32_t dw[8], ew[8];
    be_words(dw, dig);
    mbft::sha256_usig_chain(ew, dw, epoch, first + (uint64_t)i);
    for (int j = 0; j < 8; j++)
      for (int b = 0; b < 4; b++) e_out[32 * i + 4 * j + b] = (uint8_t)(ew[j] >> (24 - 8 * b));
  }
  return 0;
}

// n UIs from given signatures: r, s n x 32 big-endian bytes, counter first + i
// -> uis n x 88 (prefilled by the caller: the writer fills the whole slot),
// lens n.
int usig_check_ui(const uint8_t* r, const uint8_t* s, int n, uint64_t epoch, uint64_t first, uint8_t* uis,
                  uint8_t* lens) {
  for (int i = 0; i < n; i++) {
    uint32_t rw[8], sw[8];
    be_words(rw, r + 32 * i);
    be_words(sw, s + 32 * i);
    lens[i] = (uint8_t)mbft::usig_ui_write(uis + mbft::kUiSlot * i, first + (uint64_t)i, epoch, rw, sw);
  }
  return 0;
}

int usig_check_slot(void) { return mbft::kUiSlot; }

}  // extern "C"
