// The verifier kernels' argument block and status bytes: what the host-side
// dispatch (verify_large.hip mbft_launch::verify) fills and every verify unit
// reads.  Global namespace, as the kernels that take it (their symbols carry
// the type's name).
#pragma once
#include <stdint.h>

#include "kernels.h"

using namespace mbft;

struct VerifyArgs {
  const uint8_t* e;        // n x 32 B big-endian digest integer (hashToInt)
  const uint8_t* r;        // n x 32 B big-endian
  const uint8_t* s;        // n x 32 B big-endian
  const uint32_t* slot;    // n key slots
  const uint32_t* winv;    // optional: s^-1 * R mod N, 9 planes of n (or null)
  const uint32_t* tabG;    // generator comb table (window wg)
  const KeyDesc* keys;     // nslots key descriptors (comb table, window, valid)
  uint32_t nslots;
  int wg;
  long n;
  uint8_t* status;
  uint32_t* slowq;         // exact-path queue: item indices (n entries)
  uint32_t* slown;         // its length (zeroed before k_verify)
  uint32_t host_status;    // bit 0: slots >= kHostSlot carry the host's status (batch pipeline);
                           // bit 1 (kArgTableFree): the context holds a table-free key -- the
                           // second queue (ladder_queue, ladder_count) is live
  uint32_t* scr;           // per-thread spill of the rare comb steps: 36 planes of sstride words
  uint32_t sstride;        // = threads in the grid
  const uint32_t* ndev;    // optional (small-batch kernels): the item count on the device, <= n
  const uint32_t* uhost = nullptr;  // optional (k_verify_split): u1, u2 per item, 16 LE words (host)
};
constexpr uint32_t kArgHostStatus = 1u, kArgTableFree = 2u;

constexpr uint8_t ST_ACCEPT = 0, ST_REJECT = 1, ST_BAD_KEY = 5;
