// The verified-call memo's plan (mbft_set_verified_memo): the
// entry, the table's shape from a byte budget, the hash and the probe sequence,
// the rotation rule and the scratch of one pass, decided ONCE.  Plain C++, no
// HIP: host.cpp and keys.cpp act on it, memo.hip's kernels share the hash, the
// tag and the probe sequence, tests/csrc/memo_plan_check.cpp drives it on the
// CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mbft {

#ifdef __HIP__
#define MBFT_MEMO_HD __host__ __device__ inline
#else
#define MBFT_MEMO_HD inline
#endif

// An entry: one 128-byte fabric line, 128-byte aligned.  Word 0 is the tag:
// kMemoEmpty, kMemoBusy (claimed, the payload not yet whole), anything else
// READY (the tuple's hash bits, memo_tag).  Word 1 the key slot, words 2 .. 25
// e, r, s as they lie in the batch (96 B), the rest padding.
// INVARIANT: between two clears an entry only ever goes empty -> busy ->
// ready; nothing overwrites a ready entry.  The exact compare of a hit rests
// on it: a ready tag seen behind the publisher's release means a whole payload
// that never changes again until the next clear, and a clear runs only while
// no pass is in flight.
constexpr size_t kMemoEntryBytes = 128, kMemoEntryWords = 32;
constexpr uint32_t kMemoEmpty = 0u, kMemoBusy = 1u;
constexpr int kMemoTupleWords = 25;  // slot, e[8], r[8], s[8]

// The probe sequence: the home bucket and the kMemoProbe - 1 entries after it
// (wrapping).  8, not 4: a generation rotates at 3/4 full, and an insert is
// dropped when its whole window is taken -- at that load roughly one in ten
// windows of 8 against one in three of 4 -- and a dropped insert costs a whole
// signature check later (about 420 VALU wave-instructions an item) where the
// four more steps cost a miss four more 4-byte tag loads.
constexpr int kMemoProbe = 8;

// Two generations (young and old), each `entries` entries, a power of two.
constexpr uint64_t kMemoMinEntries = 1024;
struct MemoGeometry {
  uint64_t entries;  // per generation; 0: the budget is below the minimum
  uint64_t bytes;    // 2 * entries * kMemoEntryBytes
};
constexpr MemoGeometry memo_geometry(uint64_t bytes) {
  const uint64_t per_gen = bytes / (2u * kMemoEntryBytes);
  if (per_gen < kMemoMinEntries) return {0, 0};
  uint64_t e = kMemoMinEntries;
  while (e <= per_gen / 2u) e <<= 1;
  return {e, 2u * e * kMemoEntryBytes};
}

// The hash: a 64-bit mix of the 25 words (a multiply-rotate per word and
// murmur3's finalizer).  It has to spread, not to resist: every hit is
// confirmed by comparing all 25 words.
MBFT_MEMO_HD uint64_t memo_hash(const uint32_t w[kMemoTupleWords]) {
  uint64_t h = 0x243F6A8885A308D3ull;
  for (int i = 0; i < kMemoTupleWords; i++) {
    h ^= (uint64_t)w[i];
    h *= 0x9E3779B97F4A7C15ull;
    h = (h << 27) | (h >> 37);
  }
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return h;
}
// The home bucket (the low bits), step j of the probe sequence, and the ready
// tag (the high bits, bit 1 forced: never kMemoEmpty or kMemoBusy).
MBFT_MEMO_HD uint64_t memo_bucket(uint64_t h, uint64_t entries) { return h & (entries - 1u); }
MBFT_MEMO_HD uint64_t memo_probe_at(uint64_t h, int j, uint64_t entries) {
  return (h + (uint64_t)j) & (entries - 1u);
}
MBFT_MEMO_HD uint32_t memo_tag(uint64_t h) { return (uint32_t)(h >> 32) | 2u; }

// The rotation rule.  After each pass the host adds the pass's unique-call
// count -- an upper bound on its inserts, so nothing is read back -- to the
// young generation's running count; at 3/4 of a generation's entries a
// rotation is due: the old generation is cleared, the roles swap, the count
// starts again.  An entry lives between one and two fills.
struct MemoRotation {
  uint64_t entries = 0;
  uint64_t young_calls = 0;
  int young = 0;  // the young generation's index (0 or 1)
  uint64_t rotations = 0;
  uint64_t threshold() const { return entries / 4u * 3u; }
  // the pass's calls; true: a rotation is due
  bool add(uint64_t calls) {
    young_calls += calls;
    return young_calls >= threshold();
  }
  // the generation to clear
  int rotate() {
    const int cleared = young ^ 1;
    young = cleared;
    young_calls = 0;
    rotations++;
    return cleared;
  }
};

// One pass's scratch for n items, per pipeline buffer k beside slowq[k]: a
// 64-byte block whose word 0 is the miss counter, then the compacted e, r, s
// (32 B an item), slot and origin words and status bytes, each 64-byte
// aligned.
struct MemoScratch {
  size_t count, e, r, s, slot, origin, status, bytes;
};
constexpr size_t memo_align64(size_t x) { return (x + 63u) & ~(size_t)63u; }
constexpr MemoScratch memo_scratch(size_t n) {
  MemoScratch m{};
  m.count = 0;
  m.e = 64;
  m.r = m.e + memo_align64(32u * n);
  m.s = m.r + memo_align64(32u * n);
  m.slot = m.s + memo_align64(32u * n);
  m.origin = m.slot + memo_align64(4u * n);
  m.status = m.origin + memo_align64(4u * n);
  m.bytes = m.status + memo_align64(n);
  return m;
}

}  // namespace mbft
