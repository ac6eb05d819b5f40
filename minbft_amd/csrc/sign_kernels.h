// Host-side launch wrapper for the batch signer in sign_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minbft_gpu.h"

namespace mbft_launch {

// where a lane's digest input e comes from
enum SignMode : int {
  kSignPrehashed = 0,  // e: n x 32 bytes
  kSignFlat = 1,       // raw AuthenBytes msgs[msg_off[i] .. msg_off[i+1]): e = (m || SHA256(""))[0:32]
  kSignRecords = 2     // message records over an arena: REQUEST / REPLY / REQ-VIEW-CHANGE
};

// signer generator-table windows (4: 64 additions, 33 KB; 5: 52, 52 KB; 6: 43, 87 KB);
// the default is the fastest measured (tools/sign_probe.py)
constexpr int kSignMinWindow = 4, kSignMaxWindow = 6, kSignDefaultWindow = 5;

struct SignTagArgs {
  int mode;
  int w;                    // window of tab
  long n;
  const uint8_t* e;         // kSignPrehashed (4-byte aligned)
  const uint8_t* msgs;      // kSignFlat
  const uint32_t* msg_off;  // kSignFlat: n + 1
  const mbft_msg_rec* recs; // kSignRecords
  const uint8_t* bytes;     // kSignRecords: the arena (fields validated by the host)
  const uint8_t* key0;      // 32 B big-endian: the call's role; kSignRecords: the replica key
  const uint8_t* key1;      // kSignRecords: the client key (REQUEST)
  const uint32_t* tab;      // the signer's generator table (build_tables layout, window w)
  uint8_t* tags;            // n x 72
  uint8_t* tag_len;         // n
};

hipError_t sign_tags(const SignTagArgs& a, hipStream_t st);

// where a lane's message digest SHA256(m) comes from (k_usig_uis)
enum UsigMode : int {
  kUsigDigests = 0,  // given: n x 32 bytes
  kUsigFlat = 1,     // raw messages msgs[msg_off[i] .. msg_off[i+1])
  kUsigRecords = 2   // PREPARE / COMMIT records over an arena (AuthenBytes built in the kernel)
};

// One UI per lane: lane i signs SHA256(SHA256(m_i) || epoch_le64 || (first + i)_le64).
struct UsigArgs {
  int mode;
  int w;                    // window of tab
  long n;
  uint64_t epoch, first;    // the instance's epoch; the counter of lane 0
  const uint8_t* digests;   // kUsigDigests (4-byte aligned)
  const uint8_t* msgs;      // kUsigFlat
  const uint32_t* msg_off;  // kUsigFlat: n + 1
  const mbft_msg_rec* recs; // kUsigRecords (types and fields validated by the host)
  const uint8_t* bytes;     // kUsigRecords: the arena
  const uint8_t* key;       // 32 B big-endian: the USIG's private key
  const uint32_t* tab;      // the signer's generator table (window w)
  uint8_t* uis;             // n x MBFT_UI_SLOT
  uint8_t* ui_len;          // n (0: no usable nonce in kSignTries candidates)
};

hipError_t usig_uis(const UsigArgs& a, hipStream_t st);
// affine d G (X || Y, 64 bytes big-endian) through the signer's uniform comb:
// the public key of a secret d, 0 < d < N (the USIG identity)
hipError_t sign_pubkey(const uint8_t* key, const uint32_t* tab, int w, uint8_t* xy, hipStream_t st);

}  // namespace mbft_launch
