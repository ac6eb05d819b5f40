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

}  // namespace mbft_launch
