// Launchers the verify dispatch (verify_large.hip mbft_launch::verify) calls in
// the other kernel units: each unit launches the kernels it defines.  Internal
// to the .hip units; the host includes kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify_args.h"

namespace mbft_launch {

// ninv_kernels.hip: the s^-1 R planes of a small batch, one item per lane
// (k_ninv_local<1>) -- what verify() runs first where the plan says so.  ndev
// (optional): the item count on the device, <= n.
hipError_t batch_inverse_s_small(const uint8_t* s, long n, uint32_t* winv, const uint32_t* ndev, hipStream_t st);
// verify_pairs.hip: k_verify_pairs<lane_inv>
void verify_pairs(const VerifyArgs& A, bool lane_inv, dim3 grid, hipStream_t st);
// verify_quads.hip: k_verify_quads<inline_inv>
void verify_quads(const VerifyArgs& A, bool inline_inv, dim3 grid, hipStream_t st);
// verify_split.hip: k_verify_split<split_wide()>, one workgroup per item
void verify_split(const VerifyArgs& A, hipStream_t st);
// k_verify_split's and k_verify_server's additions: lane-group parallel
// (default) or sequential (env MBFT_SPLIT_WIDE=0)
bool split_wide();

}  // namespace mbft_launch
