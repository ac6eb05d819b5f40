// Test-only GPU harness over the P-384 class, built into
// tests/libp384_check.so:
//  * p384_check_run: the operations of p384_check_ops.inc -- the same table
//    tests/csrc/p384_host_check.cpp runs on the host -- one item per lane, for
//    tests/test_gpu_p384_field.py;
//  * p384_check_launch: mbft_launch::verify_p384 under a plan made by hand
//    (the grid given in blocks), for tests/test_gpu_p384_passes.py;
//  * p384_check_plan / p384_check_cus: the product's plan for n items.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/kernels.h"
#include "../../minbft_amd/csrc/p384_ecc.h"
#include "p384_check_ops.inc"

namespace {

// in: n x P384_OP_MAX_IN x 14 words, out: n x P384_OP_MAX_OUT x 14 words.  One
// kernel per operation: everything is inlined into it.
template <int OP>
__global__ void __launch_bounds__(64) k_p384_ops(const uint32_t* in, uint32_t* out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t a[P384_OP_MAX_IN][P384_OP_WORDS], o[P384_OP_MAX_OUT][P384_OP_WORDS];
#pragma unroll
  for (int k = 0; k < P384_OP_MAX_IN; k++)
#pragma unroll
    for (int w = 0; w < P384_OP_WORDS; w++) a[k][w] = in[(i * P384_OP_MAX_IN + k) * P384_OP_WORDS + w];
#pragma unroll
  for (int k = 0; k < P384_OP_MAX_OUT; k++)
#pragma unroll
    for (int w = 0; w < P384_OP_WORDS; w++) o[k][w] = 0;
  p384_op_run(OP, a, o);
#pragma unroll
  for (int k = 0; k < P384_OP_MAX_OUT; k++)
#pragma unroll
    for (int w = 0; w < P384_OP_WORDS; w++) out[(i * P384_OP_MAX_OUT + k) * P384_OP_WORDS + w] = o[k][w];
}

template <int OP>
void launch_ops(int op, const uint32_t* in, uint32_t* out, long n) {
  if (op == OP)
    hipLaunchKernelGGL(k_p384_ops<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
  else if constexpr (OP + 1 < OP_COUNT)
    launch_ops<OP + 1>(op, in, out, n);
}

}  // namespace

extern "C" {

// host buffers in and out; 0 or the HIP error
int p384_check_run(int op, const uint32_t* in, uint32_t* out, long n) {
  if (op < 0 || op >= OP_COUNT || n <= 0) return -1;
  const size_t ib = (size_t)n * P384_OP_MAX_IN * P384_OP_WORDS * 4, ob = (size_t)n * P384_OP_MAX_OUT * P384_OP_WORDS * 4;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, ib);
  if (e == hipSuccess) e = hipMalloc(&d_out, ob);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_ops<0>(op, d_in, d_out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

int p384_check_op_code(const char* name) { return p384_op_code(name); }

// device buffers (16-byte aligned), the grid in blocks of 256
int p384_check_launch(const uint8_t* d_e, const uint8_t* d_r, const uint8_t* d_s, const uint8_t* d_xy, long n,
                      uint8_t* d_status, long blocks, void* stream) {
  const mbft_launch::P384Batch b{d_e, d_r, d_s, d_xy, n, d_status};
  const mbft::P384Plan plan{((n + 255) / 256) * 256, blocks};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = mbft_launch::verify_p384(b, plan, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return (int)e;
}

int p384_check_cus() { return mbft_launch::device_cus(); }

long p384_check_plan_blocks(long n) { return mbft::verify_p384_plan(n, mbft_launch::device_cus()).blocks; }

}  // extern "C"
