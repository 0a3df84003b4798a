// TEST-ONLY kernel (not part of libbjj_hip.so): block_invert (csrc/k_common.hpp), the workgroup-wide simultaneous inversion
// of the affine epilogue, on per-lane values chosen by the test (tests/test_gpu_devfuzz.py::test_block_invert_directed_lanes)
// instead of the uniformly random Z products K1 feeds it -- in the three instances that ship: 512 lanes with the division-step
// core (K1), 256 lanes with it (K1's two-workgroup shape), 512 lanes with the binary GCD (every other kernel).
// Every thread loads its own 9 raw limbs (Montgomery form, != 0, N-form below 2r: the documented contract), calls block_invert
// and stores the 9 limbs it receives.  All lanes of every workgroup take part: nothing returns before the barriers, the host
// passes blocks * BLOCK values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../babyjubjub-rs_amd/csrc/bjj_launch.hpp"
#define BJJ_PNIELS_LAYOUT 0
#include "../../babyjubjub-rs_amd/csrc/k_common.hpp"

template <int BLOCK, int CORE>
__global__ void __launch_bounds__(BLOCK) bi_kernel(const u32* __restrict__ in, u32* __restrict__ out) {
  __shared__ u32 lds[NL * 64];
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  Fr x;
#pragma unroll
  for (int k = 0; k < NL; k++) x.v[k] = in[i * NL + k];
  const Fr y = block_invert<BLOCK, CORE>(x, lds);
#pragma unroll
  for (int k = 0; k < NL; k++) out[i * NL + k] = y.v[k];
}

// variant: 0 = <512, INV_K1>, 1 = <256, INV_K1>, 2 = <512, INV_GCD>.  in, out: blocks * BLOCK records of 9 limb-words.
extern "C" __attribute__((visibility("default"))) int bi_run(int variant, const uint32_t* in, uint32_t* out, int blocks, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (blocks <= 0) return -1;
  (void)hipGetLastError();
  switch (variant) {
    case 0: hipLaunchKernelGGL((bi_kernel<512, INV_K1>), dim3(blocks), dim3(512), 0, st, in, out); break;
    case 1: hipLaunchKernelGGL((bi_kernel<256, INV_K1>), dim3(blocks), dim3(256), 0, st, in, out); break;
    case 2: hipLaunchKernelGGL((bi_kernel<512, INV_GCD>), dim3(blocks), dim3(512), 0, st, in, out); break;
    default: return -1;
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
extern "C" __attribute__((visibility("default"))) int bi_block(int variant) { return variant == 1 ? 256 : (variant == 0 || variant == 2) ? 512 : 0; }
