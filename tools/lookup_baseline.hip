// Baseline of tools/lookup_bench.py: the only inversion the library had before
// the batched one, one fe_inv (a Fermat power, about 380 dependent products)
// per element, one lane each, as k_poly_leaves uses it once per point.
// Built by the tool into tools/mb_lookup_baseline.so (git-ignored):
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -Izk-research-implementations_amd/csrc \
//         -o tools/mb_lookup_baseline.so tools/lookup_baseline.hip
// BLS12-381 Fr, Montgomery tables on the device, timed by the launch's own events.
#include <hip/hip_runtime.h>

#include "field.hpp"

using zk::Fe;
using F = zk::Bls12_381Fr;

__global__ __launch_bounds__(256) void k_inverse_each(const Fe* __restrict__ in, Fe* __restrict__ out, uint64_t count) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) out[i] = zk::fe_inv<F>(in[i]);
}

// One launch over count elements; returns the kernel's milliseconds, or -1 on an error.
extern "C" float lookup_baseline_inverse_ms(const void* d_in, void* d_out, uint64_t count) {
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1.f;
  const uint64_t blocks = (count + 255) / 256;
  const uint32_t grid = (uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20));
  (void)hipEventRecord(a, nullptr);
  k_inverse_each<<<grid, 256>>>(reinterpret_cast<const Fe*>(d_in), reinterpret_cast<Fe*>(d_out), count);
  (void)hipEventRecord(b, nullptr);
  float ms = -1.f;
  if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = -1.f;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return ms;
}
