// Philox4x32-10, the counter-based generator behind every device-side draw (include/fastgrnn_hip.h: augment_draw,
// train_schedule).  The one definition, internal to each file that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fastgrnn {
namespace {

struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
    c = u32x4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

}  // namespace
}  // namespace fastgrnn
