// The IHT threshold phase shared by the two update kernels (kernels_update.hip: Adam / SGD; kernels_optim.hip: the other
// six rules of torch.optim), as mfcc_body.h is shared by the two front ends.  One workgroup of UPD_THREADS per parameter
// tensor; thread t owns elements t, t + UPD_THREADS, ... here as in the update that precedes it, so a thread only ever
// USES values it stored itself and nothing but the workgroup's barriers orders anything.
// The threshold is found exactly by radix select on the magnitudes' bit patterns (for non-NaN fp32, bits & 0x7fffffff
// orders as an unsigned integer): four 8-bit passes from the top, each a 256-bin histogram in LDS of the elements that
// still match the digits chosen so far.  Integer LDS atomics: the counts do not depend on arrival order.
#pragma once
#include "common.h"

namespace fastgrnn {
namespace {

constexpr int UPD_THREADS = 1024;

// b^e for an integer e >= 0 by squaring, in double (at most 63 steps; its rounding error, ~1e-14 relative, is far
// below the fp32 arithmetic it feeds)
__device__ double ipow(double b, long long e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__device__ __forceinline__ unsigned mag_key(float v) { return __builtin_bit_cast(unsigned, v) & 0x7fffffffu; }

// Hard threshold of p[0..n) (utils.hardThreshold): zero what lies strictly below the magnitude of 0-based rank
// keep_rank (1 <= keep_rank < n) among the ascending magnitudes, and write the support bytes.  Called by every thread
// of the workgroup (it holds barriers); hist[256] and s_sel[2] are the caller's LDS.
__device__ __forceinline__ void iht_threshold(float* p, unsigned char* sup, const int n, const int keep_rank,
                                              unsigned* hist, unsigned* s_sel) {
  const int tid = threadIdx.x;
  // the key of 0-based rank keep_rank among the ascending magnitudes, most significant digit first
  unsigned prefix = 0, known = 0, rank = (unsigned)keep_rank;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();                                           // (also orders this thread's stores of p in front of its loads)
    for (int i0 = tid; i0 < n; i0 += 4 * UPD_THREADS) {
      unsigned k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)                              // (no branch around the loads: second rule of DESIGN.md 4.0)
        k[j] = mag_key(p[min(i0 + j * UPD_THREADS, n - 1)]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {                            // (every lane adds, 0 where it does not count: no branch either)
        const bool counts = i0 + j * UPD_THREADS < n && (k[j] & known) == prefix;
        atomicAdd(&hist[(k[j] >> shift) & 255u], counts ? 1u : 0u);
      }
      lds_writes_landed();                                     // (second rule of DESIGN.md 4.0: the next iteration's loads)
    }
    __syncthreads();
    if (tid < 64) {                                            // wave 0: the bin that holds the rank, by a scan over 64 x 4 bins
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned own = c0 + c1 + c2 + c3;
      unsigned inc = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d);
        if (tid >= d) inc += t;
      }
      const unsigned exc = inc - own;
      if (rank >= exc && rank < inc) {                         // exactly one lane: the counts sum to more than rank
        unsigned r = rank - exc, bin = 4u * tid;
        if (r >= c0) { r -= c0; ++bin;
          if (r >= c1) { r -= c1; ++bin;
            if (r >= c2) { r -= c2; ++bin; } } }
        s_sel[0] = prefix | (bin << shift);
        s_sel[1] = r;
      }
    }
    __syncthreads();
    prefix = s_sel[0];
    rank = s_sel[1];
    known |= 255u << shift;
  }
  // prefix is now the threshold's bit pattern: strictly smaller magnitudes go, ties stay (utils.hardThreshold)
  for (int i = tid; i < n; i += UPD_THREADS) {
    float pn = p[i];
    if (mag_key(pn) < prefix) {
      pn = 0.f;
      p[i] = 0.f;
    }
    sup[i] = pn != 0.f ? 1 : 0;
  }
}

}  // namespace
}  // namespace fastgrnn
