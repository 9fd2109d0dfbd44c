// What the two schedule kernel files share (kernels_schedule.hip, kernels_rolling.hip): the kernel's view of a
// fastgrnn_schedule_desc, one pass of the keyed Feistel permutation and its inverse, and the learning-rate formulas.
// Philox itself stays in philox.h, which every file that includes this one includes first.
#pragma once
#include "common.h"
#include "philox.h"

namespace fastgrnn {
namespace {

struct sched_args {
  const int64_t* step;
  int32_t* index;
  float* lr;
  int32_t* iht_mode;
  int64_t* where;
  uint64_t ticks, log_len;
  uint32_t seed_lo, seed_hi;
  uint32_t N, half, mask;
  int B, world, rank;
  int num_epochs, trim_level, sparsify;
  int lr_kind, lr_lead;
  double lr_base, lr_min, gamma, stepsize, t_max;
  uint64_t step_size, reset;
};

// the smallest even k >= 2 with 2^k >= n (n < 2^31), halved: the width of one Feistel half
static inline uint32_t feistel_half(uint32_t n) {
  uint32_t k = 2;
  while (k < 32 && (1u << k) < n) k += 2;
  return k / 2;
}

static inline sched_args sched_args_of(const fastgrnn_schedule_desc& d, const int64_t* step, int32_t* index, float* lr,
                                       int32_t* iht_mode, int64_t* where) {
  sched_args a;
  a.step = step;
  a.index = index;
  a.lr = lr;
  a.iht_mode = iht_mode;
  a.where = where;
  a.ticks = (uint64_t)(d.N / (d.B * d.world));
  a.log_len = (uint64_t)d.log_len;
  a.seed_lo = (uint32_t)d.seed;
  a.seed_hi = (uint32_t)(d.seed >> 32);
  a.N = (uint32_t)d.N;
  a.half = feistel_half(a.N);
  a.mask = (1u << a.half) - 1u;
  a.B = d.B;
  a.world = d.world;
  a.rank = d.rank;
  a.num_epochs = d.num_epochs;
  a.trim_level = d.trim_level;
  a.sparsify = d.sparsify;
  a.lr_kind = d.lr_kind;
  a.lr_lead = d.lr_lead;
  a.lr_base = d.lr_base;
  a.lr_min = d.lr_min;
  a.gamma = d.gamma;
  a.stepsize = d.stepsize;
  a.t_max = d.t_max;
  a.step_size = (uint64_t)d.step_size;
  a.reset = (uint64_t)d.reset;
  return a;
}

// x < 2^(2 half) -> another; a bijection of that range for every key (Feistel).  The counter is (R, c1, c2, tag | r):
// tag = 0x80000000 for an epoch's clip order (c = the epoch), 0xC0000000 for an iteration's bag shuffle (c = the step)
__device__ __forceinline__ uint32_t feistel_pass(uint32_t x, uint32_t half, uint32_t mask, uint32_t c1, uint32_t c2,
                                                 uint32_t tag, uint32_t k0, uint32_t k1) {
  uint32_t L = x >> half, R = x & mask;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint32_t p = philox4x32_10(u32x4{R, c1, c2, tag | r}, k0, k1).x;
    const uint32_t t = L ^ (p & mask);
    L = R;
    R = t;
  }
  return (L << half) | R;
}

// the inverse pass: the rounds backwards
__device__ __forceinline__ uint32_t feistel_unpass(uint32_t x, uint32_t half, uint32_t mask, uint32_t c1, uint32_t c2,
                                                   uint32_t tag, uint32_t k0, uint32_t k1) {
  uint32_t L = x >> half, R = x & mask;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t r = 3u - i;
    const uint32_t p = philox4x32_10(u32x4{L, c1, c2, tag | r}, k0, k1).x;
    const uint32_t t = R ^ (p & mask);
    R = L;
    L = t;
  }
  return (L << half) | R;
}

__device__ __forceinline__ double lr_of(const sched_args& a, uint64_t s) {
  const uint64_t it_n = s + (uint64_t)a.lr_lead;               // (s <= 2^63 - 1: no wrap)
  const double it = (double)it_n, span = a.lr_base - a.lr_min;
  switch (a.lr_kind) {
    case 1: {
      const double c = floor(1.0 + it / (2.0 * a.stepsize));
      const double x = fabs(it / a.stepsize - 2.0 * c + 1.0);
      return a.lr_min + span * pow(a.gamma, it / 3.0) * x;
    }
    case 2: return a.lr_min + span * (1.0 + cos(3.14159265358979323846 * it / a.t_max)) / 2.0;
    case 3: return a.lr_base * pow(a.gamma, it);
    case 4: return a.lr_base * pow(a.gamma, (double)(it_n / a.step_size));
    case 5: return a.lr_base * pow(a.gamma, (double)(it_n > a.reset ? it_n - a.reset : it_n));
    default: return a.lr_base;
  }
}

// train_update's code of the IHT phase at (epoch, i_batch)
__device__ __forceinline__ int iht_phase_of(const sched_args& a, uint64_t epoch, uint64_t i_batch) {
  if (!a.sparsify) return 0;
  const uint64_t e3 = 3u * (epoch < (uint64_t)a.num_epochs ? epoch : (uint64_t)a.num_epochs);     // (no overflow)
  if (e3 < (uint64_t)a.num_epochs) return 0;
  return (e3 < 2u * (uint64_t)a.num_epochs && i_batch % (uint64_t)a.trim_level == 0) ? 1 : 2;
}

}  // namespace
}  // namespace fastgrnn
