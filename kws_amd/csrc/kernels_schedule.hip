// What a trainer iteration needs from outside the model, as a function of the step count (include/fastgrnn_hip.h:
// fastgrnn_hip_train_schedule).  gfx950 only.
//   sched_k   one thread per clip of the batch: position q of the epoch's order -> clip number through a keyed
//             permutation of 0..N-1 (a four-round Feistel network on Philox4x32-10, cycle-walked into the range); thread 0
//             of block 0 also writes the learning rate (double, rounded once), the IHT phase and the position.
// No LDS, no atomics, plain stores; everything is a function of (descriptor, step[0]) alone.
#include "common.h"
#include "philox.h"

namespace fastgrnn {
namespace {

constexpr int SCHED_THREADS = 256;

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

// position x < 2^(2 half) of epoch e -> another; a bijection of that range for every key (Feistel)
__device__ __forceinline__ uint32_t feistel_pass(uint32_t x, const sched_args& a, uint32_t e_lo, uint32_t e_hi) {
  uint32_t L = x >> a.half, R = x & a.mask;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint32_t p = philox4x32_10(u32x4{R, e_lo, e_hi, 0x80000000u | r}, a.seed_lo, a.seed_hi).x;
    const uint32_t t = L ^ (p & a.mask);
    L = R;
    R = t;
  }
  return (L << a.half) | R;
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

__global__ __launch_bounds__(SCHED_THREADS) void sched_k(sched_args a) {
  const int b = blockIdx.x * SCHED_THREADS + threadIdx.x;
  if (b >= a.B) return;                                        // (the only bound on a write to index)
  const int64_t raw = a.step[0];
  const uint64_t s = raw < 0 ? 0u : (uint64_t)raw;
  const uint64_t epoch = s / a.ticks, i_batch = s % a.ticks;   // i_batch < ticks, so q below is < ticks B world <= N
  const uint32_t e_lo = (uint32_t)epoch, e_hi = (uint32_t)(epoch >> 32);
  uint32_t x = ((uint32_t)i_batch * (uint32_t)a.world + (uint32_t)a.rank) * (uint32_t)a.B + (uint32_t)b;
  do {                                                         // cycle walking: the orbit of x < N returns below N
    x = feistel_pass(x, a, e_lo, e_hi);
  } while (x >= a.N);
  a.index[b] = (int32_t)x;
  if (b != 0) return;
  a.lr[0] = (float)lr_of(a, s);
  if (a.iht_mode) {
    int mode = 0;
    if (a.sparsify) {
      const uint64_t e3 = 3u * (epoch < (uint64_t)a.num_epochs ? epoch : (uint64_t)a.num_epochs);     // (no overflow)
      if (e3 >= (uint64_t)a.num_epochs)
        mode = (e3 < 2u * (uint64_t)a.num_epochs && i_batch % (uint64_t)a.trim_level == 0) ? 1 : 2;
    }
    a.iht_mode[0] = mode;
  }
  a.where[0] = (int64_t)epoch;
  a.where[1] = (int64_t)i_batch;
  a.where[2] = (int64_t)(s < a.log_len - 1 ? s : a.log_len - 1);
  a.where[3] = 0;
}

}  // namespace

int train_schedule_run(const fastgrnn_schedule_desc& d, const int64_t* step, int32_t* index, float* lr,
                       int32_t* iht_mode, int64_t* where, hipStream_t s) {
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
  uint32_t k = 2;
  while (k < 32 && (1u << k) < a.N) k += 2;                    // the smallest even k >= 2 with 2^k >= N (N < 2^31)
  a.half = k / 2;
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
  hipLaunchKernelGGL(sched_k, dim3((d.B + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, s, a);
  return launch_status();
}

}  // namespace fastgrnn
