// The rolling mode of the trainer (the reference's --rolling, trainClassifier.py:174-221, model.py:135-156) as functions
// of the step count (include/fastgrnn_hip.h: fastgrnn_hip_train_schedule_rolling, fastgrnn_hip_rolling_exchange).
// gfx950 only.
//   roll_sched_k     sched_k with the rolling position: short epochs of 2, 3, .. iterations in front of the full ones;
//                    thread 0 of block 0 also writes where[3] = fresh | zero << 1.
//   roll_exchange_k  one wave per batch row j, all layers: the row's image under the iteration's bag shuffle pi_s and
//                    its preimage are computed once (a few Philox calls), then per layer state[j] goes to bag[pi_s(j)]
//                    and h0[j] comes from state[pi_s^-1(j)] where that is a batch row, else from the old bag[j] (which no
//                    wave writes in that case: nothing in the launch is ordered against anything else).  On a fresh
//                    iteration h0 is zeroed instead, and where the bags start over all their rows are cleared grid-stride.
// No LDS, no atomics, plain vector loads and stores; everything is a function of (descriptors, step[0], state, bag).
#include "common.h"
#include "philox.h"
#include "schedule_common.h"

namespace fastgrnn {
namespace {

constexpr int ROLL_THREADS = 256;
constexpr int ROLL_WAVES = ROLL_THREADS / 64;
constexpr int ROLL_MAX_BLOCKS = 1024;
constexpr uint32_t BAG_TAG = 0xC0000000u;

struct roll_pos_args {
  uint64_t ticks_full, n_short, short_total;     // short_total = n_short (n_short + 3) / 2
};

struct roll_pos {
  uint64_t epoch, i_batch;
  bool fresh, zero;
};

// the 0-based iteration s -> its epoch and batch; epoch e < n_short starts at e (e + 3) / 2 and has e + 2 iterations
__device__ __forceinline__ roll_pos roll_position(const roll_pos_args& p, uint64_t s) {
  roll_pos r;
  if (s < p.short_total) {
    uint64_t lo = 0, hi = p.n_short - 1;         // the largest e with e (e + 3) / 2 <= s (n_short < 2^31: no overflow)
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) >> 1;
      if (mid * (mid + 3) / 2 <= s) lo = mid; else hi = mid - 1;
    }
    r.epoch = lo;
    r.i_batch = s - lo * (lo + 3) / 2;
  } else {
    const uint64_t t = s - p.short_total;
    r.epoch = p.n_short + t / p.ticks_full;
    r.i_batch = t % p.ticks_full;
  }
  r.zero = r.i_batch == 0 && r.epoch < p.n_short;
  r.fresh = r.i_batch == 0 && r.epoch <= p.n_short;
  return r;
}

struct roll_sched_args {
  sched_args a;
  roll_pos_args p;
};

__global__ __launch_bounds__(ROLL_THREADS) void roll_sched_k(roll_sched_args ra) {
  const sched_args& a = ra.a;
  const int b = blockIdx.x * ROLL_THREADS + threadIdx.x;
  if (b >= a.B) return;                                        // (the only bound on a write to index)
  const int64_t raw = a.step[0];
  const uint64_t s = raw < 0 ? 0u : (uint64_t)raw;
  const roll_pos pos = roll_position(ra.p, s);                 // i_batch < ticks_full, so q below is < N
  const uint32_t e_lo = (uint32_t)pos.epoch, e_hi = (uint32_t)(pos.epoch >> 32);
  uint32_t x = ((uint32_t)pos.i_batch * (uint32_t)a.world + (uint32_t)a.rank) * (uint32_t)a.B + (uint32_t)b;
  do {                                                         // cycle walking: the orbit of x < N returns below N
    x = feistel_pass(x, a.half, a.mask, e_lo, e_hi, 0x80000000u, a.seed_lo, a.seed_hi);
  } while (x >= a.N);
  a.index[b] = (int32_t)x;
  if (b != 0) return;
  a.lr[0] = (float)lr_of(a, s);
  if (a.iht_mode) a.iht_mode[0] = iht_phase_of(a, pos.epoch, pos.i_batch);
  a.where[0] = (int64_t)pos.epoch;
  a.where[1] = (int64_t)pos.i_batch;
  a.where[2] = (int64_t)(s < a.log_len - 1 ? s : a.log_len - 1);
  a.where[3] = (int64_t)((pos.fresh ? 1 : 0) | (pos.zero ? 2 : 0));
}

struct roll_xchg_args {
  const int64_t* step;
  const float* state[3];
  float* bag[3];
  float* h0[3];
  roll_pos_args p;
  uint32_t seed_lo, seed_hi;
  uint32_t B, M, half, mask;                     // M = B bag_count rows per bag, 2^(2 half) >= M
  int layers, vec;                               // vec bit l: layer l moves 16 bytes per lane
  int H[3];
};

// one row of n floats, by the lanes of a wave; src == nullptr writes +0.0.  Moved as integers: the bits are kept.
template <typename V>
__device__ __forceinline__ void roll_row(V* dst, const V* src, uint32_t n, uint32_t lane) {
  for (uint32_t i = lane; i < n; i += 64) dst[i] = src ? src[i] : V{};
}

__device__ __forceinline__ void roll_move(float* dst, const float* src, int H, bool vec, uint32_t lane) {
  if (vec) roll_row(reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(src), (uint32_t)H / 4, lane);
  else roll_row(reinterpret_cast<uint32_t*>(dst), reinterpret_cast<const uint32_t*>(src), (uint32_t)H, lane);
}

__global__ __launch_bounds__(ROLL_THREADS) void roll_exchange_k(roll_xchg_args a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * ROLL_WAVES + (threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * ROLL_WAVES;
  const int64_t raw = a.step[0];
  const uint64_t s = raw < 0 ? 0u : (uint64_t)raw;
  const roll_pos pos = roll_position(a.p, s);
  if (pos.zero) {                                              // every row of every bag, flat over the launch
    const size_t tid = (size_t)blockIdx.x * ROLL_THREADS + threadIdx.x, all = (size_t)gridDim.x * ROLL_THREADS;
#pragma unroll
    for (int l = 0; l < 3; ++l) {                              // (fixed trips: the by-value arrays stay in registers)
      if (l >= a.layers) break;
      const size_t n = (size_t)a.M * (size_t)a.H[l];           // (< 2^31 rows of < 2^31 floats: fits)
      if (a.vec >> l & 1) {
        uint4* dst = reinterpret_cast<uint4*>(a.bag[l]);
        for (size_t i = tid; i < n / 4; i += all) dst[i] = uint4{};
      } else {
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.bag[l]);
        for (size_t i = tid; i < n; i += all) dst[i] = 0u;
      }
    }
  }
  const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
  for (uint32_t j = wave; j < a.B; j += waves) {               // (j < B: the only bound on the rows of state and h0)
    if (pos.fresh) {
#pragma unroll
      for (int l = 0; l < 3; ++l)
        if (l < a.layers) roll_move(a.h0[l] + (size_t)j * a.H[l], nullptr, a.H[l], a.vec >> l & 1, lane);
      continue;
    }
    uint32_t to = j, from = j;                                 // pi_s(j) and pi_s^-1(j); both walks end below M
    do {
      to = feistel_pass(to, a.half, a.mask, s_lo, s_hi, BAG_TAG, a.seed_lo, a.seed_hi);
    } while (to >= a.M);
    do {
      from = feistel_unpass(from, a.half, a.mask, s_lo, s_hi, BAG_TAG, a.seed_lo, a.seed_hi);
    } while (from >= a.M);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      if (l >= a.layers) break;
      const int H = a.H[l];
      const bool vec = a.vec >> l & 1;
      const float* mine = a.state[l] + (size_t)j * H;
      roll_move(a.bag[l] + (size_t)to * H, mine, H, vec, lane);
      // (from >= B: no batch row lands on bag row j, so nobody writes what is read here)
      const float* src = from < a.B ? a.state[l] + (size_t)from * H : a.bag[l] + (size_t)j * H;
      roll_move(a.h0[l] + (size_t)j * H, src, H, vec, lane);
    }
  }
}

roll_pos_args roll_pos_of(const fastgrnn_schedule_desc& d, const fastgrnn_rolling_desc& r) {
  roll_pos_args p;
  const int64_t ticks = d.N / (d.B * d.world);
  int64_t max_roll = ticks;
  if ((int64_t)r.max_rolling_length + 2 < max_roll) max_roll = (int64_t)r.max_rolling_length + 2;
  if ((int64_t)d.num_epochs + 2 < max_roll) max_roll = (int64_t)d.num_epochs + 2;
  const int64_t n_short = max_roll > 2 ? max_roll - 2 : 0;
  p.ticks_full = (uint64_t)ticks;
  p.n_short = (uint64_t)n_short;
  p.short_total = (uint64_t)(n_short * (n_short + 3) / 2);
  return p;
}

}  // namespace

int train_schedule_rolling_run(const fastgrnn_schedule_desc& d, const fastgrnn_rolling_desc& r, const int64_t* step,
                               int32_t* index, float* lr, int32_t* iht_mode, int64_t* where, hipStream_t s) {
  roll_sched_args a;
  a.a = sched_args_of(d, step, index, lr, iht_mode, where);
  a.p = roll_pos_of(d, r);
  hipLaunchKernelGGL(roll_sched_k, dim3((d.B + ROLL_THREADS - 1) / ROLL_THREADS), dim3(ROLL_THREADS), 0, s, a);
  return launch_status();
}

int rolling_exchange_run(const fastgrnn_schedule_desc& d, const fastgrnn_rolling_desc& r, const int64_t* step,
                         const float* const state[3], float* const bag[3], float* const h0[3], hipStream_t s) {
  roll_xchg_args a;
  a.step = step;
  a.p = roll_pos_of(d, r);
  a.seed_lo = (uint32_t)d.seed;
  a.seed_hi = (uint32_t)(d.seed >> 32);
  a.B = (uint32_t)d.B;
  a.M = (uint32_t)((int64_t)d.B * r.bag_count);
  a.half = feistel_half(a.M);
  a.mask = (1u << a.half) - 1u;
  a.layers = r.layers;
  a.vec = 0;
  for (int l = 0; l < 3; ++l) {
    const bool on = l < r.layers;
    a.state[l] = on ? state[l] : nullptr;
    a.bag[l] = on ? bag[l] : nullptr;
    a.h0[l] = on ? h0[l] : nullptr;
    a.H[l] = on ? r.H[l] : 0;
    if (on && r.H[l] % 4 == 0 && (((uintptr_t)state[l] | (uintptr_t)bag[l] | (uintptr_t)h0[l]) & 15u) == 0)
      a.vec |= 1 << l;
  }
  // the geometry is a function of the descriptors alone (a captured launch serves every step): a wave per batch row
  // would do for the exchange; clearing the bags grid-strides over up to ROLL_MAX_BLOCKS blocks' worth of bag rows
  const int64_t want = ((int64_t)a.M + ROLL_WAVES - 1) / ROLL_WAVES;
  const int blocks = (int)(want < ROLL_MAX_BLOCKS ? want : ROLL_MAX_BLOCKS);
  hipLaunchKernelGGL(roll_exchange_k, dim3(blocks), dim3(ROLL_THREADS), 0, s, a);
  return launch_status();
}

}  // namespace fastgrnn
