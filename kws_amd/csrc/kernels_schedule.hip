// What a trainer iteration needs from outside the model, as a function of the step count (include/fastgrnn_hip.h:
// fastgrnn_hip_train_schedule).  gfx950 only.
//   sched_k   one thread per clip of the batch: position q of the epoch's order -> clip number through a keyed
//             permutation of 0..N-1 (a four-round Feistel network on Philox4x32-10, cycle-walked into the range); thread 0
//             of block 0 also writes the learning rate (double, rounded once), the IHT phase and the position.
// No LDS, no atomics, plain stores; everything is a function of (descriptor, step[0]) alone.
#include "common.h"
#include "philox.h"
#include "schedule_common.h"

namespace fastgrnn {
namespace {

constexpr int SCHED_THREADS = 256;

__global__ __launch_bounds__(SCHED_THREADS) void sched_k(sched_args a) {
  const int b = blockIdx.x * SCHED_THREADS + threadIdx.x;
  if (b >= a.B) return;                                        // (the only bound on a write to index)
  const int64_t raw = a.step[0];
  const uint64_t s = raw < 0 ? 0u : (uint64_t)raw;
  const uint64_t epoch = s / a.ticks, i_batch = s % a.ticks;   // i_batch < ticks, so q below is < ticks B world <= N
  const uint32_t e_lo = (uint32_t)epoch, e_hi = (uint32_t)(epoch >> 32);
  uint32_t x = ((uint32_t)i_batch * (uint32_t)a.world + (uint32_t)a.rank) * (uint32_t)a.B + (uint32_t)b;
  do {                                                         // cycle walking: the orbit of x < N returns below N
    x = feistel_pass(x, a.half, a.mask, e_lo, e_hi, 0x80000000u, a.seed_lo, a.seed_hi);
  } while (x >= a.N);
  a.index[b] = (int32_t)x;
  if (b != 0) return;
  a.lr[0] = (float)lr_of(a, s);
  if (a.iht_mode) a.iht_mode[0] = iht_phase_of(a, epoch, i_batch);
  a.where[0] = (int64_t)epoch;
  a.where[1] = (int64_t)i_batch;
  a.where[2] = (int64_t)(s < a.log_len - 1 ? s : a.log_len - 1);
  a.where[3] = 0;
}

}  // namespace

int train_schedule_run(const fastgrnn_schedule_desc& d, const int64_t* step, int32_t* index, float* lr,
                       int32_t* iht_mode, int64_t* where, hipStream_t s) {
  const sched_args a = sched_args_of(d, step, index, lr, iht_mode, where);
  hipLaunchKernelGGL(sched_k, dim3((d.B + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, s, a);
  return launch_status();
}

}  // namespace fastgrnn
