// Augmentation on the device, inside the featuriser (include/fastgrnn_hip.h: fastgrnn_hip_mfcc_augment,
// fastgrnn_hip_augment_draw).  gfx950 only.
//   mfcc_aug_k   the featuriser of kernels_mfcc.hip -- the same body, mfcc_body.h -- whose stage a reads a clip of an
//                audio bank through a record: a time shift, a gain and a noise of a noise bank, wrapped to the clip's
//                length, at a gain of its own.  The augmented clip goes from the registers of the two gathers into LDS
//                and is never written to memory.  Stages b-e, LDS and the rules of DESIGN.md 4.0 are mfcc_k's.
//   aug_draw_k   the records of a batch from Philox4x32-10 on (seed, step, clip): one thread per clip, two blocks each.
#include "mfcc_body.h"
#include "philox.h"

namespace fastgrnn {
namespace {

template <typename AT>
__global__ __launch_bounds__(MF_THREADS) void mfcc_aug_k(mfcc_aug_args a) {
  mfcc_body<AT, true>(a);
}

// ---- the draw ----------------------------------------------------------------------------------------------------------
// (Philox4x32-10 itself: philox.h, shared with kernels_schedule.hip)
__device__ __forceinline__ float unit_of(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }     // exact
__device__ __forceinline__ int below(uint32_t x, uint32_t n) { return (int)__umulhi(x, n); }
__device__ __forceinline__ float between(float lo, float hi, float u) {
  return add_rn(lo, mul_rn(add_rn(hi, -lo), u));
}

struct draw_args {
  const int64_t* step;
  const int32_t* index;
  const int32_t* noise_lengths;
  fastgrnn_mfcc_aug* aug;
  fastgrnn_augment_ranges r;
  uint32_t seed_lo, seed_hi;
  int B, n_noise, noise_len_max;
};

__global__ __launch_bounds__(256) void aug_draw_k(draw_args a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const uint64_t step = (uint64_t)a.step[0];
  const uint32_t s_lo = (uint32_t)step, s_hi = (uint32_t)(step >> 32);
  const u32x4 p = philox4x32_10(u32x4{(uint32_t)b, s_lo, s_hi, 0u}, a.seed_lo, a.seed_hi);
  const u32x4 q = philox4x32_10(u32x4{(uint32_t)b, s_lo, s_hi, 1u}, a.seed_lo, a.seed_hi);
  fastgrnn_mfcc_aug o;
  o.src = a.index[b];
  o.shift = 0;
  o.noise = -1;
  o.noise_off = 0;
  o.gain = 1.0f;
  o.noise_gain = 0.0f;
  if (unit_of(p.x) < a.r.p_augment) {
    o.shift = below(p.y, 2u * (uint32_t)a.r.max_shift + 1u) - a.r.max_shift;
    o.gain = between(a.r.gain_lo, a.r.gain_hi, unit_of(p.z));
    if (a.n_noise > 0 && unit_of(p.w) < a.r.p_noise) {
      o.noise = below(q.x, (uint32_t)a.n_noise);
      const int nlen = min(max(a.noise_lengths[o.noise], 1), a.noise_len_max);
      o.noise_off = below(q.y, (uint32_t)nlen);
      o.noise_gain = between(a.r.noise_gain_lo, a.r.noise_gain_hi, unit_of(q.z));
    }
  }
  a.aug[b] = o;
}

}  // namespace

int mfcc_augment_run(const fastgrnn_mfcc_desc& d, const fastgrnn_mfcc_bank& bank, const void* audio, const int32_t* lengths,
                     const void* noise, const int32_t* noise_lengths, const fastgrnn_mfcc_aug* aug, const void* tables,
                     const float* mean, const float* stdv, void* feats, hipStream_t s) {
  mfcc_aug_args a;
  a.audio = audio;
  a.lengths = lengths;
  a.tab = reinterpret_cast<const float*>(tables);
  a.mean = mean;
  a.stdv = stdv;
  a.feats = reinterpret_cast<float*>(feats);
  a.clip_stride = d.clip_stride;
  a.L = d.L;
  a.n_mfcc = d.n_mfcc;
  a.order = d.order;
  a.width = d.width;
  a.max_len = d.max_len;
  a.peak = (d.flags & FASTGRNN_MFCC_PEAK_NORMALIZE) ? 1 : 0;
  a.top_db = d.top_db;
  a.aug = aug;
  a.noise = noise;
  a.noise_lengths = noise_lengths;
  a.noise_stride = bank.noise_stride;
  a.n_clips = bank.n_clips;
  a.n_noise = bank.n_noise;
  a.noise_len_max = bank.noise_len_max;
  if (d.audio_dtype == FASTGRNN_MFCC_AUDIO_I16)
    hipLaunchKernelGGL(mfcc_aug_k<short>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(mfcc_aug_k<float>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  return launch_status();
}

int augment_draw_run(int B, uint64_t seed, const int64_t* step, const int32_t* index, const fastgrnn_augment_ranges& r,
                     int n_noise, int noise_len_max, const int32_t* noise_lengths, fastgrnn_mfcc_aug* aug, hipStream_t s) {
  draw_args a;
  a.step = step;
  a.index = index;
  a.noise_lengths = noise_lengths;
  a.aug = aug;
  a.r = r;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.B = B;
  a.n_noise = n_noise;
  a.noise_len_max = noise_len_max;
  hipLaunchKernelGGL(aug_draw_k, dim3((B + 255) / 256), dim3(256), 0, s, a);
  return launch_status();
}

}  // namespace fastgrnn
