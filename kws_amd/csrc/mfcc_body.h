// The body of the featuriser kernels, shared by kernels_mfcc.hip (mfcc_k: a clip per workgroup, read as it lies) and
// kernels_augment.hip (mfcc_aug_k: a clip of an audio bank read through an augmentation record).  One template with a
// compile-time AUG switch around stage a; stages b-e are the same code for both.  The semantics are spelled out in
// include/fastgrnn_hip.h (fastgrnn_hip_mfcc, fastgrnn_hip_mfcc_augment); the stages and the rules they keep are
// described at the top of kernels_mfcc.hip.  Stages b-e are functions of their own: kernels_mfcc_stream.hip (a
// recording's frames computed once for its overlapping clips) runs them on other row tiles around a stage a of its own.
#pragma once
#include "common.h"

namespace fastgrnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MF_THREADS = 1024;
constexpr int MF_NFFT = 400, MF_HOP = 160, MF_PAD = 200;
constexpr int MF_BINS = 201, MF_BINP = 208;       // rfft bins, padded to 13 column tiles (basis columns >= 201 are zero)
constexpr int MF_MELS = 128, MF_CMAX = 64;
constexpr int MF_ROWS = 112, MF_FRAMES = 101;     // 7 row tiles; frames of a 16 000-sample clip
// Padded sample i lives at s_aud[i + 4 (i / 160)]: four unused words per hop make a frame row 164 words, so the 16 rows
// x 4 samples of an A-operand read fall into 64 different banks (at 160 they shared four: 2.5 ms -> see DESIGN 4.10).
// Sample j of frame r is at 164 r + j + 4 (j / 160), and j / 160 is uniform over a k-step (160 is a multiple of 4).
constexpr int MF_SKEW = 4, MF_RS = MF_HOP + MF_SKEW;
constexpr int MF_PADDED = 16400;                  // 200 + 16 000 + 200
constexpr int MF_AUD = MF_PADDED + MF_SKEW * 104; // 16 816 words; the dB image [112][129] fits in it too
constexpr int MF_PS = 209, MF_DS = 129, MF_CS = 65;   // LDS row strides of the power, dB and coefficient images
constexpr int MF_MINLEN = 1280;                   // nine frames: what the API asks of every clip

// table image (floats): cos basis [400][208], sin basis [400][208], mel weights [208][128], DCT [128][64],
// taps [7 widths][2 orders][16]
constexpr size_t TB_COS = 0, TB_SIN = TB_COS + (size_t)MF_NFFT * MF_BINP, TB_MEL = TB_SIN + (size_t)MF_NFFT * MF_BINP,
                 TB_DCT = TB_MEL + (size_t)MF_BINP * MF_MELS, TB_TAP = TB_DCT + (size_t)MF_MELS * MF_CMAX,
                 TB_END = TB_TAP + 7 * 2 * 16;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

struct mfcc_args {
  const void* audio;
  const int32_t* lengths;
  const float* tab;
  const float* mean;
  const float* stdv;
  float* feats;
  long long clip_stride;
  int L, n_mfcc, order, width, max_len, peak;
  float top_db;
};

// ... and what the augmented kernels read on top (fastgrnn_hip_mfcc_augment): audio is a bank of n_clips clips, lengths
// is indexed by the record's src, the noise bank has the audio's dtype
struct mfcc_aug_args : mfcc_args {
  const fastgrnn_mfcc_aug* aug;
  const void* noise;
  const int32_t* noise_lengths;
  long long noise_stride;
  int n_clips, n_noise, noise_len_max;
};

__device__ __forceinline__ float sample_of(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float sample_of(const short* p, long long i) { return (float)p[i] * (1.0f / 32768.0f); }

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

// One fp32 operation, rounded to nearest, that the compiler may not fuse with a neighbour: the augmentation's samples
// and the draw's gains are defined operation by operation (numpy and torch reproduce them bit for bit).  HIP's
// __fmul_rn / __fadd_rn are plain `*` / `+` under the translation unit's -ffp-contract=fast and did contract.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

constexpr int MF_AUG_SHIFT_CAP = 1 << 20;        // |shift| >= 16 000 already empties a clip: the cap changes no sample

// ---- stages b-e, shared by mfcc_body and the streamed kernels (kernels_mfcc_stream.hip).  Every output row of the
// three products is a k-ordered chain of its own: which row tile, wave or workgroup computes a row does not change it.

// b. power spectrum: [16 NRT rows] x [16 bins of this wave], cos and sin tiles side by side.  arow[rt]: the LDS word of
// sample lk of the frame in row 16 rt + lr of the skewed audio image; the power goes to s_pow[16 rt + ..][MF_PS].
template <int NRT>
__device__ __forceinline__ void mfcc_power(const float* s_aud, float* s_pow, const float* tab, const int (&arow)[NRT],
                                           int wave, int lr, int lk) {
  f32x4 ac[NRT], as[NRT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
    ac[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    as[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float* bc = tab + TB_COS + (size_t)lk * MF_BINP + 16 * wave + lr;
  const float* bs = tab + TB_SIN + (size_t)lk * MF_BINP + 16 * wave + lr;
  for (int k0 = 0; k0 < MF_NFFT; k0 += 16) {
    const int ks = k0 + (k0 >= MF_HOP ? MF_SKEW : 0) + (k0 >= 2 * MF_HOP ? MF_SKEW : 0);   // (a batch never straddles a hop)
    float fa[4][NRT], fc[4], fs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fc[u] = bc[(size_t)(k0 + 4 * u) * MF_BINP];
      fs[u] = bs[(size_t)(k0 + 4 * u) * MF_BINP];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) fa[u][rt] = s_aud[arow[rt] + ks + 4 * u];
    }
    __builtin_amdgcn_sched_barrier(0);          // every operand request of the batch in front of its first MFMA
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        ac[rt] = mfma4(fa[u][rt], fc[u], ac[rt]);
        as[rt] = mfma4(fa[u][rt], fs[u], as[rt]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    completion_read(as[NRT - 1][0]);            // the youngest accumulator: the batch's registers are free again
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      s_pow[(16 * rt + 4 * lk + e) * MF_PS + 16 * wave + lr] = fmaf(ac[rt][e], ac[rt][e], as[rt][e] * as[rt][e]);
  }
}

// c. mel projection of NT row tiles against mel columns 16 ct..: prow[i] is the LDS word of bin lk of row lr of tile i
template <int NT>
__device__ __forceinline__ void mfcc_mel(const float* s_pow, const float* tab, const int (&prow)[NT], int ct, int lr, int lk,
                                         f32x4 (&acc)[NT]) {
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* bw = tab + TB_MEL + (size_t)lk * MF_MELS + 16 * ct + lr;
  for (int k0 = 0; k0 < MF_BINP; k0 += 16) {
    float fa[4][NT], fb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fb[u] = bw[(size_t)(k0 + 4 * u) * MF_MELS];
#pragma unroll
      for (int i = 0; i < NT; ++i) fa[u][i] = s_pow[prow[i] + k0 + 4 * u];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < NT; ++i) acc[i] = mfma4(fa[u][i], fb[u], acc[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
    completion_read(acc[NT - 1][0]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ __forceinline__ float mfcc_db(float mel) { return 10.0f * log10f(fmaxf(1e-10f, mel)); }

// d. DCT-II of the dB image [112][MF_DS] into the coefficient image [112][MF_CS], the top_db clip applied to the A
// operands on the way in: wave w owns coefficient columns 16 (w & 3).. and row tiles w >> 2, (w >> 2) + 4
__device__ __forceinline__ void mfcc_dct(const float* s_db, float* s_coef, const float* tab, float floor_db, int wave,
                                         int lr, int lk) {
  const int ct = wave & 3, r0 = wave >> 2;
  f32x4 acc[2];
  int drow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    drow[i] = (16 * min(r0 + 4 * i, 6) + lr) * MF_DS + lk;
  }
  const float* bd = tab + TB_DCT + (size_t)lk * MF_CMAX + 16 * ct + lr;
  for (int k0 = 0; k0 < MF_MELS; k0 += 16) {
    float fa[4][2], fb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fb[u] = bd[(size_t)(k0 + 4 * u) * MF_CMAX];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[u][i] = fmaxf(s_db[drow[i] + k0 + 4 * u], floor_db);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] = mfma4(fa[u][i], fb[u], acc[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
    completion_read(acc[1][0]);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rt = r0 + 4 * i;
    if (rt < 7) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s_coef[(16 * rt + 4 * lk + e) * MF_CS + 16 * ct + lr] = acc[i][e];
    }
  }
}

// e. deltas, pad / cut, normalisation, stores: element i of a clip's [max_len][F] block `out`, from its n frames of
// coefficients
__device__ __forceinline__ void mfcc_rows(const float* s_coef, const float* s_tap, int n, int C, int order, int width,
                                          int max_len, const float* mean, const float* stdv, float* out, int tid) {
  const int F = C * (order + 1), total = max_len * F, h = width >> 1;
  const int last = max(n - 1 - h, h);             // (n >= width for every length the caller may pass; in bounds for any)
  const bool norm = mean != nullptr;
  for (int i = tid; i < total; i += MF_THREADS) {
    const int t = i / F, f = i - t * F, o = f / C, c = f - o * C;
    const int tt = min(t, n - 1);
    const int tc = min(max(tt, h), last) - h;     // first row under the FIR; the interp edges are constant (deriv == polyorder)
    float val = s_coef[tt * MF_CS + c], d = 0.f;
    const float* tap = s_tap + (o == 2 ? 16 : 0);
    for (int k = 0; k < width; ++k) d = fmaf(tap[k], s_coef[(tc + k) * MF_CS + c], d);
    val = o == 0 ? val : d;
    val = t < n ? val : 0.f;
    if (norm) val = (val - mean[f]) / stdv[f];
    out[i] = val;
  }
}

template <typename AT, bool AUG, typename ARGS>
__device__ __forceinline__ void mfcc_body(const ARGS& a) {
  __shared__ float s_aud[MF_AUD];               // a-b: padded clip;   c-d: dB image [112][129]
  __shared__ float s_pow[MF_ROWS * MF_PS];      // b-c: power [112][209];   d-e: coefficients [112][65]
  __shared__ float s_red[16];
  __shared__ float s_tap[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;     // MFMA operand maps: A[row lr][k lk], B[k lk][col lr]; C/D[row 4 lk + reg][col lr]
  unsigned clip = blockIdx.x;
  if constexpr (AUG) clip = (unsigned)min(max(a.aug[blockIdx.x].src, 0), a.n_clips - 1);     // (whatever the record says)
  const AT* src = reinterpret_cast<const AT*>(a.audio) + (long long)clip * a.clip_stride;
  int len = a.L;
  if (a.lengths) len = min(max(a.lengths[clip], MF_MINLEN), a.L);   // (whatever the caller wrote: reads stay inside the row)
  const int n = 1 + len / MF_HOP;
  if (tid < 32) s_tap[tid] = a.tab[TB_TAP + ((a.width - 3) >> 1) * 32 + tid];

  // ---- a. the padded clip: every load is issued (clamped into the clip), what lies outside becomes zero
  {
    float v[17];
    if constexpr (!AUG) {
#pragma unroll
      for (int j = 0; j < 17; ++j) {
        const int s = tid + j * MF_THREADS - MF_PAD;
        v[j] = sample_of(src, (long long)min(max(s, 0), len - 1));
      }
    } else {
      // y'[i] = gain y[i - shift] + noise_gain nz[(noise_off + i) mod nlen]: two clamped gathers per sample, all 34
      // issued before the first is used.  Everything the record decides is uniform over the workgroup.
      const fastgrnn_mfcc_aug r = a.aug[blockIdx.x];
      const int shift = min(max(r.shift, -MF_AUG_SHIFT_CAP), MF_AUG_SHIFT_CAP);
      const bool has = r.noise >= 0 && a.n_noise > 0;
      float z[17];
#pragma unroll
      for (int j = 0; j < 17; ++j) {
        const int q = tid + j * MF_THREADS - MF_PAD - shift;
        v[j] = sample_of(src, (long long)min(max(q, 0), len - 1));
        z[j] = 0.f;
      }
      lds_writes_landed();                        // (the taps: no LDS write is pending at the branch around the gather)
      if (has) {                                  // (uniform) an absent noise is not read at all: no 0 * NaN
        const int row = min(r.noise, a.n_noise - 1);
        const int nlen = min(max(a.noise_lengths[row], 1), a.noise_len_max);
        const AT* nz = reinterpret_cast<const AT*>(a.noise) + (long long)row * a.noise_stride;
        int off = r.noise_off % nlen;             // sample i >= 0 reads (off + i) mod nlen; thread-sample s = i - 200
        off = off < 0 ? off + nlen : off;
        int base = (off - MF_PAD) % nlen;
        base = base < 0 ? base + nlen : base;
        const int step = MF_THREADS % nlen;
        int k = (int)(((unsigned)base + (unsigned)tid) % (unsigned)nlen);
#pragma unroll
        for (int j = 0; j < 17; ++j) {
          z[j] = sample_of(nz, (long long)k);     // (0 <= k < nlen for every thread, also where s lies outside the clip)
          k += step;
          k = k >= nlen ? k - nlen : k;
        }
      }
#pragma unroll
      for (int j = 0; j < 17; ++j) {
        const int q = tid + j * MF_THREADS - MF_PAD - shift;
        const float y = (q >= 0 && q < len) ? v[j] : 0.f;
        const float g = mul_rn(r.gain, y);
        v[j] = has ? add_rn(g, mul_rn(r.noise_gain, z[j])) : g;
      }
    }
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 17; ++j) {
      const int s = tid + j * MF_THREADS - MF_PAD;
      v[j] = (s >= 0 && s < len) ? v[j] : 0.f;
      m = fmaxf(m, fabsf(v[j]));
    }
    if (a.peak) {                                 // (uniform over the workgroup) inferencetry.py:172-175, in fp32
      m = wave_max(m);
      if (lane == 0) s_red[wave] = m;
      __syncthreads();
      m = s_red[0];
#pragma unroll
      for (int w = 1; w < 16; ++w) m = fmaxf(m, s_red[w]);
      if (m > 0.f) {
#pragma unroll
        for (int j = 0; j < 17; ++j) v[j] = v[j] / m;
      }
    }
#pragma unroll
    for (int j = 0; j < 17; ++j) {
      const int i = tid + j * MF_THREADS;
      if (i < MF_PADDED) s_aud[i + MF_SKEW * (i / MF_HOP)] = v[j];    // (only the 17th round is ragged; no loop here)
    }
  }
  __syncthreads();

  // ---- b. power spectrum: [112 frames] x [16 bins of this wave], cos and sin tiles side by side
  if (wave < 13) {                                // (wave-uniform, around the whole loop)
    int arow[7];
#pragma unroll
    for (int rt = 0; rt < 7; ++rt)
      arow[rt] = min(16 * rt + lr, MF_FRAMES - 1) * MF_RS + lk;    // (rows 101..111 repeat frame 100; nothing reads them back)
    mfcc_power<7>(s_aud, s_pow, a.tab, arow, wave, lr, lk);
  }
  __syncthreads();

  // ---- c. mel projection and dB: wave w owns mel columns 16 (w & 7).. and the row tiles of parity w >> 3
  float mx = -INFINITY;
  {
    const int ct = wave & 7, r0 = wave >> 3;
    f32x4 acc[4];
    int prow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      prow[i] = (16 * min(r0 + 2 * i, 6) + lr) * MF_PS + lk;      // (a fourth tile of the odd waves repeats tile 6, unstored)
    mfcc_mel<4>(s_pow, a.tab, prow, ct, lr, lk, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rt = r0 + 2 * i;
      if (rt < 7) {                               // (wave-uniform)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * rt + 4 * lk + e;
          const float db = mfcc_db(acc[i][e]);
          s_aud[row * MF_DS + 16 * ct + lr] = db;
          mx = row < n ? fmaxf(mx, db) : mx;
        }
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = s_red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = fmaxf(mx, s_red[w]);
  const float floor_db = a.top_db >= 0.f ? mx - a.top_db : -INFINITY;

  // ---- d. DCT-II: the dB image in s_aud -> the coefficients in s_pow
  mfcc_dct(s_aud, s_pow, a.tab, floor_db, wave, lr, lk);
  __syncthreads();

  // ---- e. deltas, pad / cut, normalisation, stores
  const int total = a.max_len * a.n_mfcc * (a.order + 1);
  mfcc_rows(s_pow, s_tap, n, a.n_mfcc, a.order, a.width, a.max_len, a.mean, a.stdv,
            a.feats + (size_t)blockIdx.x * (size_t)total, tid);
}

}  // namespace
}  // namespace fastgrnn
