// The reference's featuriser on the device: librosa.feature.mfcc + librosa.feature.delta at librosa 0.10.2's defaults
// (data_pipeline/mfccProcessor.py:43-58), padded or cut to max_len frames and normalised (preprocessing.py:79-88,
// inferencetry.py:165-200).  gfx950 only.  The semantics are spelled out in include/fastgrnn_hip.h (fastgrnn_hip_mfcc).
// One workgroup of 16 waves owns a clip and everything between the samples and the feature rows stays on its CU:
//   a. the clip, centre-padded with 200 zeros on each side and zero-filled past its length, goes to LDS (16 400 fp32,
//      skewed by four words per hop against bank conflicts);
//      peak normalisation is a workgroup maximum over the registers that carry it there.
//   b. DFT as a matrix product on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32: one rounding per product,
//      a k-ordered fmaf chain).  Frame r, sample j is padded sample 160 r + j: the A operands are read from the overlapping
//      frames in place, no frame matrix exists.  Wave w < 13 owns bins 16w..16w+15 -- the cos and the sin column tile of
//      the window-folded basis -- and runs all 7 row tiles (n <= 101 frames) against them, so the 665 KB basis is read
//      from L2 once per clip.  |X|^2 goes to LDS beside the audio ([112][209] fp32; 67.3 + 93.6 KB of the CU's 160).
//   c. mel = power . W (208 x 128, fp32 MFMA again), 10 log10(max(1e-10, .)) with the accurate log10f, into the LDS the
//      audio occupied; the clip-wide maximum over the valid frames by shuffles and one LDS exchange (no atomics).
//   d. DCT-II as a third product, the top_db clip applied to its A operands on the way in; the coefficients land in
//      the LDS the power spectrum occupied.
//   e. the Savitzky-Golay FIRs along time with their constant edges, pad / cut to max_len, normalisation, row stores.
// Clips shorter than L take no path of their own: frames past n are computed on zeros and masked out of the maximum,
// the delta edges and the output.  DESIGN.md 4.0: every MFMA loop loads a batch of operands into registers of its own,
// issues its MFMAs and ends in a completion read before the next batch is requested (operand rule); no loop contains
// an LDS write, and none has a conditional branch other than its back edge.
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

// ---- tables: fp64, rounded once --------------------------------------------------------------------------------------
// Slaney mel scale (librosa.mel_frequencies, htk=False): point i of 130 equally spaced in mel over 0..8000 Hz, in Hz
__device__ double mel_point_hz(int i) {
  const double f_sp = 200.0 / 3.0, min_log_mel = 1000.0 / f_sp, logstep = log(6.4) / 27.0;
  const double mel_max = min_log_mel + log(8000.0 / 1000.0) / logstep;
  const double m = i == MF_MELS + 1 ? mel_max : i * (mel_max / (MF_MELS + 1));
  return m >= min_log_mel ? 1000.0 * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

__global__ __launch_bounds__(256) void mfcc_tables_k(float* __restrict__ tab) {
  const double two_pi = 6.283185307179586476925286766559;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < TB_END; i += (size_t)gridDim.x * 256) {
    double v = 0.0;
    if (i < TB_MEL) {                                   // hann[j] * cos|sin(2 pi j k / 400), the angle reduced exactly
      const int r = (int)(i % ((size_t)MF_NFFT * MF_BINP)), j = r / MF_BINP, k = r % MF_BINP;
      if (k < MF_BINS) {
        const double w = 0.5 - 0.5 * cos(two_pi * j / MF_NFFT), ang = two_pi * ((j * k) % MF_NFFT) / MF_NFFT;
        v = w * (i < TB_SIN ? cos(ang) : sin(ang));
      }
    } else if (i < TB_DCT) {                            // librosa.filters.mel(norm="slaney"), transposed: [bin][mel]
      const int r = (int)(i - TB_MEL), k = r / MF_MELS, m = r % MF_MELS;
      if (k < MF_BINS) {
        const double f = k * (8000.0 / (MF_BINS - 1)), f0 = mel_point_hz(m), f1 = mel_point_hz(m + 1), f2 = mel_point_hz(m + 2);
        const double lower = (f - f0) / (f1 - f0), upper = (f2 - f) / (f2 - f1);
        v = fmax(0.0, fmin(lower, upper)) * (2.0 / (f2 - f0));
      }
    } else if (i < TB_TAP) {                            // scipy.fft.dct(type=2, norm="ortho"), transposed: [mel][c]
      const int r = (int)(i - TB_DCT), m = r / MF_CMAX, c = r % MF_CMAX;
      const double ang = two_pi * ((c * (2 * m + 1)) % (4 * MF_MELS)) / (4 * MF_MELS);
      v = (c == 0 ? sqrt(1.0 / MF_MELS) : sqrt(2.0 / MF_MELS)) * cos(ang);
    } else {                                            // savgol taps, deriv = polyorder = 1, 2; y[t] = sum_k tap[k] x[t+k]
      const int r = (int)(i - TB_TAP), width = 3 + 2 * (r / 32), order = 1 + (r % 32) / 16, t = r % 16, h = width / 2;
      if (t < width) {
        double s2 = 0.0, s4 = 0.0;
        for (int q = -h; q <= h; ++q) { s2 += (double)q * q; s4 += (double)q * q * q * q; }
        const double k = t - h;
        v = order == 1 ? k / s2 : 2.0 * (width * k * k - s2) / (width * s4 - s2 * s2);
      }
    }
    tab[i] = (float)v;
  }
}

// ---- the featuriser --------------------------------------------------------------------------------------------------
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

__device__ __forceinline__ float sample_of(const float* p, long long i) { return p[i]; }
__device__ __forceinline__ float sample_of(const short* p, long long i) { return (float)p[i] * (1.0f / 32768.0f); }

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

template <typename AT>
__global__ __launch_bounds__(MF_THREADS) void mfcc_k(mfcc_args a) {
  __shared__ float s_aud[MF_AUD];               // a-b: padded clip;   c-d: dB image [112][129]
  __shared__ float s_pow[MF_ROWS * MF_PS];      // b-c: power [112][209];   d-e: coefficients [112][65]
  __shared__ float s_red[16];
  __shared__ float s_tap[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;     // MFMA operand maps: A[row lr][k lk], B[k lk][col lr]; C/D[row 4 lk + reg][col lr]
  const AT* src = reinterpret_cast<const AT*>(a.audio) + (long long)blockIdx.x * a.clip_stride;
  int len = a.L;
  if (a.lengths) len = min(max(a.lengths[blockIdx.x], MF_MINLEN), a.L);   // (whatever the caller wrote: reads stay inside the row)
  const int n = 1 + len / MF_HOP;
  if (tid < 32) s_tap[tid] = a.tab[TB_TAP + ((a.width - 3) >> 1) * 32 + tid];

  // ---- a. the padded clip: every load is issued (clamped into the clip), what lies outside becomes zero
  {
    float v[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) {
      const int s = tid + j * MF_THREADS - MF_PAD;
      v[j] = sample_of(src, (long long)min(max(s, 0), len - 1));
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
    f32x4 ac[7], as[7];
    int arow[7];
#pragma unroll
    for (int rt = 0; rt < 7; ++rt) {
      ac[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
      as[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
      arow[rt] = min(16 * rt + lr, MF_FRAMES - 1) * MF_RS + lk;    // (rows 101..111 repeat frame 100; nothing reads them back)
    }
    const float* bc = a.tab + TB_COS + (size_t)lk * MF_BINP + 16 * wave + lr;
    const float* bs = a.tab + TB_SIN + (size_t)lk * MF_BINP + 16 * wave + lr;
    for (int k0 = 0; k0 < MF_NFFT; k0 += 16) {
      const int ks = k0 + (k0 >= MF_HOP ? MF_SKEW : 0) + (k0 >= 2 * MF_HOP ? MF_SKEW : 0);   // (a batch never straddles a hop)
      float fa[4][7], fc[4], fs[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fc[u] = bc[(size_t)(k0 + 4 * u) * MF_BINP];
        fs[u] = bs[(size_t)(k0 + 4 * u) * MF_BINP];
#pragma unroll
        for (int rt = 0; rt < 7; ++rt) fa[u][rt] = s_aud[arow[rt] + ks + 4 * u];
      }
      __builtin_amdgcn_sched_barrier(0);          // every operand request of the batch in front of its first MFMA
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int rt = 0; rt < 7; ++rt) {
          ac[rt] = mfma4(fa[u][rt], fc[u], ac[rt]);
          as[rt] = mfma4(fa[u][rt], fs[u], as[rt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      completion_read(as[6][0]);                  // the youngest accumulator: the batch's registers are free again
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < 7; ++rt) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        s_pow[(16 * rt + 4 * lk + e) * MF_PS + 16 * wave + lr] = fmaf(ac[rt][e], ac[rt][e], as[rt][e] * as[rt][e]);
    }
  }
  __syncthreads();

  // ---- c. mel projection and dB: wave w owns mel columns 16 (w & 7).. and the row tiles of parity w >> 3
  float mx = -INFINITY;
  {
    const int ct = wave & 7, r0 = wave >> 3;
    f32x4 acc[4];
    int prow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      prow[i] = (16 * min(r0 + 2 * i, 6) + lr) * MF_PS + lk;      // (a fourth tile of the odd waves repeats tile 6, unstored)
    }
    const float* bw = a.tab + TB_MEL + (size_t)lk * MF_MELS + 16 * ct + lr;
    for (int k0 = 0; k0 < MF_BINP; k0 += 16) {
      float fa[4][4], fb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fb[u] = bw[(size_t)(k0 + 4 * u) * MF_MELS];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[u][i] = s_pow[prow[i] + k0 + 4 * u];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma4(fa[u][i], fb[u], acc[i]);
      }
      __builtin_amdgcn_sched_barrier(0);
      completion_read(acc[3][0]);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rt = r0 + 2 * i;
      if (rt < 7) {                               // (wave-uniform)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * rt + 4 * lk + e;
          const float db = 10.0f * log10f(fmaxf(1e-10f, acc[i][e]));
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

  // ---- d. DCT-II: wave w owns coefficient columns 16 (w & 3).. and row tiles w >> 2, (w >> 2) + 4
  {
    const int ct = wave & 3, r0 = wave >> 2;
    f32x4 acc[2];
    int drow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      drow[i] = (16 * min(r0 + 4 * i, 6) + lr) * MF_DS + lk;
    }
    const float* bd = a.tab + TB_DCT + (size_t)lk * MF_CMAX + 16 * ct + lr;
    for (int k0 = 0; k0 < MF_MELS; k0 += 16) {
      float fa[4][2], fb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        fb[u] = bd[(size_t)(k0 + 4 * u) * MF_CMAX];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[u][i] = fmaxf(s_aud[drow[i] + k0 + 4 * u], floor_db);
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
        for (int e = 0; e < 4; ++e) s_pow[(16 * rt + 4 * lk + e) * MF_CS + 16 * ct + lr] = acc[i][e];
      }
    }
  }
  __syncthreads();

  // ---- e. deltas, pad / cut, normalisation, stores: element i of the clip's [max_len][F] block
  const int C = a.n_mfcc, F = C * (a.order + 1), total = a.max_len * F, h = a.width >> 1;
  const int last = max(n - 1 - h, h);             // (n >= width for every length the caller may pass; in bounds for any)
  float* out = a.feats + (size_t)blockIdx.x * (size_t)total;
  const bool norm = a.mean != nullptr;
  for (int i = tid; i < total; i += MF_THREADS) {
    const int t = i / F, f = i - t * F, o = f / C, c = f - o * C;
    const int tt = min(t, n - 1);
    const int tc = min(max(tt, h), last) - h;     // first row under the FIR; the interp edges are constant (deriv == polyorder)
    float val = s_pow[tt * MF_CS + c], d = 0.f;
    const float* tap = s_tap + (o == 2 ? 16 : 0);
    for (int k = 0; k < a.width; ++k) d = fmaf(tap[k], s_pow[(tc + k) * MF_CS + c], d);
    val = o == 0 ? val : d;
    val = t < n ? val : 0.f;
    if (norm) val = (val - a.mean[f]) / a.stdv[f];
    out[i] = val;
  }
}

}  // namespace

size_t mfcc_tables_bytes() { return align256(TB_END * sizeof(float)); }

int mfcc_init_tables(void* tables, hipStream_t s) {
  hipLaunchKernelGGL(mfcc_tables_k, dim3(512), dim3(256), 0, s, reinterpret_cast<float*>(tables));
  return hipGetLastError() == hipSuccess ? FASTGRNN_OK : FASTGRNN_ERR_LAUNCH;
}

int mfcc_run(const fastgrnn_mfcc_desc& d, const void* audio, const int32_t* lengths, const void* tables, const float* mean,
             const float* stdv, void* feats, hipStream_t s) {
  mfcc_args a;
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
  if (d.audio_dtype == FASTGRNN_MFCC_AUDIO_I16)
    hipLaunchKernelGGL(mfcc_k<short>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(mfcc_k<float>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  return hipGetLastError() == hipSuccess ? FASTGRNN_OK : FASTGRNN_ERR_LAUNCH;
}

}  // namespace fastgrnn
