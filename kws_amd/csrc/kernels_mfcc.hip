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
// The body itself is mfcc_body.h: kernels_augment.hip instantiates it a second time, reading an audio bank through
// augmentation records in stage a.
#include "mfcc_body.h"

namespace fastgrnn {
namespace {

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
template <typename AT>
__global__ __launch_bounds__(MF_THREADS) void mfcc_k(mfcc_args a) {
  mfcc_body<AT, false>(a);
}

}  // namespace

size_t mfcc_tables_bytes() { return align256(TB_END * sizeof(float)); }

int mfcc_init_tables(void* tables, hipStream_t s) {
  hipLaunchKernelGGL(mfcc_tables_k, dim3(512), dim3(256), 0, s, reinterpret_cast<float*>(tables));
  return launch_status();
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
  return launch_status();
}

}  // namespace fastgrnn
