// The featuriser for the detector's overlapping clips of ONE recording: every 10 ms frame of the recording goes through
// the DFT and the mel projection once, not once per clip that contains it.  gfx950 only.  The semantics are spelled out
// in include/fastgrnn_hip.h (fastgrnn_hip_mfcc_stream_frames / _clips); the stages are mfcc_body.h's, the same code
// the per-clip kernels run (kernels_mfcc.hip describes them and the rules they keep).
//
// A clip that starts at a multiple of the hop, sample 160 kb, has frame r = the recording's frame g = kb + r.  Frames
// 2..98 read clip samples 120..15879 only: their mel power does not depend on the clip.  Frames 0, 1, 99, 100 see the
// clip's own zero padding.  Two kernels, a workspace between them:
//   stream_frames_k   one workgroup per SEGMENT of 101 global frames (g0 = 101 seg): stage a loads the 16 400 samples
//       160 g0 - 200 .. with their real neighbours (zeros outside the recording) into the body's skewed LDS image,
//       stages b and c are the body's (7 row tiles), and the mel power -- before the dB -- of frames g <= N / 160 goes
//       to the workspace, [G][128] fp32.  The block maxima max|y[160 j .. 160 j + 159]|, j = g0 .. g0 + 100, are read
//       off the same LDS image into the workspace's second region, [G] fp32.  Neighbouring segments share the 240
//       samples a frame straddles; no frame is computed twice.
//   stream_clips_k    one workgroup per clip.  The peak m is the maximum of the clip's 100 block maxima (exact, so
//       order-free: the per-clip kernel's m bit for bit).  The four edge frames are stage b on ONE row tile -- rows
//       q, q + 4, .. all hold edge frame q -- over the clip's first and last 560 padded samples, divided by m as the
//       per-clip kernel divides them; stage c on that tile.  The 97 interior rows come from the workspace, requested
//       before stage b and scaled (M s) s, s = 1 / m, one rounding each, on the way into the dB image.  From there
//       stages d and e are the body's.
// Without peak normalisation nothing is scaled and every row is the per-clip kernel's chain on the per-clip kernel's
// operands: the features are equal bit for bit.  No atomics; no LDS write in a loop with a branch; every MFMA loop is
// the shared one (operand batches, completion reads).
#include "mfcc_body.h"

namespace fastgrnn {
namespace {

constexpr int ST_SEG = MF_FRAMES;                 // global frames per segment of the frames kernel
constexpr int ST_EDGE = 560;                      // padded samples under frames 0, 1 (and under 99, 100)
constexpr int ST_ES = ST_EDGE + MF_SKEW * 4;      // words of one skewed edge piece
constexpr int ST_TAIL = 99 * MF_HOP;              // first padded sample of frame 99
constexpr int ST_INNER = 97;                      // frames 2..98

struct stream_args {
  const void* audio;
  const float* tab;
  float* mel;                                     // workspace: [G][128] mel power of the recording's frames
  float* blk;                                     //            [G] block maxima
  const float* mean;
  const float* stdv;
  float* feats;
  long long N;
  int G;                                          // N / 160 + 1 global frames
  int kh, clip0;                                  // hop / 160; first clip of this call
  int n_mfcc, order, width, max_len, peak;
  float top_db;
};

template <typename AT>
__global__ __launch_bounds__(MF_THREADS) void stream_frames_k(stream_args a) {
  __shared__ float s_aud[MF_AUD];
  __shared__ float s_pow[MF_ROWS * MF_PS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const AT* src = reinterpret_cast<const AT*>(a.audio);
  const int g0 = blockIdx.x * ST_SEG;
  const long long base = (long long)g0 * MF_HOP - MF_PAD;

  // ---- a. the segment with its real neighbours: every load is issued (clamped into the recording)
  {
    float v[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) {
      const long long q = base + tid + j * MF_THREADS;
      v[j] = sample_of(src, min(max(q, 0ll), a.N - 1));
    }
#pragma unroll
    for (int j = 0; j < 17; ++j) {
      const int i = tid + j * MF_THREADS;
      const long long q = base + i;
      const float y = (q >= 0 && q < a.N) ? v[j] : 0.f;
      if (i < MF_PADDED) s_aud[i + MF_SKEW * (i / MF_HOP)] = y;
    }
  }
  __syncthreads();

  // ---- block maxima: wave w takes blocks g0 + w, g0 + w + 16, .. (the seventh round repeats block 100)
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int jj = min(wave + 16 * j, ST_SEG - 1);
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int i = MF_PAD + MF_HOP * jj + min(lane + 64 * u, MF_HOP - 1);
      m = fmaxf(m, fabsf(s_aud[i + MF_SKEW * (i / MF_HOP)]));
    }
    m = wave_max(m);
    if (lane == 0 && g0 + jj < a.G) a.blk[g0 + jj] = m;
  }

  // ---- b. power spectrum, as the per-clip body runs it
  if (wave < 13) {                                // (wave-uniform, around the whole loop)
    int arow[7];
#pragma unroll
    for (int rt = 0; rt < 7; ++rt) arow[rt] = min(16 * rt + lr, MF_FRAMES - 1) * MF_RS + lk;
    mfcc_power<7>(s_aud, s_pow, a.tab, arow, wave, lr, lk);
  }
  __syncthreads();

  // ---- c. mel projection; the power itself is the result
  {
    const int ct = wave & 7, r0 = wave >> 3;
    f32x4 acc[4];
    int prow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) prow[i] = (16 * min(r0 + 2 * i, 6) + lr) * MF_PS + lk;
    mfcc_mel<4>(s_pow, a.tab, prow, ct, lr, lk, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rt = r0 + 2 * i;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * rt + 4 * lk + e, g = g0 + row;
        if (rt < 7 && row < ST_SEG && g < a.G) a.mel[(size_t)g * MF_MELS + 16 * ct + lr] = acc[i][e];
      }
    }
  }
}

template <typename AT>
__global__ __launch_bounds__(MF_THREADS) void stream_clips_k(stream_args a) {
  __shared__ float s_db[MF_ROWS * MF_DS];         // dB image [112][129]; rows 101.. repeat edge frames
  __shared__ float s_coef[MF_ROWS * MF_CS];       // coefficients [112][65]
  __shared__ float s_pow[16 * MF_PS];             // power of the edge tile [16][209]
  __shared__ float s_edge[2 * ST_ES];             // padded samples 0..559 and 15 840..16 399, skewed per hop
  __shared__ float s_red[16];
  __shared__ float s_tap[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int kb = (a.clip0 + (int)blockIdx.x) * a.kh;            // the clip's first global frame (and block)
  const AT* src = reinterpret_cast<const AT*>(a.audio) + (long long)kb * MF_HOP;
  if (tid < 32) s_tap[tid] = a.tab[TB_TAP + ((a.width - 3) >> 1) * 32 + tid];

  // ---- the clip's peak from its 100 block maxima, in every wave (no exchange)
  float m = fmaxf(a.blk[kb + lane], a.blk[kb + min(lane + 64, 99)]);
  m = wave_max(m);
  const bool scale = a.peak && m > 0.f;           // (uniform over the workgroup)
  const float s = 1.0f / m;

  // ---- interior frames 2..98: [97][128] mel power of the recording, four words per request (the fourth round's
  // rows past 98 repeat row 98 -- same words, same values)
  f32x4 in[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + j * MF_THREADS, row = 2 + min(i >> 5, ST_INNER - 1);
    in[j] = *reinterpret_cast<const f32x4*>(a.mel + (size_t)(kb + row) * MF_MELS + 4 * (i & 31));
  }

  // ---- a. the samples under the four edge frames, zero-padded as the clip's, y / m as the per-clip kernel's
  {
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = min(tid + j * MF_THREADS, 2 * ST_EDGE - 1), piece = e >= ST_EDGE ? 1 : 0;
      const int q = e - ST_EDGE * piece + ST_TAIL * piece - MF_PAD;     // clip sample
      v[j] = sample_of(src, (long long)min(max(q, 0), 15999));
      v[j] = (q >= 0 && q < 16000) ? v[j] : 0.f;
      v[j] = scale ? v[j] / m : v[j];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = min(tid + j * MF_THREADS, 2 * ST_EDGE - 1), piece = e >= ST_EDGE ? 1 : 0;
      const int il = e - ST_EDGE * piece;
      s_edge[piece * ST_ES + il + MF_SKEW * (il / MF_HOP)] = v[j];     // (past 1119: sample 1119 again)
    }
  }
  __syncthreads();

  // ---- b. power spectrum of one row tile: row q + 4 i is edge frame {0, 1, 99, 100}[q]
  if (wave < 13) {                                // (wave-uniform, around the whole loop)
    const int q = lr & 3;
    const int arow[1] = {(q >> 1) * ST_ES + (q & 1) * MF_RS + lk};
    mfcc_power<1>(s_edge, s_pow, a.tab, arow, wave, lr, lk);
  }

  // ---- the interior rows of the dB image
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + j * MF_THREADS, row = 2 + min(i >> 5, ST_INNER - 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = scale ? mul_rn(mul_rn(in[j][e], s), s) : in[j][e];
      const float db = mfcc_db(p);
      s_db[row * MF_DS + 4 * (i & 31) + e] = db;
      mx = fmaxf(mx, db);
    }
  }
  __syncthreads();

  // ---- c. mel projection and dB of the edge tile: wave w < 8 owns mel columns 16 w..
  if (wave < 8) {                                 // (wave-uniform, around the whole loop)
    f32x4 acc[1];
    const int prow[1] = {lr * MF_PS + lk};
    mfcc_mel<1>(s_pow, a.tab, prow, wave, lr, lk, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // row 4 lk + e of the tile is edge frame e; lk = 0 writes it where it belongs, the copies fill rows 101..111
      const int row = lk == 0 ? (e < 2 ? e : 97 + e) : min(97 + 4 * lk + e, MF_ROWS - 1);
      const float db = mfcc_db(acc[0][e]);
      s_db[row * MF_DS + 16 * wave + lr] = db;
      mx = fmaxf(mx, db);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = s_red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = fmaxf(mx, s_red[w]);
  const float floor_db = a.top_db >= 0.f ? mx - a.top_db : -INFINITY;

  // ---- d, e: as the per-clip body
  mfcc_dct(s_db, s_coef, a.tab, floor_db, wave, lr, lk);
  __syncthreads();
  const int total = a.max_len * a.n_mfcc * (a.order + 1);
  mfcc_rows(s_coef, s_tap, MF_FRAMES, a.n_mfcc, a.order, a.width, a.max_len, a.mean, a.stdv,
            a.feats + (size_t)blockIdx.x * (size_t)total, tid);
}

struct stream_ws {
  float* mel;
  float* blk;
  size_t bytes;
};

stream_ws stream_layout(const fastgrnn_mfcc_stream_desc& d, void* ws) {
  const size_t G = (size_t)(d.N / MF_HOP) + 1;
  Carve c(ws);
  stream_ws w;
  w.mel = c.take<float>(G * MF_MELS);
  w.blk = c.take<float>(G);
  w.bytes = c.off;
  return w;
}

stream_args stream_pack(const fastgrnn_mfcc_stream_desc& d, const void* audio, const void* tables, void* ws) {
  const stream_ws w = stream_layout(d, ws);
  stream_args a;
  a.audio = audio;
  a.tab = reinterpret_cast<const float*>(tables);
  a.mel = w.mel;
  a.blk = w.blk;
  a.mean = a.stdv = nullptr;
  a.feats = nullptr;
  a.N = d.N;
  a.G = (int)(d.N / MF_HOP) + 1;
  a.kh = d.hop / MF_HOP;
  a.clip0 = d.clip0;
  a.n_mfcc = d.n_mfcc;
  a.order = d.order;
  a.width = d.width;
  a.max_len = d.max_len;
  a.peak = (d.flags & FASTGRNN_MFCC_PEAK_NORMALIZE) ? 1 : 0;
  a.top_db = d.top_db;
  return a;
}

}  // namespace

size_t mfcc_stream_ws_bytes(const fastgrnn_mfcc_stream_desc& d) { return stream_layout(d, nullptr).bytes; }

int mfcc_stream_frames_run(const fastgrnn_mfcc_stream_desc& d, const void* audio, const void* tables, void* ws,
                           hipStream_t s) {
  const stream_args a = stream_pack(d, audio, tables, ws);
  const dim3 grid((a.G + ST_SEG - 1) / ST_SEG);
  if (d.audio_dtype == FASTGRNN_MFCC_AUDIO_I16)
    hipLaunchKernelGGL(stream_frames_k<short>, grid, dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(stream_frames_k<float>, grid, dim3(MF_THREADS), 0, s, a);
  return launch_status();
}

int mfcc_stream_clips_run(const fastgrnn_mfcc_stream_desc& d, const void* audio, const void* tables, void* ws,
                          const float* mean, const float* stdv, void* feats, hipStream_t s) {
  stream_args a = stream_pack(d, audio, tables, ws);
  a.mean = mean;
  a.stdv = stdv;
  a.feats = reinterpret_cast<float*>(feats);
  if (d.audio_dtype == FASTGRNN_MFCC_AUDIO_I16)
    hipLaunchKernelGGL(stream_clips_k<short>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(stream_clips_k<float>, dim3(d.B), dim3(MF_THREADS), 0, s, a);
  return launch_status();
}

}  // namespace fastgrnn
