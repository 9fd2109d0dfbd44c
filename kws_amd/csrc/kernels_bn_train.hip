// Training-mode BatchNorm FastGRNN (the reference's FastGRNNBatchNormCell, rnn.py:316-452, every BatchNorm1d in
// training mode): forward and backward recurrences, fp32, dense H = 128 / 256 (include/fastgrnn_hip.h,
// FASTGRNN_FLAG_BN_TRAIN).
//
// Per frame t the four BatchNorm layers need statistics over the whole batch, so the scan is ONE LAUNCH PER FRAME.
// Workgroups split the batch (rows); every workgroup writes per-unit partial sums of its rows, and the workgroup that
// arrives last at the frame's counter (split-K hand-off: agent-scope release before the ticket, acquire after it)
// combines them in a fixed order and writes the frame's statistics.  The next launch reads them.  No workgroup ever
// waits for another, so no grid can deadlock, and no float atomics are used: two identical calls are bitwise equal.
// The counters are zeroed by a memset node at the start of every call (graph replay included).
//
// Forward, launch t (t = 0 .. T): finish frame t-1 for the workgroup's rows (BatchNorm with the frame's statistics,
// gate / update, h_{t-1} -> hs), then uC_t = h_{t-1} . U^T for the same rows (fp32 FMA, h rows in LDS) -> saved,
// and the rows' partials of frame t: local mean, centred sum of squares of uC, co-moment with wC, centred sum of wC.
// The statistics of wC = X . W^T do not depend on the recurrence: one pass over all frames before the scan.
//   bn_gate / bn_update normalise the same s = bn_w(wC) + bn_u(uC) (+ a per-unit bias that cancels): mean(s) is
//   beta_w + beta_u, var(s) = g_w^2 v_w/(v_w+e_w) + g_u^2 v_u/(v_u+e_u) + 2 g_w g_u cov/sqrt((v_w+e_w)(v_u+e_u)).
// Backward, launch t (t = T-1 .. -1): finish frame t+1 (its BatchNorm backward with the frame's reduced sums:
// d uC, d wC), d h_t = grad_hs[t] + z_{t+1} d h_{t+1} + d uC_{t+1} . U, then frame t's d pre-activations and their
// partial sums (sum dpg, dpu, and their products with d, n_u, n_w; the zeta / nu terms).  The weight gradients and
// d_x are the existing split-precision GEMMs behind the scan.
#include "common.h"

namespace fastgrnn {
namespace {

constexpr int BNT_THREADS = 256;
constexpr int BNT_CHUNK = 16;        // rows of a workgroup's LDS tile per pass
constexpr int BNT_MAX_WG = 128;      // rows are spread over at most this many workgroups (the last arriver's reads)
constexpr int BNT_KF = 6;            // forward partials per unit (bnt_fwd_step: 4, bnt_fwd_sstat: 6)
constexpr int BNT_KB = 10;           // backward sums per unit (see bnt_bwd_step)
// per-frame statistics per unit: 0 mean_w, 1 var_w, 2 mean_u, 3 var_u, 4 cov(wC, uC) (bnt_fwd_step), 5 mean(d),
// 6 var(d), 7 mean((d - mean d) n_u), 8 mean((d - mean d) n_w) (bnt_fwd_sstat), d = g_w n_w + g_u n_u
constexpr int BNT_KS = 9;

struct BnConst {
  const float *gw, *bw, *gu, *bu, *gg, *bg, *gc, *bc;
  float ew, eu, eg, ec;
  const float *zeta, *nu;
};

// per-unit constants of one frame (fp64: a few scalars per unit and frame)
struct FrameUnit {
  double mw, iw, mu, iu, gw, gu, md, ig, ic, gg, bg, gc, bc, dnu, dnw;
};

// full = false: only what d = g_w n_w + g_u n_u needs (bnt_fwd_sstat, before the frame's d statistics exist)
__device__ __forceinline__ FrameUnit frame_unit(const double* __restrict__ st, int H, int j, const BnConst& k,
                                                bool full = true) {
  FrameUnit f;
  f.mw = st[j];
  f.iw = 1.0 / sqrt(st[H + j] + (double)k.ew);
  f.mu = st[2 * H + j];
  f.iu = 1.0 / sqrt(st[3 * H + j] + (double)k.eu);
  f.gw = k.gw[j];
  f.gu = k.gu[j];
  f.md = f.ig = f.ic = f.gg = f.bg = f.gc = f.bc = f.dnu = f.dnw = 0.0;
  if (full) {
    const double vd = st[6 * H + j];
    f.md = st[5 * H + j];
    f.ig = 1.0 / sqrt(vd + (double)k.eg);
    f.ic = 1.0 / sqrt(vd + (double)k.ec);
    f.gg = k.gg[j];
    f.bg = k.bg[j];
    f.gc = k.gc[j];
    f.bc = k.bc[j];
    f.dnu = st[7 * H + j];
    f.dnw = st[8 * H + j];
  }
  return f;
}

// the normalised inputs of one element and d - mean(d): the same expression in every kernel
__device__ __forceinline__ void bn_pre(float wcv, float ucv, const FrameUnit& f, double& nw, double& nu, double& dc) {
  nw = ((double)wcv - f.mw) * f.iw;
  nu = ((double)ucv - f.mu) * f.iu;
  dc = f.gw * nw + f.gu * nu - f.md;
}

__device__ __forceinline__ size_t seq_row(int b, int t, int B, int T, bool bm) {
  return bm ? (size_t)b * T + t : (size_t)t * B + b;
}

// d uC rows for the dU GEMM (C = dUC^T . H_prev with rows of H_prev below B from h0, the rest hs shifted by B rows):
// time-major: row t*B + b.  Batch-major: rows 0..B-1 hold frame 0 (paired with h0), row B + b*T + t holds frame t+1
// (paired with hs[b, t]); row B + b*T + T-1 is zero.
__device__ __forceinline__ size_t duc_row(int b, int t, int B, int T, bool bm) {
  return bm ? (t == 0 ? (size_t)b : (size_t)B + (size_t)b * T + t - 1) : (size_t)t * B + b;
}

// Split-K hand-off (cdna_hip_programming.md, Guideline 16): returns true in every thread of the last-arriving
// workgroup, after which the other workgroups' partials are visible to it.  flag: one LDS word.
__device__ __forceinline__ bool arrive_last(unsigned* cnt, unsigned nwg, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == nwg - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

__device__ __forceinline__ float gate_act(float a, int nl) {
  return nl == FASTGRNN_NL_SIGMOID ? 1.0f / (1.0f + expf(-a)) : (nl == FASTGRNN_NL_RELU ? (a > 0.f ? a : 0.f) : tanhf(a));
}
__device__ __forceinline__ float gate_dact(float y, int nl) {
  return nl == FASTGRNN_NL_SIGMOID ? (1.0f - y) * y : (nl == FASTGRNN_NL_RELU ? (y > 0.f ? 1.0f : 0.0f) : 1.0f - y * y);
}
__device__ __forceinline__ float sigm(float a) { return 1.0f / (1.0f + expf(-a)); }

// rows of the partial p = wg * RG + rg: the workgroup's rows [r0, r1) with (row - r0) % RG == rg
__device__ __forceinline__ int part_rows(int p, int RG, int rpw, int B) {
  const int wg = p / RG, rg = p % RG;
  const int r0 = wg * rpw;
  const int n = (B - r0 < rpw ? B - r0 : rpw);
  return n > rg ? (n - rg + RG - 1) / RG : 0;
}

// ---- statistics of wC per frame and unit (mean, biased variance: two passes) ------------------------------------
// grid (T, H / 64), block 256 = 64 units x 4 row groups
__global__ __launch_bounds__(256) void bnt_wstats(int T, int B, int H, bool bm, const float* __restrict__ wc,
                                                  double* __restrict__ stats) {
  __shared__ double red[4][64];
  const int t = blockIdx.x, jl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + jl;
  double s = 0.0;
  for (int b = rg; b < B; b += 4) s += wc[seq_row(b, t, B, T, bm) * H + j];
  red[rg][jl] = s;
  __syncthreads();
  const double mean = (((red[0][jl] + red[1][jl]) + red[2][jl]) + red[3][jl]) / (double)B;
  __syncthreads();
  double m2 = 0.0;
  for (int b = rg; b < B; b += 4) {
    const double v = wc[seq_row(b, t, B, T, bm) * H + j] - mean;
    m2 += v * v;
  }
  red[rg][jl] = m2;
  __syncthreads();
  if (rg == 0) {
    stats[(size_t)t * BNT_KS * H + j] = mean;
    stats[(size_t)t * BNT_KS * H + H + j] = (((red[0][jl] + red[1][jl]) + red[2][jl]) + red[3][jl]) / (double)B;
  }
}

// ---- frame product for F = 32 (rows_gemm takes K >= 64): wc[r, j] = sum_f x[r, f] w[j, f] ------------------------
template <int H>
__global__ __launch_bounds__(256) void bnt_frame_f32(size_t R, const float* __restrict__ x, const float* __restrict__ w,
                                                     float* __restrict__ wc) {
  constexpr int F = 32, RG = BNT_THREADS / H, RPT = BNT_CHUNK / RG;
  __shared__ float xs[BNT_CHUNK][F];
  const int j = threadIdx.x % H, rg = threadIdx.x / H;
  float wr[F];
#pragma unroll
  for (int f = 0; f < F; ++f) wr[f] = w[(size_t)j * F + f];
  const size_t r0 = (size_t)blockIdx.x * BNT_CHUNK;
  for (int e = threadIdx.x; e < BNT_CHUNK * F; e += BNT_THREADS) {
    const size_t r = r0 + e / F;
    xs[e / F][e % F] = r < R ? x[r * F + e % F] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int rr = rg + RG * i;
    float a = 0.f;
#pragma unroll
    for (int f = 0; f < F; ++f) a = fmaf(xs[rr][f], wr[f], a);
    if (r0 + rr < R) wc[(r0 + rr) * H + j] = a;
  }
}

// u [out,in] -> ut[k][j] = u[j][k]
__global__ __launch_bounds__(256) void bnt_transpose(int H, const float* __restrict__ u, float* __restrict__ ut) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)H * H) {
    const int k = (int)(e / H), j = (int)(e % H);
    ut[e] = u[(size_t)j * H + k];
  }
}

// ---- forward: one launch per frame ---------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(256) void bnt_fwd_step(int t, int T, int B, int rpw, int nwg, bool bm, int gate_nl,
                                                    BnConst k, const float* __restrict__ wc,
                                                    const float* __restrict__ ut, const float* __restrict__ h0,
                                                    float* __restrict__ hs, float* __restrict__ uc,
                                                    double* __restrict__ stats, double* __restrict__ part,
                                                    unsigned* __restrict__ cnt) {
  constexpr int RG = BNT_THREADS / H, RPT = BNT_CHUNK / RG;
  __shared__ __attribute__((aligned(16))) double lds[BNT_CHUNK * H + 2];
  double (*hp)[H] = reinterpret_cast<double (*)[H]>(lds);
  const int j = threadIdx.x % H, rg = threadIdx.x / H;
  const int wg = blockIdx.x;
  const int r0 = wg * rpw, nrows = (B - r0 < rpw ? B - r0 : rpw);
  const float zs = sigm(k.zeta[0]), ns = sigm(k.nu[0]);
  FrameUnit fp;                                          // frame t-1
  if (t > 0) fp = frame_unit(stats + (size_t)(t - 1) * BNT_KS * H, H, j, k);
  const double mw = t < T ? stats[(size_t)t * BNT_KS * H + j] : 0.0;
  double su = 0.0;
  for (int c0 = 0; c0 < nrows; c0 += BNT_CHUNK) {
    // finish frame t-1 for the chunk (or load h0), into LDS
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int rr = rg + RG * i, lr = c0 + rr;
      float h = 0.f;
      if (lr < nrows) {
        const int b = r0 + lr;
        if (t == 0) {
          h = h0[(size_t)b * H + j];
        } else {
          const float hprev = t == 1 ? h0[(size_t)b * H + j] : hs[seq_row(b, t - 2, B, T, bm) * H + j];
          double nw, nu, d;
          bn_pre(wc[seq_row(b, t - 1, B, T, bm) * H + j], uc[((size_t)(t - 1) * B + b) * H + j], fp, nw, nu, d);
          const float z = gate_act((float)(fp.gg * (d * fp.ig) + fp.bg), gate_nl);
          const float cc = tanhf((float)(fp.gc * (d * fp.ic) + fp.bc));
          h = z * hprev + (zs * (1.0f - z) + ns) * cc;
          hs[seq_row(b, t - 1, B, T, bm) * H + j] = h;
        }
      }
      hp[rr][j] = h;
    }
    __syncthreads();
    if (t < T) {
      // fp32 operands, exact products, fp64 accumulation
      double acc[RPT];
#pragma unroll
      for (int i = 0; i < RPT; ++i) acc[i] = 0.0;
#pragma unroll 16
      for (int kk = 0; kk < H; kk += 2) {                 // (unrolled: 32 loads of U in flight, not one L2 trip per k)
        const double u0 = ut[(size_t)(kk + 0) * H + j], u1 = ut[(size_t)(kk + 1) * H + j];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          const double2 hv = *reinterpret_cast<const double2*>(&hp[rg + RG * i][kk]);
          acc[i] = fma(hv.x, u0, acc[i]);
          acc[i] = fma(hv.y, u1, acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int lr = c0 + rg + RG * i;
        if (lr < nrows) {
          const float v = (float)acc[i];
          uc[((size_t)t * B + r0 + lr) * H + j] = v;
          su += v;
        }
      }
    }
    __syncthreads();
  }
  if (t >= T) return;
  // partials of frame t over this thread's rows (the rows it wrote itself)
  const int p = wg * RG + rg;
  const int n = part_rows(p, RG, rpw, B);
  const double m = n > 0 ? su / (double)n : 0.0;
  double m2 = 0.0, cw = 0.0, sw = 0.0;
  for (int lr = rg; lr < nrows; lr += RG) {
    const int b = r0 + lr;
    const double du = uc[((size_t)t * B + b) * H + j] - m;
    const double dw = wc[seq_row(b, t, B, T, bm) * H + j] - mw;
    m2 += du * du;
    cw += dw * du;
    sw += dw;
  }
  double* pp = part + (size_t)p * BNT_KF * H;
  pp[j] = m;
  pp[H + j] = m2;
  pp[2 * H + j] = cw;
  pp[3 * H + j] = sw;
  if (!arrive_last(cnt + t, (unsigned)nwg, reinterpret_cast<int*>(lds + BNT_CHUNK * H))) return;
  if (rg != 0) return;
  // last arriver: combine every partial in a fixed order (Chan et al.: mean first, then the centred sums)
  const int P = nwg * RG;
  double mean = 0.0;
  for (int q = 0; q < P; ++q) mean += (double)part_rows(q, RG, rpw, B) * part[(size_t)q * BNT_KF * H + j];
  mean /= (double)B;
  double M2 = 0.0, CV = 0.0;
  for (int q = 0; q < P; ++q) {
    const double* pq = part + (size_t)q * BNT_KF * H;
    const double nq = (double)part_rows(q, RG, rpw, B);
    const double dm = pq[j] - mean;
    M2 += pq[H + j] + nq * dm * dm;
    CV += pq[2 * H + j] + dm * pq[3 * H + j];
  }
  double* st = stats + (size_t)t * BNT_KS * H;
  st[2 * H + j] = mean;
  st[3 * H + j] = M2 / (double)B;
  st[4 * H + j] = CV / (double)B;
}

// ---- forward, second reduction of frame t: mean and variance of d = g_w n_w + g_u n_u (bn_gate / bn_update
// normalise d plus a per-unit constant) and its co-moments with n_u, n_w (the BatchNorm backward's coupling terms),
// formed from the values the other kernels use.  var(d) from the variances and the covariance of wC and uC alone
// cancels when g_w n_w and g_u n_u nearly cancel (at B = 2 every unit's two inputs are perfectly correlated).
template <int H>
__global__ __launch_bounds__(256) void bnt_fwd_sstat(int t, int T, int B, int rpw, int nwg, bool bm, BnConst k,
                                                     const float* __restrict__ wc, const float* __restrict__ uc,
                                                     double* __restrict__ stats, double* __restrict__ part,
                                                     unsigned* __restrict__ cnt) {
  constexpr int RG = BNT_THREADS / H;
  __shared__ int flag[1];
  const int j = threadIdx.x % H, rg = threadIdx.x / H;
  const int wg = blockIdx.x;
  const int r0 = wg * rpw, nrows = (B - r0 < rpw ? B - r0 : rpw);
  double* st = stats + (size_t)t * BNT_KS * H;
  const FrameUnit f = frame_unit(st, H, j, k, false);
  const int p = wg * RG + rg;
  const int n = part_rows(p, RG, rpw, B);
  double sd = 0.0;
  for (int lr = rg; lr < nrows; lr += RG) {
    const int b = r0 + lr;
    double nw, nu, d;
    bn_pre(wc[seq_row(b, t, B, T, bm) * H + j], uc[((size_t)t * B + b) * H + j], f, nw, nu, d);
    sd += d;
  }
  const double m = n > 0 ? sd / (double)n : 0.0;
  double m2 = 0.0, cu = 0.0, cw = 0.0, su = 0.0, sw = 0.0;
  for (int lr = rg; lr < nrows; lr += RG) {
    const int b = r0 + lr;
    double nw, nu, d;
    bn_pre(wc[seq_row(b, t, B, T, bm) * H + j], uc[((size_t)t * B + b) * H + j], f, nw, nu, d);
    const double dd = d - m;
    m2 += dd * dd;
    cu += dd * nu;
    cw += dd * nw;
    su += nu;
    sw += nw;
  }
  double* pp = part + (size_t)p * BNT_KF * H;
  pp[j] = m;
  pp[H + j] = m2;
  pp[2 * H + j] = cu;
  pp[3 * H + j] = cw;
  pp[4 * H + j] = su;
  pp[5 * H + j] = sw;
  if (!arrive_last(cnt + t, (unsigned)nwg, flag)) return;
  if (rg != 0) return;
  const int P = nwg * RG;
  double mean = 0.0;
  for (int q = 0; q < P; ++q) mean += (double)part_rows(q, RG, rpw, B) * part[(size_t)q * BNT_KF * H + j];
  mean /= (double)B;
  double M2 = 0.0, CU = 0.0, CW = 0.0;
  for (int q = 0; q < P; ++q) {
    const double* pq = part + (size_t)q * BNT_KF * H;
    const double nq = (double)part_rows(q, RG, rpw, B);
    const double dm = pq[j] - mean;
    M2 += pq[H + j] + nq * dm * dm;
    CU += pq[2 * H + j] + dm * pq[4 * H + j];
    CW += pq[3 * H + j] + dm * pq[5 * H + j];
  }
  st[5 * H + j] = mean;
  st[6 * H + j] = M2 / (double)B;
  st[7 * H + j] = CU / (double)B;
  st[8 * H + j] = CW / (double)B;
}

// running statistics: T updates per layer in frame order.  grid 4 (bn_w, bn_u, bn_gate, bn_update), block H.
struct RunStat {
  float* mean[4];
  float* var[4];
  const int64_t* nbt[4];
  float mom[4];                 // < 0: cumulative average (momentum=None)
};

__global__ __launch_bounds__(256) void bnt_running(int T, int B, int H, BnConst k, const float* __restrict__ bias_gate,
                                                   const float* __restrict__ bias_update, const double* __restrict__ stats,
                                                   RunStat rs) {
  const int which = blockIdx.x, j = threadIdx.x;
  if (j >= H) return;
  float* rm = rs.mean[which];
  float* rv = rs.var[which];
  float m = rm[j], v = rv[j];
  const double n0 = rs.mom[which] < 0.f ? (double)rs.nbt[which][0] : 0.0;
  const float unbias = (float)B / (float)(B - 1);
  const float shift = which == 2 ? k.bw[j] + k.bu[j] + bias_gate[j] : k.bw[j] + k.bu[j] + bias_update[j];
  for (int t = 0; t < T; ++t) {
    const double* st = stats + (size_t)t * BNT_KS * H;
    float mean, var;
    if (which == 0) {
      mean = (float)st[j];
      var = (float)st[H + j];
    } else if (which == 1) {
      mean = (float)st[2 * H + j];
      var = (float)st[3 * H + j];
    } else {
      mean = (float)((double)shift + st[5 * H + j]);
      var = (float)st[6 * H + j];
    }
    const float f = rs.mom[which] < 0.f ? (float)(1.0 / (n0 + t + 1)) : rs.mom[which];
    m = f * mean + (1.0f - f) * m;
    v = f * (var * unbias) + (1.0f - f) * v;
  }
  rm[j] = m;
  rv[j] = v;
}

// ---- backward: one launch per frame, t = T-1 .. -1 ------------------------------------------------------------------
// sums per unit (index: meaning):  0 dpg  1 dpu  2 dpg.d  3 dpu.d  4 dpg.n_u  5 dpu.n_u  6 dpg.n_w  7 dpu.n_w
//                                  8 dh (1-z) c  9 dh c
template <int H>
__global__ __launch_bounds__(256) void bnt_bwd_step(int t, int T, int B, int rpw, int nwg, bool bm, int gate_nl,
                                                    BnConst k, const float* __restrict__ wc,
                                                    const float* __restrict__ u, const float* __restrict__ h0,
                                                    const float* __restrict__ hs, const float* __restrict__ ghs,
                                                    const float* __restrict__ uc, const double* __restrict__ stats,
                                                    float* __restrict__ dpg_s, float* __restrict__ dpu_s,
                                                    float* __restrict__ dhz_s, float* __restrict__ duc,
                                                    float* __restrict__ dwc, double* __restrict__ red,
                                                    double* __restrict__ part, unsigned* __restrict__ cnt,
                                                    float* __restrict__ d_h0) {
  constexpr int RG = BNT_THREADS / H, RPT = BNT_CHUNK / RG;
  __shared__ __attribute__((aligned(16))) double lds[BNT_CHUNK * H + 2];
  double (*dl)[H] = reinterpret_cast<double (*)[H]>(lds);
  const int j = threadIdx.x % H, rg = threadIdx.x / H;
  const int wg = blockIdx.x;
  const int r0 = wg * rpw, nrows = (B - r0 < rpw ? B - r0 : rpw);
  const float zs = sigm(k.zeta[0]), ns = sigm(k.nu[0]);
  const bool have_next = t + 1 <= T - 1;
  // frame t+1: BatchNorm backward coefficients from its reduced sums
  // (fp64: ddu / ddw are differences of nearly equal terms)
  double cg = 0.0, cc = 0.0, kg = 0.0, kc = 0.0, ddu = 0.0, ddw = 0.0, fu = 0.0, fw = 0.0;
  FrameUnit fn;
  if (have_next) {
    fn = frame_unit(stats + (size_t)(t + 1) * BNT_KS * H, H, j, k);
    const double* r = red + (size_t)(t + 1) * BNT_KB * H;
    const double ag = fn.gg * fn.ig, ac = fn.gc * fn.ic;
    // dd = ag (dpg - Sg/B - d ig^2 Sgd/B) + ac (dpu - Sc/B - d ic^2 Scd/B),  d centred
    cg = ag;
    cc = ac;
    kg = (ag * r[j] + ac * r[H + j]) / B;                                             // constant part
    kc = (ag * fn.ig * fn.ig * r[2 * H + j] + ac * fn.ic * fn.ic * r[3 * H + j]) / B;   // coefficient of d
    ddu = ag * r[4 * H + j] + ac * r[5 * H + j] - kc * B * fn.dnu;                      // sum dd n_u
    ddw = ag * r[6 * H + j] + ac * r[7 * H + j] - kc * B * fn.dnw;                      // sum dd n_w
    fu = fn.gu * fn.iu;
    fw = fn.gw * fn.iw;
  }
  FrameUnit fc;
  if (t >= 0) fc = frame_unit(stats + (size_t)t * BNT_KS * H, H, j, k);
  double s[BNT_KB];                                      // (fp64: zeta / nu sum terms that largely cancel)
#pragma unroll
  for (int q = 0; q < BNT_KB; ++q) s[q] = 0.0;
  for (int c0 = 0; c0 < nrows; c0 += BNT_CHUNK) {
    float dhz[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int rr = rg + RG * i, lr = c0 + rr;
      float v = 0.f;
      dhz[i] = 0.f;
      if (lr < nrows) {
        const int b = r0 + lr;
        if (have_next) {
          const size_t e = (size_t)b * H + j;
          double nw, nu, d;
          bn_pre(wc[seq_row(b, t + 1, B, T, bm) * H + j], uc[((size_t)(t + 1) * B + b) * H + j], fn, nw, nu, d);
          const double dd = cg * dpg_s[e] + cc * dpu_s[e] - kg - kc * d;
          v = (float)(fu * (dd - nu * ddu / B));
          duc[duc_row(b, t + 1, B, T, bm) * H + j] = v;
          dwc[seq_row(b, t + 1, B, T, bm) * H + j] = (float)(fw * (dd - nw * ddw / B));
          dhz[i] = dhz_s[e];
        } else if (bm) {
          duc[((size_t)B + (size_t)b * T + T - 1) * H + j] = 0.f;      // no frame T: the row that pairs with h_{T-1}
        }
      }
      dl[rr][j] = v;
    }
    __syncthreads();
    // d h_t = dhz + d uC_{t+1} . U   (u: [out,in], coalesced over this thread's column j)
    double acc[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) acc[i] = 0.0;
    if (have_next) {
#pragma unroll 16
      for (int kk = 0; kk < H; kk += 2) {
        const double u0 = u[(size_t)(kk + 0) * H + j], u1 = u[(size_t)(kk + 1) * H + j];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          const double2 dv = *reinterpret_cast<const double2*>(&dl[rg + RG * i][kk]);
          acc[i] = fma(dv.x, u0, acc[i]);
          acc[i] = fma(dv.y, u1, acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int lr = c0 + rg + RG * i;
      if (lr >= nrows) continue;
      const int b = r0 + lr;
      const size_t e = (size_t)b * H + j;
      float dh = (float)acc[i] + dhz[i];
      if (t < 0) {
        d_h0[e] = dh;
        continue;
      }
      dh += ghs[seq_row(b, t, B, T, bm) * H + j];
      const float hprev = t == 0 ? h0[e] : hs[seq_row(b, t - 1, B, T, bm) * H + j];
      double nw, nu, d;
      bn_pre(wc[seq_row(b, t, B, T, bm) * H + j], uc[((size_t)t * B + b) * H + j], fc, nw, nu, d);
      const float z = gate_act((float)(fc.gg * (d * fc.ig) + fc.bg), gate_nl);
      const float c = tanhf((float)(fc.gc * (d * fc.ic) + fc.bc));
      const float dz = dh * (hprev - zs * c);
      const float dc = dh * (zs * (1.0f - z) + ns);
      const float dpg = dz * gate_dact(z, gate_nl);
      const float dpu = dc * (1.0f - c * c);
      dpg_s[e] = dpg;
      dpu_s[e] = dpu;
      dhz_s[e] = dh * z;
      s[0] += dpg;
      s[1] += dpu;
      s[2] += dpg * d;
      s[3] += dpu * d;
      s[4] += dpg * nu;
      s[5] += dpu * nu;
      s[6] += dpg * nw;
      s[7] += dpu * nw;
      s[8] += (double)(dh * (1.0f - z)) * c;
      s[9] += (double)dh * c;
    }
    __syncthreads();
  }
  if (t < 0) return;
  const int p = wg * RG + rg;
  double* pp = part + (size_t)p * BNT_KB * H;
#pragma unroll
  for (int q = 0; q < BNT_KB; ++q) pp[q * H + j] = s[q];
  if (!arrive_last(cnt + t, (unsigned)nwg, reinterpret_cast<int*>(lds + BNT_CHUNK * H))) return;
  if (rg != 0) return;
  const int P = nwg * RG;
  double* r = red + (size_t)t * BNT_KB * H;
#pragma unroll
  for (int q = 0; q < BNT_KB; ++q) {
    double a = 0.0;
    for (int pq = 0; pq < P; ++pq) a += part[((size_t)pq * BNT_KB + q) * H + j];
    r[q * H + j] = a;
  }
}

// BatchNorm affine, zeta / nu gradients from the per-frame sums.  One workgroup of 256 threads.
struct BnGradOut {
  float *dgw, *dbw, *dgu, *dbu, *dgg, *dbg, *dgc, *dbc, *dbias_gate, *dbias_update, *dzeta, *dnu;
};

// (fp64 accumulators over frames and units: zeta and nu sum T x H per-frame sums that largely cancel)
__global__ __launch_bounds__(256) void bnt_param_grads(int T, int B, int H, BnConst k, const double* __restrict__ stats,
                                                       const double* __restrict__ red, BnGradOut o) {
  __shared__ double sz[256], sn[256];
  const int j = threadIdx.x;
  double a_gg = 0.0, a_bg = 0.0, a_gc = 0.0, a_bc = 0.0, a_gu = 0.0, a_gw = 0.0, a_z = 0.0, a_n = 0.0;
  if (j < H) {
    const double Bf = (double)B;
    for (int t = 0; t < T; ++t) {
      const FrameUnit f = frame_unit(stats + (size_t)t * BNT_KS * H, H, j, k);
      const double* r = red + (size_t)t * BNT_KB * H;
      const double ag = f.gg * f.ig, ac = f.gc * f.ic;
      const double kc = (ag * f.ig * f.ig * r[2 * H + j] + ac * f.ic * f.ic * r[3 * H + j]) / Bf;
      const double dnu = f.dnu, dnw = f.dnw;
      a_gg += r[2 * H + j] * f.ig;
      a_bg += r[j];
      a_gc += r[3 * H + j] * f.ic;
      a_bc += r[H + j];
      a_gu += ag * r[4 * H + j] + ac * r[5 * H + j] - kc * Bf * dnu;
      a_gw += ag * r[6 * H + j] + ac * r[7 * H + j] - kc * Bf * dnw;
      a_z += r[8 * H + j];
      a_n += r[9 * H + j];
    }
    o.dgg[j] = (float)a_gg;
    o.dbg[j] = (float)a_bg;
    o.dgc[j] = (float)a_gc;
    o.dbc[j] = (float)a_bc;
    o.dgu[j] = (float)a_gu;
    o.dgw[j] = (float)a_gw;
    // beta_w, beta_u, bias_gate and bias_update shift the input of a batch-normalised layer: zero gradient
    o.dbw[j] = 0.f;
    o.dbu[j] = 0.f;
    o.dbias_gate[j] = 0.f;
    o.dbias_update[j] = 0.f;
  }
  sz[j] = a_z;
  sn[j] = a_n;
  __syncthreads();
  if (j == 0) {
    double z = 0.0, n = 0.0;
    for (int q = 0; q < H; ++q) {
      z += sz[q];
      n += sn[q];
    }
    const double zsg = sigm(k.zeta[0]), nsg = sigm(k.nu[0]);
    o.dzeta[0] = (float)(z * zsg * (1.0 - zsg));
    o.dnu[0] = (float)(n * nsg * (1.0 - nsg));
  }
}

struct Layout {
  int rpw, nwg, RG;
};

Layout layout(int B, int H) {
  const int chunks = (B + BNT_CHUNK - 1) / BNT_CHUNK;
  const int per = (chunks + BNT_MAX_WG - 1) / BNT_MAX_WG;
  Layout l;
  l.rpw = per * BNT_CHUNK;
  l.nwg = (B + l.rpw - 1) / l.rpw;
  l.RG = BNT_THREADS / H;
  return l;
}

BnConst make_const(const fastgrnn_bn_params& bn, const fastgrnn_params& p) {
  BnConst k;
  k.gw = (const float*)bn.w.gamma;
  k.bw = (const float*)bn.w.beta;
  k.gu = (const float*)bn.u.gamma;
  k.bu = (const float*)bn.u.beta;
  k.gg = (const float*)bn.gate.gamma;
  k.bg = (const float*)bn.gate.beta;
  k.gc = (const float*)bn.update.gamma;
  k.bc = (const float*)bn.update.beta;
  k.ew = (float)bn.w.eps;
  k.eu = (float)bn.u.eps;
  k.eg = (float)bn.gate.eps;
  k.ec = (float)bn.update.eps;
  k.zeta = (const float*)p.zeta;
  k.nu = (const float*)p.nu;
  return k;
}

int frame_product(const fastgrnn_desc& d, const void* x, const float* w, float* wc, hipStream_t s) {
  const size_t R = (size_t)d.T * d.B;
  if (d.F == 32) {
    const dim3 grid((unsigned)((R + BNT_CHUNK - 1) / BNT_CHUNK));
    if (d.H == 128) hipLaunchKernelGGL(bnt_frame_f32<128>, grid, dim3(256), 0, s, R, (const float*)x, w, wc);
    else hipLaunchKernelGGL(bnt_frame_f32<256>, grid, dim3(256), 0, s, R, (const float*)x, w, wc);
    return launch_status();
  }
  return rows_gemm(R, d.H, d.F, false, x, w, wc, false, false, s);
}

struct FwdWs {
  float *ut, *wc;
  double* part;
  unsigned* cnt;
  size_t bytes;
};

FwdWs fwd_ws(const fastgrnn_desc& d, void* base) {
  const Layout l = layout(d.B, d.H);
  Carve c(base);
  FwdWs w;
  w.ut = c.take<float>((size_t)d.H * d.H);
  w.wc = c.take<float>((size_t)d.T * d.B * d.H);
  w.part = c.take<double>((size_t)l.nwg * l.RG * BNT_KF * d.H);
  w.cnt = c.take<unsigned>(2 * (size_t)d.T);             // bnt_fwd_step's T counters, then bnt_fwd_sstat's
  w.bytes = c.off;
  return w;
}

struct BwdWs {
  float *wc, *duc, *dwc, *dpg, *dpu, *dhz, *gpart;
  double *part, *red;
  unsigned* cnt;
  size_t bytes;
};

BwdWs bwd_ws(const fastgrnn_desc& d, void* base) {
  const Layout l = layout(d.B, d.H);
  const bool bm = (d.flags & FASTGRNN_FLAG_BATCH_MAJOR) != 0;
  const size_t R = (size_t)d.T * d.B, Ru = bm ? R + d.B : R, BH = (size_t)d.B * d.H;
  const size_t g1 = tn_gemm_big_ws(Ru, d.H, d.H), g2 = tn_gemm_big_ws(R, d.H, d.F);
  Carve c(base);
  BwdWs w;
  w.wc = c.take<float>(R * d.H);
  w.duc = c.take<float>(Ru * d.H);
  w.dwc = c.take<float>(R * d.H);
  w.dpg = c.take<float>(BH);
  w.dpu = c.take<float>(BH);
  w.dhz = c.take<float>(BH);
  w.part = c.take<double>((size_t)l.nwg * l.RG * BNT_KB * d.H);
  w.red = c.take<double>((size_t)d.T * BNT_KB * d.H);
  w.gpart = c.take<float>((g1 > g2 ? g1 : g2) / sizeof(float) + 1);
  w.cnt = c.take<unsigned>((size_t)d.T + 1);
  w.bytes = c.off;
  return w;
}

}  // namespace

bool bn_train_supported(const fastgrnn_desc& d) {
  if (d.dtype != FASTGRNN_F32 || d.w_rank || d.u_rank || d.B < 2) return false;
  if (d.gate_nl < FASTGRNN_NL_SIGMOID || d.gate_nl > FASTGRNN_NL_TANH || d.update_nl != FASTGRNN_NL_TANH) return false;
  if (d.flags & ~(FASTGRNN_FLAG_BN_TRAIN | FASTGRNN_FLAG_BATCH_MAJOR)) return false;
  if (d.H == 128) return d.F == 32 || d.F == 64 || d.F == 128 || d.F == 256;
  if (d.H == 256) return d.F == 32 || d.F == 64 || d.F == 128;
  return false;
}

size_t bn_train_forward_ws(const fastgrnn_desc& d) { return fwd_ws(d, nullptr).bytes; }
size_t bn_train_backward_ws(const fastgrnn_desc& d) { return bwd_ws(d, nullptr).bytes; }

int bn_train_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const fastgrnn_bn_params& bn, const void* x,
                     const void* h0, void* hs, void* saved, void* stats, void* ws, hipStream_t s) {
  const FwdWs w = fwd_ws(d, ws);
  const Layout l = layout(d.B, d.H);
  const bool bm = (d.flags & FASTGRNN_FLAG_BATCH_MAJOR) != 0;
  const BnConst k = make_const(bn, p);
  double* st = (double*)stats;
  if (hipMemsetAsync(w.cnt, 0, 2 * (size_t)d.T * sizeof(unsigned), s) != hipSuccess) return FASTGRNN_ERR_LAUNCH;
  hipLaunchKernelGGL(bnt_transpose, dim3((unsigned)(((size_t)d.H * d.H + 255) / 256)), dim3(256), 0, s, d.H,
                     (const float*)p.u, w.ut);
  int r = frame_product(d, x, (const float*)p.w, w.wc, s);
  if (r) return r;
  hipLaunchKernelGGL(bnt_wstats, dim3(d.T, d.H / 64), dim3(256), 0, s, d.T, d.B, d.H, bm, (const float*)w.wc, st);
  for (int t = 0; t <= d.T; ++t) {
    if (d.H == 128)
      hipLaunchKernelGGL(bnt_fwd_step<128>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm,
                         d.gate_nl, k, (const float*)w.wc, (const float*)w.ut, (const float*)h0, (float*)hs,
                         (float*)saved, st, w.part, w.cnt);
    else
      hipLaunchKernelGGL(bnt_fwd_step<256>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm,
                         d.gate_nl, k, (const float*)w.wc, (const float*)w.ut, (const float*)h0, (float*)hs,
                         (float*)saved, st, w.part, w.cnt);
    if (t == d.T) break;
    if (d.H == 128)
      hipLaunchKernelGGL(bnt_fwd_sstat<128>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm, k,
                         (const float*)w.wc, (const float*)saved, st, w.part, w.cnt + d.T);
    else
      hipLaunchKernelGGL(bnt_fwd_sstat<256>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm, k,
                         (const float*)w.wc, (const float*)saved, st, w.part, w.cnt + d.T);
  }
  RunStat rs;
  const fastgrnn_bn_layer* layers[4] = {&bn.w, &bn.u, &bn.gate, &bn.update};
  for (int q = 0; q < 4; ++q) {
    rs.mean[q] = (float*)layers[q]->running_mean;
    rs.var[q] = (float*)layers[q]->running_var;
    rs.nbt[q] = layers[q]->num_batches_tracked;
    rs.mom[q] = layers[q]->momentum < 0 ? -1.0f : (float)layers[q]->momentum;
  }
  hipLaunchKernelGGL(bnt_running, dim3(4), dim3(d.H), 0, s, d.T, d.B, d.H, k, (const float*)p.bias_gate,
                     (const float*)p.bias_update, (const double*)st, rs);
  return launch_status();
}

int bn_train_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const fastgrnn_bn_params& bn,
                      const void* ghs, const void* x, const void* hs, const void* saved, const void* stats,
                      const void* h0, const fastgrnn_grads& g, const fastgrnn_bn_grads& bg, void* ws, hipStream_t s) {
  const BwdWs w = bwd_ws(d, ws);
  const Layout l = layout(d.B, d.H);
  const bool bm = (d.flags & FASTGRNN_FLAG_BATCH_MAJOR) != 0;
  const BnConst k = make_const(bn, p);
  const double* st = (const double*)stats;
  const size_t R = (size_t)d.T * d.B;
  if (hipMemsetAsync(w.cnt, 0, ((size_t)d.T + 1) * sizeof(unsigned), s) != hipSuccess) return FASTGRNN_ERR_LAUNCH;
  int r = frame_product(d, x, (const float*)p.w, w.wc, s);
  if (r) return r;
  for (int t = d.T - 1; t >= -1; --t) {
    if (d.H == 128)
      hipLaunchKernelGGL(bnt_bwd_step<128>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm,
                         d.gate_nl, k, (const float*)w.wc, (const float*)p.u, (const float*)h0, (const float*)hs,
                         (const float*)ghs, (const float*)saved, st, w.dpg, w.dpu, w.dhz, w.duc, w.dwc, w.red, w.part,
                         w.cnt, (float*)g.d_h0);
    else
      hipLaunchKernelGGL(bnt_bwd_step<256>, dim3(l.nwg), dim3(BNT_THREADS), 0, s, t, d.T, d.B, l.rpw, l.nwg, bm,
                         d.gate_nl, k, (const float*)w.wc, (const float*)p.u, (const float*)h0, (const float*)hs,
                         (const float*)ghs, (const float*)saved, st, w.dpg, w.dpu, w.dhz, w.duc, w.dwc, w.red, w.part,
                         w.cnt, (float*)g.d_h0);
  }
  BnGradOut o{(float*)bg.d_gamma_w, (float*)bg.d_beta_w, (float*)bg.d_gamma_u, (float*)bg.d_beta_u,
              (float*)bg.d_gamma_gate, (float*)bg.d_beta_gate, (float*)bg.d_gamma_update, (float*)bg.d_beta_update,
              (float*)g.d_bias_gate, (float*)g.d_bias_update, (float*)g.d_zeta, (float*)g.d_nu};
  hipLaunchKernelGGL(bnt_param_grads, dim3(1), dim3(256), 0, s, d.T, d.B, d.H, k, st, (const double*)w.red, o);
  // d_u[j][k] = sum over frames and rows of d uC[j] . h_prev[k]
  const size_t Ru = bm ? R + d.B : R;
  if ((r = tn_gemm_big_run(Ru, d.H, d.H, w.duc, d.H, (const float*)h0, hs, (size_t)d.B, d.H, w.gpart,
                           (float*)g.d_u, d.H, s)))
    return r;
  // d_w[j][f] = sum d wC[j] . x[f];  d_x = d wC . w
  if ((r = dpre_bwd_tail(d, w.dwc, w.gpart, nullptr, x, p.w, g, s))) return r;
  return launch_status();
}

}  // namespace fastgrnn
