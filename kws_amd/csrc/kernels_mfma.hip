// MFMA-tiled fp32 FastGRNN scan for gfx950 (dense W/U, tanh update, sigmoid/relu/tanh gate).
//
// Geometry.  One workgroup = 4 waves = one tile of 16 utterances for ALL T frames.  The
// recurrent product is evaluated transposed, D[n][b] = sum_k U[n][k] h[b][k], with
// v_mfma_f32_16x16x4_f32 (exact fp32 fma chain): the 16 utterances sit on the MFMA's N
// (lane&15) axis, hidden units on M.  Wave w owns the H/4 hidden units
//     n_own(g,mt,r) = w*H/4 + g*4*MT + mt*4 + r        (g = lane>>4, MT = H/64 tiles, r = reg)
// so a lane's 4*MT results are CONTIGUOUS in memory (float4 stores of hs/z/c; four
// lane groups cover one 128-B line per utterance).  The A operands (slices of U, W, or
// of their transposes in the backward) are loaded ONCE into VGPRs and stay there for
// the whole scan: U is never re-read from LDS or HBM.  Per step only the 16 x H state
// tile crosses waves, through an 8 KB LDS image [k/4][b] of float4 that is written with
// ds_write_b128 and read back, conflict-free, as the next step's B operand.
//
// The K index of every product is permuted (k = 16q + 4g + r for MFMA step 4q+r) so that
// the B operand of a lane is 4 contiguous floats per q; A is loaded with the same
// permutation, which leaves the sum unchanged.
//
// Backward additionally keeps the per-workgroup dW/dU partial sums in accumulator VGPRs
// across all T steps (d_pre^T . [x | h_prev] with K = the 16 utterances) and flushes them
// once; a tiny second kernel reduces the per-workgroup slabs deterministically.
//
// Reference semantics: forward .cu:42-60 + .cu:367-413; backward .cu:91-119 + .cu:473-545.
#include "scan_common.h"
#include "variant_pick.h"

namespace fastgrnn {
namespace {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// SCHED_PIN(idx): scheduling-region boundary.  Measured: with these pins hipcc keeps the
// load requests, the dependent MFMA chain and the VALU/MFMA overlap region in the order
// written, which is 20-25 % faster than its free schedule.  DIAG bit 32 removes the pins
// (A/B), bit 16 additionally reads s_memtime there (diagnostic build only).
#ifdef FASTGRNN_DIAG_STAMPS
__device__ unsigned long long g_diag[4][16];
#define SCHED_PIN(idx)                                                                    \
  if (DIAG & 16) {                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    unsigned long long now_;                                                              \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");          \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    dsum[idx] += now_ - dlast; dlast = now_;                                              \
  } else if (!(DIAG & 32)) {                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  }
#else
#define SCHED_PIN(idx) if (!(DIAG & 32)) { __builtin_amdgcn_sched_barrier(0); }
#endif

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// Step anatomy (one barrier per step; everything else is one basic block so that the
// scheduler can interleave freely):
//   top     request x_{t+1}; read the state tile h_{t-1} from LDS; 2*KX/… W.x_t MFMAs (they do
//           not depend on h, so they cover the LDS round trip)
//   chain   MT x H/4 dependent MFMAs U.h_{t-1}; the global stores of step t-1 (hs, z, c) are
//           issued here, spread under the chain instead of in a burst in front of the barrier
//   tail    gate/candidate/update on the VALU, new state tile to LDS, barrier
// GATES_OUT: also write z_s / c_s (the reference operator's outputs).  RAGGED: B % 16 != 0
// (stores are lane-predicated; kept out of the full-tile build so it has no branches).
// DIAG (tools/diag_scan.hip only; production instantiates 0): 1 = no global stores,
// 2 = no per-step barrier, 4 = cheap epilogue, 8 = no recurrent-chain MFMAs, 16 = cycle
// stamps.  Ablations for timing; their results are wrong by construction.
// The instantiations the library holds (shapes: shape_ok): every GATES_OUT and RAGGED of the reference's three gates.
constexpr bool fwd_mfma_built(int gate) { return gate <= FASTGRNN_NL_TANH; }
template <int H, int F, int GATE, bool GATES_OUT, bool RAGGED, int DIAG = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void fwd_scan_mfma(
    int Tn, int B, const float* __restrict__ x, const float* __restrict__ h0,
    const float* __restrict__ w, const float* __restrict__ u,
    const float* __restrict__ bz, const float* __restrict__ bh,
    const float* __restrict__ zeta, const float* __restrict__ nu,
    float* __restrict__ hs, float* __restrict__ zs, float* __restrict__ cs) {
  constexpr int HS = H / 4;        // hidden units per wave
  constexpr int MT = HS / 16;      // 16-row MFMA tiles per wave
  constexpr int KH = H / 4;        // MFMA steps over the hidden dim
  constexpr int KX = F / 4;        // MFMA steps over the feature dim
  constexpr int NQ = H / 16;
  static_assert(H % 64 == 0 && F % 16 == 0, "tile shape");
  __shared__ f32x4 hl[2][(H / 4) * 16];   // state tile, [k/4][b] float4, double-buffered

  const int tid = threadIdx.x;
  const int wv = tid >> 6, l = tid & 63, i = l & 15, g = l >> 4;
  const int b = blockIdx.x * 16 + i;
  const bool valid = !RAGGED || b < B;
  const int bc = valid ? b : B - 1;                 // clamped row for loads
  const int n0 = wv * HS + g * (4 * MT);            // first of this lane's 4*MT hidden units

  // ---- resident A operands -----------------------------------------------------------------
  float Uf[MT][KH], Wf[MT][KX];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int nA = wv * HS + (i >> 2) * (4 * MT) + mt * 4 + (i & 3);   // A row i of tile mt
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      f32x4 v = ld4(u + (size_t)nA * H + 16 * q + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) Uf[mt][4 * q + r] = v[r];
    }
#pragma unroll
    for (int kq = 0; kq < KX / 4; ++kq) {
      f32x4 v = ld4(w + (size_t)nA * F + g * KX + 4 * kq);
#pragma unroll
      for (int r = 0; r < 4; ++r) Wf[mt][4 * kq + r] = v[r];
    }
  }
  f32x4 bzv[MT], bhv[MT], hown[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    bzv[mt] = ld4(bz + n0 + 4 * mt);
    bhv[mt] = ld4(bh + n0 + 4 * mt);
    hown[mt] = ld4(h0 + (size_t)bc * H + n0 + 4 * mt);
    hl[0][(wv * (HS / 4) + g * MT + mt) * 16 + i] = hown[mt];
  }
  const float sz = fsigmoid(zeta[0]), sn = fsigmoid(nu[0]);

  struct Feat { f32x4 v[KX / 4]; };       // one frame's features for this lane
  struct Gates { f32x4 z[MT], c[MT]; };   // z_t, c_t awaiting their store
  auto load_x = [&](int t, Feat& q) __attribute__((always_inline)) {
    const float* xp = x + ((size_t)t * B + bc) * F + g * KX;
#pragma unroll
    for (int kq = 0; kq < KX / 4; ++kq) q.v[kq] = ld4(xp + 4 * kq);
  };
  auto store_step = [&](int t, const Gates& gt) __attribute__((always_inline)) {     // hown still holds h_t here
    if (DIAG & 1) return;
    if (valid) {
      const size_t o = ((size_t)t * B + b) * H + n0;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) st4(hs + o + 4 * mt, hown[mt]);
      if (GATES_OUT) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { st4(zs + o + 4 * mt, gt.z[mt]); st4(cs + o + 4 * mt, gt.c[mt]); }
      }
    }
  };

#ifdef FASTGRNN_DIAG_STAMPS
  unsigned long long dsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dlast = 0;
  if (DIAG & 16) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dlast)::"memory"); }
#endif
  // Two register sets alternate between consecutive steps (features, gates), so that no
  // copy -- and hence no wait for a load -- sits at a step boundary.
  auto step = [&](auto first_tag, int t, int cur, Feat& xuse, Feat& xload, Gates& gprev, Gates& gout) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_tag)::value;
    load_x(t + 1 < Tn ? t + 1 : t, xload);            // clamped: the tail load is unused
    float hB[KH];                                      // B operand: the whole state tile h_{t-1}
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      f32x4 v = hl[cur][(4 * q + g) * 16 + i];
#pragma unroll
      for (int r = 0; r < 4; ++r) hB[4 * q + r] = v[r];
    }
    // the state reads are issued before the first MFMA: each gets registers of its own (left alone the compiler
    // issues W.x first and lands them in the feature registers those MFMAs read; operand rule)
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KX; ++kk)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma4(Wf[mt][kk], xuse.v[kk >> 2][kk & 3], acc[mt]);
    SCHED_PIN(0)   // x request + LDS state read + W.x MFMAs issued
    if (!FIRST) store_step(t - 1, gprev);
    if (!(DIAG & 8)) {
#pragma unroll
      for (int kk = 0; kk < KH; ++kk)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma4(Uf[mt][kk], hB[kk], acc[mt]);   // .cu:368
    } else {
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) acc[kk % MT][kk & 3] += Uf[kk % MT][kk] * hB[kk];
    }
    if (!FIRST && !(DIAG & (1 | 8 | 64))) {
      // spread the NST store instructions of step t-1 evenly under the MT*KH chain MFMAs
      constexpr int NST = GATES_OUT ? 3 * MT : MT;
      constexpr int PER = (MT * KH) / (NST + 1);
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);     // VMEM write
      }
      __builtin_amdgcn_sched_group_barrier(0x008, MT * KH - NST * PER, 0);
    }
    SCHED_PIN(1)   // stores of step t-1 + recurrent chain issued
    // epilogue (.cu:55-58)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pre = acc[mt][r];
        const float z = (DIAG & 4) ? pre * bzv[mt][r] : gate_act<GATE>(pre + bzv[mt][r]);
        const float c = (DIAG & 4) ? pre * bhv[mt][r] : ftanh(pre + bhv[mt][r]);
        hown[mt][r] = (sz * (1.0f - z) + sn) * c + hown[mt][r] * z;
        gout.z[mt][r] = z; gout.c[mt][r] = c;
      }
      hl[cur ^ 1][(wv * (HS / 4) + g * MT + mt) * 16 + i] = hown[mt];
    }
    SCHED_PIN(2)   // epilogue + LDS write issued
    if (!(DIAG & 2)) lds_barrier();
    SCHED_PIN(3)   // barrier passed
  };

  Feat xa, xb;
  Gates ga, gb;
  load_x(0, xa);
  __syncthreads();
  step(std::true_type{}, 0, 0, xa, xb, gb, ga);
  int t = 1;
  for (; t + 1 < Tn; t += 2) {
    step(std::false_type{}, t, 1, xb, xa, ga, gb);
    step(std::false_type{}, t + 1, 0, xa, xb, gb, ga);
  }
  if (t < Tn) {                       // Tn even: one more step, parity 1
    step(std::false_type{}, t, 1, xb, xa, ga, gb);
    store_step(Tn - 1, gb);
  } else {
    store_step(Tn - 1, ga);
  }
  // The weight registers stay allocated through the last step (its state reads would otherwise be streamed
  // through them, right behind the MFMAs that read them).  hown comes from the last accumulators: retired.
  {
    float tie = hown[0][0];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int kk = 0; kk < KH; kk += 8)
        asm volatile("" : "+v"(tie) : "v"(Uf[mt][kk]), "v"(Uf[mt][kk + 1]), "v"(Uf[mt][kk + 2]), "v"(Uf[mt][kk + 3]),
                     "v"(Uf[mt][kk + 4]), "v"(Uf[mt][kk + 5]), "v"(Uf[mt][kk + 6]), "v"(Uf[mt][kk + 7]));
#pragma unroll
      for (int kk = 0; kk < KX; kk += 4)
        asm volatile("" : "+v"(tie) : "v"(Wf[mt][kk]), "v"(Wf[mt][kk + 1]), "v"(Wf[mt][kk + 2]), "v"(Wf[mt][kk + 3]));
    }
  }
#ifdef FASTGRNN_DIAG_STAMPS
  if ((DIAG & 16) && blockIdx.x == 7 && l == 0) {
    for (int k = 0; k < 8; ++k) g_diag[wv][k] = dsum[k];
  }
#endif
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// floats per workgroup slab of backward partial sums, padded to 64
__host__ __device__ constexpr int slab_stride(int H, int F) { return (H * H + H * F + 2 * H + 2 + 63) & ~63; }

template <int H, int F>
struct BwdLds {
  static constexpr int HS = H / 4;
  f32x4 P[2][(H / 4) * 16];          // d_pre tile, [n/4][b] float4   (B operand of d_h, d_x)
  float Tt[2][4][HS][20];            // d_pre^T per wave, [n_local][b] (A operand of dW, dU)
  float Hp[2][16][H + 4];            // h_prev tile, [b][k]            (B operand of dU)
  f32x4 DX[2][4][F / 16][64];        // d_x partial sums of every wave, per feature tile
  float red[8];
};

// Reverse scan, software-pipelined over two steps.  Per step t and per wave:
//   MM(t)  64 dependent MFMAs  d_h = z*g + U^T d_pre_t          (the serial chain)
//          96 independent MFMAs d_x partial, dW += d_pre_t^T x_t, dU += d_pre_t^T h_{t-1}
//   EW(t)  gate/candidate derivatives on the VALU -> d_pre_t, published through LDS
// Iteration t runs [chain(t)] then [off-chain MM(t) || EW(t-1)] in ONE basic block, so the
// matrix pipe works on the 96 independent MFMAs while the VALU prepares the next step's
// d_pre; one raw s_barrier per step.  Global operands are requested one iteration before
// their use into alternating register sets (no copies, no early waits).
// The instantiations the library holds (shapes: shape_ok).  No ragged-batch one for H = 128: it needs more registers
// than a wave has (F = 64) or spills inside the loop (F = 32), and spill reloads are loads nobody placed (operand rule,
// DESIGN.md 4.0; tools/war_scan.py rejects both); mfma_supported() sends that case on -- in practice only under
// FASTGRNN_FLAG_FORCE_F32_MFMA, the split-precision kernels take these shapes first.
constexpr bool bwd_mfma_built(int h, int gate, bool ragged) { return gate <= FASTGRNN_NL_TANH && !(h == 128 && ragged); }
template <int H, int F, int GATE, bool RAGGED, int DIAG = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void bwd_scan_mfma(
    int Tn, int B, const float* __restrict__ ghs, const float* __restrict__ x,
    const float* __restrict__ hs, const float* __restrict__ zs, const float* __restrict__ cs,
    const float* __restrict__ h0, const float* __restrict__ w, const float* __restrict__ u,
    const float* __restrict__ zeta, const float* __restrict__ nu,
    float* __restrict__ d_x, float* __restrict__ d_h0,
    float* __restrict__ part)      // [nwg][slab_stride(H,F)]: dU | dW | d_bz | d_bh | (d_zeta, d_nu) sums
{
  constexpr int HS = H / 4, MT = HS / 16, KH = H / 4, NQ = H / 16;
  constexpr int NCT = H / 16;      // column tiles of dU
  constexpr int NFT = F / 16;      // feature tiles (d_x rows, dW columns)
  constexpr int KD = 4 * MT;       // MFMA steps of this wave's d_x partial (K = its own hidden slice)
  static_assert(NFT >= 1 && NFT <= 4, "F must be 16..64");
  __shared__ BwdLds<H, F> S;

  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63, i = l & 15, g = l >> 4;
  const int b = blockIdx.x * 16 + i;
  const bool valid = !RAGGED || b < B;
  const int bc = valid ? b : B - 1;
  const int n0 = wv * HS + g * (4 * MT);
  const float sz = fsigmoid(zeta[0]), sn = fsigmoid(nu[0]);

  // ---- resident A operands -----------------------------------------------------------------
  // d_h[k][b] = sum_n U[n][k] d_pre[b][n]:  A row i of tile mt is k = wv*HS + (i>>2)*4MT + mt*4 + (i&3)
  float UTf[MT][KH];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int kA = wv * HS + (i >> 2) * (4 * MT) + mt * 4 + (i & 3);
#pragma unroll
    for (int kk = 0; kk < KH; ++kk) {
      const int n = 16 * (kk >> 2) + 4 * g + (kk & 3);
      UTf[mt][kk] = u[(size_t)n * H + kA];
    }
  }
  // d_x[f][b] = sum_n W[n][f] d_pre[b][n]: every wave contracts over ITS OWN hidden slice, with
  // the B operand taken straight from its d_pre registers (MFMA step 4mt+r <-> n = n0+4mt+r);
  // the four partial sums meet in LDS.
  float WTf[NFT][KD];
#pragma unroll
  for (int f2 = 0; f2 < NFT; ++f2)
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) WTf[f2][kk] = w[(size_t)(n0 + kk) * F + f2 * 16 + i];

  f32x4 accU[MT][NCT], accW[MT][NFT];
#pragma unroll
  for (int a = 0; a < MT; ++a) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) accU[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NFT; ++c) accW[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 sbz[MT], sbh[MT], dh[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    sbz[mt] = f32x4{0.f, 0.f, 0.f, 0.f}; sbh[mt] = sbz[mt]; dh[mt] = sbz[mt];
  }
  float pz = 0.f, pn = 0.f;

  struct EwOps { f32x4 g[MT], z[MT], c[MT], h[MT]; };   // operands of EW(t)
  struct XT { float v[NFT][4]; };                        // x_t^T fragments for dW
  auto load_ew = [&](int t, EwOps& q) __attribute__((always_inline)) {
    const size_t o = ((size_t)t * B + bc) * H + n0;
    const float* hprev = (t == 0) ? h0 + (size_t)bc * H + n0 : hs + o - (size_t)B * H;   // .cu:478-481
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      q.g[mt] = ld4(ghs + o + 4 * mt);
      q.z[mt] = ld4(zs + o + 4 * mt);
      q.c[mt] = ld4(cs + o + 4 * mt);
      q.h[mt] = ld4(hprev + 4 * mt);
    }
  };
  auto load_xt = [&](int t, XT& q) __attribute__((always_inline)) {   // B[k = utterance 4g+kk][j = i]: feature i*NFT + f2
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int bb = blockIdx.x * 16 + 4 * g + kk;
      const float* xp = x + ((size_t)t * B + ((!RAGGED || bb < B) ? bb : B - 1)) * F + i * NFT;
      if (NFT == 2) {
        const float2 v = *reinterpret_cast<const float2*>(xp);        // rows past B multiply d_pre = 0
        q.v[0][kk] = v.x; q.v[1][kk] = v.y;
      } else if (NFT == 4) {
        const f32x4 v = ld4(xp);
#pragma unroll
        for (int f2 = 0; f2 < NFT; ++f2) q.v[f2][kk] = v[f2];
      } else {
#pragma unroll
        for (int f2 = 0; f2 < NFT; ++f2) q.v[f2][kk] = xp[f2];
      }
    }
  };

  // EW(t): .cu:107-117, in NR = 4 chunks of MT elements so that each chunk can share a pinned
  // scheduling region with a batch of independent MFMAs.  Consumes dh = d_old_h from
  // chain(t+1) and leaves dh = z*g, the C-in of chain(t).
  struct EwOut { f32x4 dp[MT], hp[MT]; };
  auto ew_chunk = [&](int j, const EwOps& q, EwOut& o) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      const int e = j * MT + k, mt = e >> 2, r = e & 3;
      const float gg = q.g[mt][r] + dh[mt][r];                                   // .cu:474
      const float z = q.z[mt][r], c = q.c[mt][r];
      float hv = q.h[mt][r];
      float dcp = (sz * (1.0f - z) + sn) * (1.0f - c * c) * gg;                  // .cu:109
      float dzp = (hv - sz * c) * gate_dact<GATE>(z) * gg;                       // .cu:110
      float zg = z * gg;                                                          // .cu:108
      float tz = (1.0f - z) * c * gg, tn = c * gg;                                // .cu:114-115
      if (RAGGED && !valid) { dcp = 0.f; dzp = 0.f; zg = 0.f; tz = 0.f; tn = 0.f; hv = 0.f; }
      sbz[mt][r] += dzp; sbh[mt][r] += dcp; pz += tz; pn += tn;
      o.dp[mt][r] = dzp + dcp;                                                    // .cu:113
      o.hp[mt][r] = hv;
      dh[mt][r] = zg;
    }
  };
  // publish d_pre_t / h_{t-1} in LDS buffers [t&1]; keep d_pre_t in registers for d_x
  auto ew_publish = [&](int t, const EwOut& o, f32x4 (&dpo)[MT]) __attribute__((always_inline)) {
    const int buf = t & 1;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      S.P[buf][(wv * (HS / 4) + g * MT + mt) * 16 + i] = o.dp[mt];
      *reinterpret_cast<f32x4*>(&S.Hp[buf][i][n0 + 4 * mt]) = o.hp[mt];
#pragma unroll
      for (int r = 0; r < 4; ++r) S.Tt[buf][wv][g * (4 * MT) + mt * 4 + r][i] = o.dp[mt][r];
      dpo[mt] = o.dp[mt];
    }
  };
  // d_x partial of step t over this wave's hidden slice (.cu:538): register operands only
  auto dx_partial = [&](int t, const f32x4 (&dpo)[MT]) __attribute__((always_inline)) {
    f32x4 accx[NFT];
#pragma unroll
    for (int f2 = 0; f2 < NFT; ++f2) accx[f2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f2 = 0; f2 < NFT; ++f2) accx[f2] = mfma4(WTf[f2][4 * mt + r], dpo[mt][r], accx[f2]);
#pragma unroll
    for (int f2 = 0; f2 < NFT; ++f2) S.DX[t & 1][wv][f2][l] = accx[f2];
  };
  // d_x of step t = sum of the four waves' partials; wave f2 < NFT finishes feature tile f2.
  auto finish_dx = [&](int t) __attribute__((always_inline)) {
    if (wv < NFT) {                         // wave-uniform (wv is an SGPR)
      f32x4 sacc = (S.DX[t & 1][0][wv][l] + S.DX[t & 1][1][wv][l]) + (S.DX[t & 1][2][wv][l] + S.DX[t & 1][3][wv][l]);
      if (valid) st4(d_x + ((size_t)t * B + b) * F + wv * 16 + 4 * g, sacc);
    }
  };

#ifdef FASTGRNN_DIAG_STAMPS
  unsigned long long dsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dlast = 0;
  if (DIAG & 16) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dlast)::"memory"); }
#endif

  // One pipelined iteration.  dpo holds d_pre_{t+1} on entry (B operand of d_x(t+1)) and
  // receives d_pre_{t-1} at the end.
  //   top    LDS reads for chain(t); the 8*NFT register-only d_x(t+1) MFMAs cover their latency
  //   chain  64 dependent MFMAs; the global operand requests are issued in their shadow
  //   4 x    { dW/dU MFMAs of step t  ||  one chunk of EW(t-1) }   (pinned regions)
  //   end    publish d_pre_{t-1}; barrier
  auto iter = [&](auto last_tag, int t, f32x4 (&dpo)[MT], const EwOps& eo, EwOps& e_load, const XT& xo,
                  XT& x_load) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last_tag)::value;
    const int buf = t & 1;
    // ---- operands from LDS ------------------------------------------------------------------
    float dpB[KH];
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
      f32x4 v = S.P[buf][(4 * qq + g) * 16 + i];
#pragma unroll
      for (int r = 0; r < 4; ++r) dpB[4 * qq + r] = v[r];
    }
    f32x4 dpT[MT];
#pragma unroll
    for (int a2 = 0; a2 < MT; ++a2) dpT[a2] = *reinterpret_cast<const f32x4*>(&S.Tt[buf][wv][a2 * 16 + i][4 * g]);
    __builtin_amdgcn_sched_barrier(0);   // every LDS read of the phase is issued before its first MFMA
    if (t + 1 < Tn) dx_partial(t + 1, dpo);
    SCHED_PIN(0)   // LDS reads + d_x(t+1) MFMAs
    // ---- d_h chain (.cu:537): C-in = z*g --------------------------------------------------
#pragma unroll
    for (int kk = 0; kk < KH; ++kk)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) dh[mt] = mfma4(UTf[mt][kk], dpB[kk], dh[mt]);
    SCHED_PIN(1)   // chain issued
    {
      // dh read = the chain has retired: the h rows requested next may reuse its B registers
      float touch = 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) touch += dh[mt][0];
      completion_read(touch);
      __builtin_amdgcn_sched_barrier(0);
    }
    // Operands of EW(t-2) and of dW(t-1) are requested here, a whole iteration before their use (eo / xo were
    // requested during iteration t+1), into the alternate register set -- AFTER the chain has retired: spread
    // through the chain's shadow (as this kernel first had them) the compiler lands them in the chain's own B
    // registers as those die, right behind the MFMAs that read them.  Now those registers are
    // free for them, and the four regions below cover the latency.
    lds_writes_landed();                   // (second rule of DESIGN.md 4.0: conditional requests and stores follow)
    if (!LAST) {
      load_xt(t - 1, x_load);
      load_ew(t >= 2 ? t - 2 : 0, e_load);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < Tn) finish_dx(t + 2);      // published at the top of the previous iteration
    // ---- dW (.cu:539), dU (.cu:540) with K = the 16 utterances, overlapped with EW(t-1) --------
    EwOut eo_out;
    // Region j = MFMA K-step j (utterances 4g+j): B operands are row 4g+j of the h_prev tile,
    // NCT contiguous floats per lane (dU column of tile c2, lane i is i*NCT + c2), read one
    // region ahead so that no MFMA waits on LDS latency.
    f32x4 hrow[2][NCT / 4];
    auto read_hrow = [&](int j, f32x4 (&dst)[NCT / 4]) __attribute__((always_inline)) {
#pragma unroll
      for (int v = 0; v < NCT / 4; ++v) dst[v] = *reinterpret_cast<const f32x4*>(&S.Hp[buf][4 * g + j][i * NCT + 4 * v]);
    };
    read_hrow(0, hrow[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j + 1 < 4) read_hrow(j + 1, hrow[(j + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);   // issued before this region's MFMAs: registers of its own
#pragma unroll
      for (int a2 = 0; a2 < MT; ++a2)
#pragma unroll
        for (int f2 = 0; f2 < NFT; ++f2) accW[a2][f2] = mfma4(dpT[a2][j], xo.v[f2][j], accW[a2][f2]);
#pragma unroll
      for (int c2 = 0; c2 < NCT; ++c2)
#pragma unroll
        for (int a2 = 0; a2 < MT; ++a2) accU[a2][c2] = mfma4(dpT[a2][j], hrow[j & 1][c2 >> 2][c2 & 3], accU[a2][c2]);
      if (!LAST) ew_chunk(j, eo, eo_out);
      if (!LAST && !(DIAG & 128)) {
        // fine interleave: the VALU work of the chunk goes between the independent MFMAs
        constexpr int NM = MT * NFT + MT * NCT;
#pragma unroll
        for (int k = 0; k < NM; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // VALU
        }
      }
      SCHED_PIN(2)   // region j
      {
        // One element of every accumulator the region wrote: its MFMAs have retired before the next region's
        // h rows (and the next iteration's LDS reads) may land in the registers they read.
        float touch = 0.f;
#pragma unroll
        for (int a2 = 0; a2 < MT; ++a2) {
#pragma unroll
          for (int f2 = 0; f2 < NFT; ++f2) touch += accW[a2][f2][0];
#pragma unroll
          for (int c2 = 0; c2 < NCT; ++c2) touch += accU[a2][c2][0];
        }
        completion_read(touch);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (!LAST) ew_publish(t - 1, eo_out, dpo);
    SCHED_PIN(3)   // LDS publish
    lds_barrier();
    SCHED_PIN(4)   // barrier passed
  };

  f32x4 dpoE[MT], dpoO[MT];     // d_pre_s of even / odd s
  EwOps eE, eO;                 // operands of EW(s) for even / odd s
  XT xE, xO;                    // x_s^T for even / odd s
  {
    EwOut o0;
    if ((Tn - 1) & 1) {
      load_ew(Tn - 1, eO); load_xt(Tn - 1, xO);
      if (Tn >= 2) load_ew(Tn - 2, eE);
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_chunk(j, eO, o0);
      ew_publish(Tn - 1, o0, dpoO);
    } else {
      load_ew(Tn - 1, eE); load_xt(Tn - 1, xE);
      if (Tn >= 2) load_ew(Tn - 2, eO);
#pragma unroll
      for (int j = 0; j < 4; ++j) ew_chunk(j, eE, o0);
      ew_publish(Tn - 1, o0, dpoE);
    }
  }
  lds_barrier();
  {
    // iteration t: d_x(t+1) from dpo[(t+1)&1]; dW(t) with x[t&1]; EW(t-1) with e[(t-1)&1] -> dpo[(t-1)&1];
    // requests x_{t-1} -> x[(t-1)&1] and EW(t-2) operands -> e[t&1]
    int t = Tn - 1;
    if ((t & 1) && t >= 1) { iter(std::false_type{}, t, dpoE, eE, eO, xO, xE); --t; }
    for (; t >= 2; t -= 2) {
      iter(std::false_type{}, t, dpoO, eO, eE, xE, xO);
      iter(std::false_type{}, t - 1, dpoE, eE, eO, xO, xE);
    }
    iter(std::true_type{}, 0, dpoO, eO, eE, xE, xO);
  }
  dx_partial(0, dpoE);
  if (1 < Tn) finish_dx(1);
  lds_barrier();
  finish_dx(0);
#ifdef FASTGRNN_DIAG_STAMPS
  if ((DIAG & 16) && blockIdx.x == 7 && l == 0) {
    for (int k = 0; k < 8; ++k) g_diag[wv][k] = dsum[k];
  }
#endif
  // ---- flush ---------------------------------------------------------------------------------
  if (valid) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) st4(d_h0 + (size_t)b * H + n0 + 4 * mt, dh[mt]);
  }
  // dU / dW slabs: D row 4g+r of tile a is n = wv*HS + a*16 + 4g + r; lane i of column tile c
  // is column i*NCT + c (dW: feature i*NFT + f2), so a lane's tiles are contiguous in memory
  {
    float* pu = part + (size_t)blockIdx.x * slab_stride(H, F);
    float* pw = pu + H * H;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = wv * HS + a * 16 + 4 * g + r;
#pragma unroll
        for (int v = 0; v < NCT / 4; ++v)
          st4(pu + (size_t)n * H + i * NCT + 4 * v,
              f32x4{accU[a][4 * v][r], accU[a][4 * v + 1][r], accU[a][4 * v + 2][r], accU[a][4 * v + 3][r]});
#pragma unroll
        for (int f2 = 0; f2 < NFT; ++f2) pw[(size_t)n * F + i * NFT + f2] = accW[a][f2][r];
      }
  }
  // bias partials: sum over the 16 utterance lanes of each group
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float a = sbz[mt][r], c = sbh[mt][r];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) { a += __shfl_xor(a, m); c += __shfl_xor(c, m); }
      if (i == 0) {
        float* pb = part + (size_t)blockIdx.x * slab_stride(H, F) + H * H + H * F;
        pb[n0 + 4 * mt + r] = a;
        pb[H + n0 + 4 * mt + r] = c;
      }
    }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { pz += __shfl_xor(pz, m); pn += __shfl_xor(pn, m); }
  if (l == 0) { S.red[wv] = pz; S.red[4 + wv] = pn; }
  __syncthreads();
  if (tid == 0) {
    float* pzn = part + (size_t)blockIdx.x * slab_stride(H, F) + H * H + H * F + 2 * H;
    pzn[0] = S.red[0] + S.red[1] + S.red[2] + S.red[3];
    pzn[1] = S.red[4] + S.red[5] + S.red[6] + S.red[7];
  }
}

// Deterministic reduction of the per-workgroup slabs in ONE launch: out[i] = sum_wg part[wg][i]
// for the whole gradient vector dU | dW | d_bz | d_bh | d_zeta | d_nu (.cu:542-545), by
// fixed_order_sum (scan_common.h) with 8 loads per round.
__global__ __launch_bounds__(1024) void reduce_slabs(int nwg, int H, int F, int stride,
                                                     const float* __restrict__ part,
                                                     const float* __restrict__ zeta, const float* __restrict__ nu,
                                                     float* __restrict__ d_u, float* __restrict__ d_w,
                                                     float* __restrict__ d_bz, float* __restrict__ d_bh,
                                                     float* __restrict__ d_zeta, float* __restrict__ d_nu) {
  const int oW = H * H, oBz = oW + H * F, oBh = oBz + H, oZ = oBh + H;
  fixed_order_sum<8>(
      nwg, oZ + 2, [&](int wg, int idx) { return part + (size_t)wg * stride + idx; },
      [&](int idx, float t) {
        if (idx < oW) d_u[idx] = t;
        else if (idx < oBz) d_w[idx - oW] = t;
        else if (idx < oBh) d_bz[idx - oBz] = t;
        else if (idx < oZ) d_bh[idx - oBh] = t;
        else if (idx == oZ) d_zeta[0] = raw_scalar_grad(t, zeta);
        else d_nu[0] = raw_scalar_grad(t, nu);
      });
}

size_t bwd_ws_bytes(const fastgrnn_desc& d) {
  size_t nwg = (d.B + 15) / 16;
  return align256(nwg * (size_t)slab_stride(d.H, d.F) * 4);
}

template <int H, int F>
int launch_fwd(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0, void* hs, void* zs,
               void* cs, hipStream_t s) {
  dim3 grid((d.B + 15) / 16), block(256);
  auto args = [&](auto kern) __attribute__((always_inline)) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, d.T, d.B, (const float*)x, (const float*)h0, (const float*)p.w,
                       (const float*)p.u, (const float*)p.bias_gate, (const float*)p.bias_update,
                       (const float*)p.zeta, (const float*)p.nu, (float*)hs, (float*)zs, (float*)cs);
  };
  const bool launched =
      pick_int<0, 1, 2>(d.gate_nl, [&](auto G_) {
      return pick_bool(zs != nullptr, [&](auto GO_) {
      return pick_bool((d.B % 16) != 0, [&](auto RG_) {
        constexpr int G = decltype(G_)::value;
        if constexpr (fwd_mfma_built(G)) { args(fwd_scan_mfma<H, F, G, decltype(GO_)::value, decltype(RG_)::value>); return true; }
        else return false;
      }); }); });
  if (!launched) return FASTGRNN_ERR_UNSUPPORTED;
  return launch_status();
}

template <int H, int F>
int launch_bwd(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x, const void* hs,
               const void* zs, const void* cs, const void* h0, const fastgrnn_grads& g, void* ws, hipStream_t s) {
  float* part = reinterpret_cast<float*>(ws);
  const int nwg = (d.B + 15) / 16;
  dim3 grid(nwg), block(256);
  auto args = [&](auto kern) __attribute__((always_inline)) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, d.T, d.B, (const float*)ghs, (const float*)x, (const float*)hs,
                       (const float*)zs, (const float*)cs, (const float*)h0, (const float*)p.w, (const float*)p.u,
                       (const float*)p.zeta, (const float*)p.nu, (float*)g.d_x, (float*)g.d_h0, part);
  };
  const bool launched =
      pick_int<0, 1, 2>(d.gate_nl, [&](auto G_) {
      return pick_bool((d.B % 16) != 0, [&](auto RG_) {
        constexpr int G = decltype(G_)::value;
        constexpr bool RG = decltype(RG_)::value;
        if constexpr (bwd_mfma_built(H, G, RG)) { args(bwd_scan_mfma<H, F, G, RG>); return true; }
        else return false;
      }); });
  if (!launched) return FASTGRNN_ERR_UNSUPPORTED;
  const int ntot = H * H + H * F + 2 * H + 2;
  hipLaunchKernelGGL(reduce_slabs, dim3((ntot + 63) / 64), dim3(1024), 0, s, nwg, H, F, slab_stride(H, F), part,
                     (const float*)p.zeta, (const float*)p.nu, (float*)g.d_u, (float*)g.d_w,
                     (float*)g.d_bias_gate, (float*)g.d_bias_update, (float*)g.d_zeta, (float*)g.d_nu);
  return launch_status();
}

bool shape_ok(int H, int F) { return (H == 128 && F == 32) || (H == 64 && F == 32) || (H == 128 && F == 64); }

}  // namespace

bool mfma_supported(const fastgrnn_desc& d, int direction) {
  if (direction == 1 && d.H == 128 && (d.B % 16) != 0) return false;   // see launch_bwd
  return d.dtype == FASTGRNN_F32 && d.w_rank == 0 && d.u_rank == 0 && d.update_nl == FASTGRNN_NL_TANH &&
         d.gate_nl >= FASTGRNN_NL_SIGMOID && d.gate_nl <= FASTGRNN_NL_TANH && shape_ok(d.H, d.F);
}
size_t mfma_forward_ws(const fastgrnn_desc&) { return 0; }
size_t mfma_backward_ws(const fastgrnn_desc& d) { return bwd_ws_bytes(d); }

int mfma_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0, void* hs,
                 void* zs, void* cs, void*, hipStream_t s) {
  if ((zs == nullptr) != (cs == nullptr)) return FASTGRNN_ERR_NULL_POINTER;
  if (d.H == 128 && d.F == 32) return launch_fwd<128, 32>(d, p, x, h0, hs, zs, cs, s);
  if (d.H == 64 && d.F == 32) return launch_fwd<64, 32>(d, p, x, h0, hs, zs, cs, s);
  if (d.H == 128 && d.F == 64) return launch_fwd<128, 64>(d, p, x, h0, hs, zs, cs, s);
  return FASTGRNN_ERR_UNSUPPORTED;
}

int mfma_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x, const void* hs,
                  const void* zs, const void* cs, const void* h0, const fastgrnn_grads& g, void* ws,
                  hipStream_t s) {
  if (d.H == 128 && d.F == 32) return launch_bwd<128, 32>(d, p, ghs, x, hs, zs, cs, h0, g, ws, s);
  if (d.H == 64 && d.F == 32) return launch_bwd<64, 32>(d, p, ghs, x, hs, zs, cs, h0, g, ws, s);
  if (d.H == 128 && d.F == 64) return launch_bwd<128, 64>(d, p, ghs, x, hs, zs, cs, h0, g, ws, s);
  return FASTGRNN_ERR_UNSUPPORTED;
}

}  // namespace fastgrnn
