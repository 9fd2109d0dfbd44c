// The end of a trainer iteration in one launch: optimizer.step() (trainClassifier.py:249) for every parameter tensor of
// a model, then the IHT phase on the W/U matrices (trainClassifier.py:251-259 -> utils.py:53-81).  gfx950 only.
// (No inline assembly of its own; lds_writes_landed() is common.h's one-instruction wait, which the second rule of
// DESIGN.md 4.0 asks for in any loop that mixes LDS operations with memory instructions.)
//   The eight rules of the trainer's configure_optimizer (trainClassifier.py:67-95), by the public algo code: Adam, SGD
//   (fastgrnn_hip_train_update), RMSprop, Adagrad, Adadelta, Adamax, ASGD, Rprop (fastgrnn_hip_optim_update).  They are
//   torch.optim's at torch 2.10 on the foreach=False, maximize=False, non-differentiable path (amsgrad off, L2 weight
//   decay; include/fastgrnn_hip.h spells them out): fp32 operands, fp32 arithmetic with fmaf where torch's kernels
//   contract too, correctly rounded division and square root; what depends on the step count -- Adam's and Adamax's bias
//   corrections, Adagrad's decayed learning rate, ASGD's next eta and mu -- is computed in double by one thread.
//   lerp(a, g, w) is torch's: a + w (g - a) below w = 0.5, g - (g - a)(1 - w) from there on (exact at w = 1).
//   IHT mode 1 (utils.hardThreshold): zero what lies strictly below the magnitude of 0-based rank keep_rank and record
//   the support; mode 2 (utils.supportBasedThreshold): zero what the recorded support excludes.
// One workgroup of UPD_THREADS per parameter tensor ("segment"), no communication between workgroups.  Thread t owns
// elements t, t + UPD_THREADS, ... in EVERY phase, so a thread only ever USES values it stored itself (the clamped loads
// of a ragged last iteration fetch element n-1, whoever owns it, and discard it) and the threshold phase follows the
// update behind a workgroup barrier.  lr, the step count and the IHT mode are device scalars: a captured graph of the
// call serves a whole training run.
// The threshold is found exactly by radix select on the magnitudes' bit patterns (for non-NaN fp32, bits & 0x7fffffff
// orders as an unsigned integer): four 8-bit passes from the top, each a 256-bin histogram in LDS of the elements that
// still match the digits chosen so far.  Integer LDS atomics: the counts do not depend on arrival order.
// ASGD's eta and mu are read by every workgroup of every launch of a call and replaced by the same call: they live in
// scalars[4] as two pairs, indexed by the step's parity.  Step t reads pair (t-1) & 1 and every workgroup's thread 0
// writes the same two values into pair t & 1 with ordinary stores, so no workgroup can read what another has already
// replaced.  Step 1 reads nothing: eta = lr, mu = 1, as torch initialises them.
// One kernel per rule (a template argument), so that no rule carries another's registers.
// kernels_guard.hip runs the same eight rules under the gradient guard and needs this file's kernel, its radix select,
// its segment table and the host code that fills it.  It gets them by including THIS file with UPDATE_GUARD defined as
// 1: the kernel template then comes out as guarded_update_k<ALGO>, which takes a fastgrnn_guard_state in place of the
// step scalar, and the host entry point below is left out.  The switch is textual on purpose: compiled on its own
// (UPDATE_GUARD 0) the kernel's body reaches the compiler as the text it was before the guard existed, and the eight
// kernels come out with the same device code, digest for digest (profiles/r17_guard.md); the host side around it did
// change (the table fill became update_launches, shared with the guarded entry).  The rules as an inlined device
// function called by two wrappers came out with another schedule for two of the eight.
// The three macros of the switch live from the kernel's signature to the end of its body and nowhere else.
// Latency-bound byte work on at most 32 CUs (a model has 6-14 tensors of at most 256x256): what it saves is launches
// and the host round trip, not bandwidth.
#include <type_traits>

#include "common.h"

#ifndef UPDATE_GUARD
#define UPDATE_GUARD 0
#endif

namespace fastgrnn {
namespace {

constexpr int UPD_THREADS = 1024;

struct upd_seg {                 // one row of the table that rides in the kernel arguments (64 bytes; 32 rows: 2048)
  float* p;
  const float* g;
  float* s0;                     // Adam exp_avg, SGD momentum buffer, RMSprop square_avg, Adagrad sum, Adadelta square_avg,
                                 // Adamax exp_avg, ASGD ax, Rprop prev
  float* s1;                     // Adam exp_avg_sq, RMSprop momentum_buffer, Adadelta acc_delta, Adamax exp_inf, Rprop step_size
  float* s2;                     // RMSprop grad_avg
  unsigned char* sup;            // [n] bytes, IHT segments only
  int n, keep_rank, iht, pad;
};
struct upd_table { upd_seg seg[FASTGRNN_UPDATE_MAX_SEGS]; };

struct upd_hyper {               // fields by rule, below at to_hyper()
  double d0, d1, d2;
  float f0, f1, f2, f3;
  float eps, wd;
  int i0, i1;
};

enum { ADAM = 0, SGD = 1, RMSPROP = 2, ADAGRAD = 3, ADADELTA = 4, ADAMAX = 5, ASGD = 6, RPROP = 7 };

// b^e for an integer e >= 0 by squaring, in double (at most 63 steps; its rounding error, ~1e-14 relative, is far
// below the fp32 arithmetic it feeds)
__device__ double ipow(double b, long long e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__device__ __forceinline__ float lerp_torch(float a, float g, float w, float omw) {
  const float diff = g - a;
  return w < 0.5f ? fmaf(w, diff, a) : g - diff * omw;
}

__device__ __forceinline__ unsigned mag_key(float v) { return __builtin_bit_cast(unsigned, v) & 0x7fffffffu; }

// Hard threshold of p[0..n) (utils.hardThreshold): zero what lies strictly below the magnitude of 0-based rank
// keep_rank (1 <= keep_rank < n) among the ascending magnitudes, and write the support bytes.  Called by every thread
// of the workgroup (it holds barriers); hist[256] and s_sel[2] are the caller's LDS.
__device__ __forceinline__ void iht_threshold(float* p, unsigned char* sup, const int n, const int keep_rank,
                                              unsigned* hist, unsigned* s_sel) {
  const int tid = threadIdx.x;
  // the key of 0-based rank keep_rank among the ascending magnitudes, most significant digit first
  unsigned prefix = 0, known = 0, rank = (unsigned)keep_rank;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();                                           // (also orders this thread's stores of p in front of its loads)
    for (int i0 = tid; i0 < n; i0 += 4 * UPD_THREADS) {
      unsigned k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)                              // (no branch around the loads: second rule of DESIGN.md 4.0)
        k[j] = mag_key(p[min(i0 + j * UPD_THREADS, n - 1)]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {                            // (every lane adds, 0 where it does not count: no branch either)
        const bool counts = i0 + j * UPD_THREADS < n && (k[j] & known) == prefix;
        atomicAdd(&hist[(k[j] >> shift) & 255u], counts ? 1u : 0u);
      }
      lds_writes_landed();                                     // (second rule of DESIGN.md 4.0: the next iteration's loads)
    }
    __syncthreads();
    if (tid < 64) {                                            // wave 0: the bin that holds the rank, by a scan over 64 x 4 bins
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      const unsigned own = c0 + c1 + c2 + c3;
      unsigned inc = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d);
        if (tid >= d) inc += t;
      }
      const unsigned exc = inc - own;
      if (rank >= exc && rank < inc) {                         // exactly one lane: the counts sum to more than rank
        unsigned r = rank - exc, bin = 4u * tid;
        if (r >= c0) { r -= c0; ++bin;
          if (r >= c1) { r -= c1; ++bin;
            if (r >= c2) { r -= c2; ++bin; } } }
        s_sel[0] = prefix | (bin << shift);
        s_sel[1] = r;
      }
    }
    __syncthreads();
    prefix = s_sel[0];
    rank = s_sel[1];
    known |= 255u << shift;
  }
  // prefix is now the threshold's bit pattern: strictly smaller magnitudes go, ties stay (utils.hardThreshold)
  for (int i = tid; i < n; i += UPD_THREADS) {
    float pn = p[i];
    if (mag_key(pn) < prefix) {
      pn = 0.f;
      p[i] = 0.f;
    }
    sup[i] = pn != 0.f ? 1 : 0;
  }
}

// One workgroup's work: the rule ALGO on segment blockIdx.x of the table, then that segment's IHT phase.
// UPDATE_GUARD 0: step_p is the caller's step count.
// UPDATE_GUARD 1: the step count is guard->applied, every gradient element is multiplied by guard->coef (one fp32
// multiply in front of the weight-decay fmaf), and with guard->skip set the rule is the identity: the update arm
// stores nothing -- no parameter, no state tensor, no ASGD scalar -- and the IHT phase runs on the parameters as they
// are.  All three come from loads at kernel entry, through a pointer that is uniform over the launch: the skip branch
// is wave-uniform and is taken before the first LDS write.
#if UPDATE_GUARD
#define UPDATE_KERNEL guarded_update_k
#define UPDATE_COUNT_ARG const fastgrnn_guard_state* __restrict__ guard
#define UPDATE_GRAD(i) (g[i] * coef)
#else
#define UPDATE_KERNEL update_k
#define UPDATE_COUNT_ARG const long long* __restrict__ step_p
#define UPDATE_GRAD(i) g[i]
#endif
template <int ALGO>
__global__ __launch_bounds__(UPD_THREADS) void UPDATE_KERNEL(upd_table tab, upd_hyper hy, const float* __restrict__ lr_p,
                                                             UPDATE_COUNT_ARG, const int* __restrict__ mode_p,
                                                             float* scalars) {
  __shared__ unsigned hist[256];
  // Adam: lr / (1 - beta1^t), sqrt(1 - beta2^t);  Adagrad: lr / (1 + (t-1) lr_decay);  Adamax: lr / (1 - beta1^t)
  __shared__ float s_sc[ALGO == ADAM ? 2 : 1];
  __shared__ unsigned s_sel[2];    // radix select: digits chosen so far, rank left among the elements that match them
  const int tid = threadIdx.x;
  const upd_seg sg = tab.seg[blockIdx.x];
  const int n = sg.n;
  float* p = sg.p;
  const float* g = sg.g;
  const float lr = lr_p[0];
#if UPDATE_GUARD
  const long long step = guard->applied;
  const float coef = guard->coef;
  const bool skip = guard->skip != 0;
#else
  const long long step = step_p[0];
#endif
  int mode = mode_p ? mode_p[0] : 0;
  if (!sg.iht || (mode != 1 && mode != 2)) mode = 0;         // (any other value on the device behaves as 0)

  // ---- a. the update; mode 2's mask and the support of a keep-everything segment ride along (elementwise)
  const bool mask_now = mode == 2;
  const bool sup_now = mode == 1 && sg.keep_rank <= 0;
  auto store_p = [&](int i, float pn) {
    if (mask_now && sg.sup[i] == 0) pn = 0.f;
    p[i] = pn;
    if (sup_now) sg.sup[i] = pn != 0.f ? 1 : 0;
  };

#if UPDATE_GUARD
  if (skip) {
    // a rejected step: p' = p.  What rides along with the stores of p still happens, on the old values
    if (mask_now || sup_now)
      for (int i = tid; i < n; i += UPD_THREADS) store_p(i, p[i]);
  } else
#endif
  if constexpr (ALGO == ADAM) {
    // d0 = beta1, d1 = beta2; f0 = beta1, f1 = 1 - beta1, f2 = beta2, f3 = 1 - beta2
    if (tid == 0) {
      const double bc1 = 1.0 - ipow(hy.d0, step), bc2 = 1.0 - ipow(hy.d1, step);
      s_sc[0] = (float)((double)lr / bc1);
      s_sc[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    const float step_size = s_sc[0], bc2_sqrt = s_sc[1];
    float* m = sg.s0;
    float* v = sg.s1;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float mi = fmaf(hy.f0, m[i], hy.f1 * gi);
      const float vi = fmaf(hy.f2, v[i], hy.f3 * gi * gi);
      const float denom = sqrtf(vi) / bc2_sqrt + hy.eps;
      const float pn = fmaf(-step_size, mi / denom, pi);
      m[i] = mi;
      v[i] = vi;
      store_p(i, pn);
    }
  } else if constexpr (ALGO == SGD) {
    // f0 = momentum, f1 = 1 - dampening; i0 = nesterov
    float* b = sg.s0;
    const bool first = step <= 1, has_mom = hy.f0 != 0.f;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      float d = gi;
      if (has_mom) {                                           // (torch keeps no buffer, and ignores dampening, without momentum)
        const float bi = first ? gi : fmaf(hy.f0, b[i], hy.f1 * gi);
        b[i] = bi;
        d = hy.i0 ? fmaf(hy.f0, bi, gi) : bi;
      }
      store_p(i, fmaf(-lr, d, pi));
    }
  } else if constexpr (ALGO == RMSPROP) {
    // f0 = alpha, f1 = 1 - alpha (the lerp weight), f2 = 1 - f1 in float, f3 = momentum; i0 = centered, i1 = momentum > 0
    float* v = sg.s0;
    float* b = sg.s1;
    float* a = sg.s2;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float v0 = v[i];
      const float a0 = hy.i0 ? a[i] : 0.f;
      const float b0 = hy.i1 ? b[i] : 0.f;
      const float vi = fmaf(hy.f0, v0, hy.f1 * gi * gi);
      v[i] = vi;
      float rad = vi;
      if (hy.i0) {
        const float ai = lerp_torch(a0, gi, hy.f1, hy.f2);
        a[i] = ai;
        rad = fmaf(-ai, ai, vi);
      }
      float d = gi / (sqrtf(rad) + hy.eps);
      if (hy.i1) {
        d = fmaf(hy.f3, b0, d);
        b[i] = d;
      }
      store_p(i, fmaf(-lr, d, pi));
    }
  } else if constexpr (ALGO == ADAGRAD) {
    // d0 = lr_decay
    if (tid == 0) s_sc[0] = (float)((double)lr / (1.0 + (double)(step - 1) * hy.d0));
    __syncthreads();
    const float clr = s_sc[0];
    float* s = sg.s0;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float si = fmaf(gi, gi, s[i]);
      s[i] = si;
      store_p(i, fmaf(-clr, gi / (sqrtf(si) + hy.eps), pi));
    }
  } else if constexpr (ALGO == ADADELTA) {
    // f0 = rho, f1 = 1 - rho
    float* v = sg.s0;
    float* a = sg.s1;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float ai = a[i];
      const float vi = fmaf(hy.f0, v[i], hy.f1 * gi * gi);
      v[i] = vi;
      const float dl = sqrtf(ai + hy.eps) / sqrtf(vi + hy.eps) * gi;
      a[i] = fmaf(hy.f0, ai, hy.f1 * dl * dl);
      store_p(i, fmaf(-lr, dl, pi));
    }
  } else if constexpr (ALGO == ADAMAX) {
    // d0 = beta1; f0 = 1 - beta1 (the lerp weight), f1 = 1 - f0 in float, f2 = beta2
    if (tid == 0) s_sc[0] = (float)((double)lr / (1.0 - ipow(hy.d0, step)));
    __syncthreads();
    const float clr = s_sc[0];
    float* m = sg.s0;
    float* u = sg.s1;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float mi = lerp_torch(m[i], gi, hy.f0, hy.f1);
      const float ui = fmaxf(hy.f2 * u[i], fabsf(gi) + hy.eps);
      m[i] = mi;
      u[i] = ui;
      store_p(i, fmaf(-clr, mi / ui, pi));
    }
  } else if constexpr (ALGO == ASGD) {
    // d0 = lambd, d1 = alpha, d2 = t0
    float eta = lr, mu = 1.f;
    if (step > 1) {                                            // (uniform) what step t-1 left
      const float* prev = scalars + 2 * (int)((step - 1) & 1);
      eta = prev[0];
      mu = prev[1];
    }
    if (tid == 0) {                                            // what step t+1 reads: the other pair
      float* next = scalars + 2 * (int)(step & 1);
      const double t = (double)step, dif = t - hy.d2;
      next[0] = (float)((double)lr / pow(1.0 + hy.d0 * (double)lr * t, hy.d1));
      next[1] = (float)(1.0 / (dif > 1.0 ? dif : 1.0));
    }
    const float decay = (float)(1.0 - hy.d0 * (double)eta);   // torch forms 1 - lambd eta in double and rounds it once
    const bool copy = mu == 1.f;
    float* ax = sg.s0;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, UPDATE_GRAD(i));
      const float pn = fmaf(-eta, gi, pi * decay);
      const float axi = ax[i];
      ax[i] = copy ? pn : fmaf(mu, pn - axi, axi);             // (the average follows the unmasked step, as all state does)
      store_p(i, pn);
    }
  } else {
    // Rprop: f0 = etaminus, f1 = etaplus, f2 = step_min, f3 = step_max; lr and the step count are not read
    float* prev = sg.s0;
    float* ss = sg.s1;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float gi = UPDATE_GRAD(i), pi = p[i], s0 = ss[i];
      const float s = gi * prev[i];                            // (torch takes the sign of the rounded fp32 product)
      const float factor = s > 0.f ? hy.f1 : s < 0.f ? hy.f0 : 1.f;
      const float st = fminf(fmaxf(s0 * factor, hy.f2), hy.f3);
      const float gk = s < 0.f ? 0.f : gi;
      const float sgn = gk > 0.f ? 1.f : gk < 0.f ? -1.f : 0.f;
      ss[i] = st;
      prev[i] = gk;
      store_p(i, fmaf(-sgn, st, pi));
    }
  }
  if (mode != 1 || sg.keep_rank <= 0) return;                  // (uniform over the workgroup: the barriers below are safe)

  // ---- b. hard threshold: strictly below the magnitude of 0-based rank keep_rank goes, the support is recorded
  iht_threshold(p, sg.sup, n, sg.keep_rank, hist, s_sel);
}
#undef UPDATE_GRAD
#undef UPDATE_COUNT_ARG
#undef UPDATE_KERNEL

// ---- the two public shapes of a call, brought to the kernel's: every float derives from the public doubles here
inline upd_hyper to_hyper(const fastgrnn_update_hyper& h) {
  upd_hyper hy = {};
  hy.d0 = h.beta1_or_momentum;
  hy.d1 = h.beta2_or_dampening;
  hy.f0 = (float)h.beta1_or_momentum;
  hy.f1 = (float)(1.0 - (h.algo == ADAM ? h.beta1_or_momentum : h.beta2_or_dampening));
  hy.f2 = (float)h.beta2_or_dampening;
  hy.f3 = (float)(1.0 - h.beta2_or_dampening);
  hy.eps = (float)h.eps;
  hy.wd = (float)h.weight_decay;
  hy.i0 = h.nesterov;
  return hy;
}

inline upd_hyper to_hyper(const fastgrnn_optim_hyper& h) {
  upd_hyper hy = {};
  hy.wd = (float)h.weight_decay;
  switch (h.algo) {
    case RMSPROP:                                              // h = alpha, eps, momentum
      hy.f0 = (float)h.h[0];
      hy.f1 = (float)(1.0 - h.h[0]);
      hy.f2 = 1.f - hy.f1;
      hy.f3 = (float)h.h[2];
      hy.eps = (float)h.h[1];
      hy.i0 = h.flags & 1;
      hy.i1 = h.h[2] > 0.0;
      break;
    case ADAGRAD:                                              // h = lr_decay, eps
      hy.d0 = h.h[0];
      hy.eps = (float)h.h[1];
      break;
    case ADADELTA:                                             // h = rho, eps
      hy.f0 = (float)h.h[0];
      hy.f1 = (float)(1.0 - h.h[0]);
      hy.eps = (float)h.h[1];
      break;
    case ADAMAX:                                               // h = beta1, beta2, eps
      hy.d0 = h.h[0];
      hy.f0 = (float)(1.0 - h.h[0]);
      hy.f1 = 1.f - hy.f0;
      hy.f2 = (float)h.h[1];
      hy.eps = (float)h.h[2];
      break;
    case ASGD:                                                 // h = lambd, alpha, t0
      hy.d0 = h.h[0];
      hy.d1 = h.h[1];
      hy.d2 = h.h[2];
      break;
    default:                                                   // Rprop: h = etaminus, etaplus, step_min, step_max
      hy.f0 = (float)h.h[0];
      hy.f1 = (float)h.h[1];
      hy.f2 = (float)h.h[2];
      hy.f3 = (float)h.h[3];
      hy.wd = 0.f;
      break;
  }
  return hy;
}

inline void set_states(upd_seg& d, const fastgrnn_update_seg& a) {
  d.s0 = reinterpret_cast<float*>(a.state0);
  d.s1 = reinterpret_cast<float*>(a.state1);
}

inline void set_states(upd_seg& d, const fastgrnn_optim_seg& a) {
  d.s0 = reinterpret_cast<float*>(a.state[0]);
  d.s1 = reinterpret_cast<float*>(a.state[1]);
  d.s2 = reinterpret_cast<float*>(a.state[2]);
}

// The launches of a call: one per FASTGRNN_UPDATE_MAX_SEGS segments, the table filled from the public segments;
// launch(std::integral_constant<int, ALGO>, cnt, tab, hy) starts the kernel of the call's rule.
template <typename Hyper, typename Seg, typename Launch>
void update_launches(const Hyper& h, const Seg* segs, int n_segs, Launch launch) {
  const upd_hyper hy = to_hyper(h);
  for (int s0 = 0; s0 < n_segs; s0 += FASTGRNN_UPDATE_MAX_SEGS) {
    const int cnt = n_segs - s0 < FASTGRNN_UPDATE_MAX_SEGS ? n_segs - s0 : FASTGRNN_UPDATE_MAX_SEGS;
    upd_table tab = {};
    for (int k = 0; k < cnt; ++k) {
      const Seg& a = segs[s0 + k];
      upd_seg& d = tab.seg[k];
      d.p = reinterpret_cast<float*>(a.param);
      d.g = reinterpret_cast<const float*>(a.grad);
      set_states(d, a);
      d.sup = a.support;
      d.n = (int)a.n;
      d.keep_rank = (int)a.keep_rank;
      d.iht = a.iht != 0;
    }
    switch (h.algo) {
      case ADAM: launch(std::integral_constant<int, ADAM>{}, cnt, tab, hy); break;
      case SGD: launch(std::integral_constant<int, SGD>{}, cnt, tab, hy); break;
      case RMSPROP: launch(std::integral_constant<int, RMSPROP>{}, cnt, tab, hy); break;
      case ADAGRAD: launch(std::integral_constant<int, ADAGRAD>{}, cnt, tab, hy); break;
      case ADADELTA: launch(std::integral_constant<int, ADADELTA>{}, cnt, tab, hy); break;
      case ADAMAX: launch(std::integral_constant<int, ADAMAX>{}, cnt, tab, hy); break;
      case ASGD: launch(std::integral_constant<int, ASGD>{}, cnt, tab, hy); break;
      default: launch(std::integral_constant<int, RPROP>{}, cnt, tab, hy); break;
    }
  }
}

}  // namespace

#if !UPDATE_GUARD
template <typename Hyper, typename Seg>
int update_step(const Hyper& h, const Seg* segs, int n_segs, const float* lr, const int64_t* step,
                const int32_t* iht_mode, float* scalars, hipStream_t s) {
  update_launches(h, segs, n_segs, [&](auto algo, int cnt, const upd_table& tab, const upd_hyper& hy) {
    hipLaunchKernelGGL(update_k<decltype(algo)::value>, dim3(cnt), dim3(UPD_THREADS), 0, s, tab, hy, lr,
                       (const long long*)step, (const int*)iht_mode, scalars);
  });
  return launch_status();
}

template int update_step(const fastgrnn_update_hyper&, const fastgrnn_update_seg*, int, const float*, const int64_t*,
                         const int32_t*, float*, hipStream_t);
template int update_step(const fastgrnn_optim_hyper&, const fastgrnn_optim_seg*, int, const float*, const int64_t*,
                         const int32_t*, float*, hipStream_t);
#endif

}  // namespace fastgrnn
