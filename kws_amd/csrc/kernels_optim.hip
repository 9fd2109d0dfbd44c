// optimizer.step() for the other six rules of the trainer's configure_optimizer (trainClassifier.py:67-95) -- RMSprop,
// Adagrad, Adadelta, Adamax, ASGD, Rprop -- and then the IHT phase, in one launch: kernels_update.hip's shape with up
// to three state tensors per parameter.  gfx950 only.  (No inline assembly of its own; the threshold phase and its
// one-instruction LDS wait are iht_select.h's, shared with kernels_update.hip.)
//   The rules are torch.optim's at torch 2.10 on the foreach=False, maximize=False, non-differentiable path
//   (include/fastgrnn_hip.h spells them out): fp32 operands, fp32 arithmetic with fmaf where torch's kernels contract
//   too, correctly rounded division and square root; what depends on the step count -- Adagrad's decayed learning rate,
//   Adamax's bias correction, ASGD's next eta and mu -- is computed in double by one thread.
//   lerp(a, g, w) is torch's: a + w (g - a) below w = 0.5, g - (g - a)(1 - w) from there on (exact at w = 1).
// One workgroup of UPD_THREADS per parameter tensor ("segment"), no communication between workgroups.  Thread t owns
// elements t, t + UPD_THREADS, ... in EVERY phase, so the threshold phase follows the update behind a workgroup barrier.
// ASGD's eta and mu are read by every workgroup of every launch of a call and replaced by the same call: they live in
// scalars[4] as two pairs, indexed by the step's parity.  Step t reads pair (t-1) & 1 and every workgroup's thread 0
// writes the same two values into pair t & 1 with ordinary stores, so no workgroup can read what another has already
// replaced.  Step 1 reads nothing: eta = lr, mu = 1, as torch initialises them.
// One kernel per rule (a template argument), so that no rule carries another's registers.
// Latency-bound byte work on at most 32 CUs, as train_update_k: what it saves is launches and the host round trip.
#include "iht_select.h"

namespace fastgrnn {
namespace {

struct opt_seg {                 // one row of the table that rides in the kernel arguments (64 bytes; 32 rows: 2048)
  float* p;
  const float* g;
  float* s0;                     // RMSprop square_avg, Adagrad sum, Adadelta square_avg, Adamax exp_avg, ASGD ax, Rprop prev
  float* s1;                     // RMSprop momentum_buffer, Adadelta acc_delta, Adamax exp_inf, Rprop step_size
  float* s2;                     // RMSprop grad_avg
  unsigned char* sup;            // [n] bytes, IHT segments only
  int n, keep_rank, iht, pad;
};
struct opt_table { opt_seg seg[FASTGRNN_UPDATE_MAX_SEGS]; };

struct opt_hyper {               // fields by rule, below at optim_update()
  double d0, d1, d2;
  float f0, f1, f2, f3;
  float eps, wd;
  int centered, has_mom;
};

enum { RMSPROP = 2, ADAGRAD = 3, ADADELTA = 4, ADAMAX = 5, ASGD = 6, RPROP = 7 };

__device__ __forceinline__ float lerp_torch(float a, float g, float w, float omw) {
  const float diff = g - a;
  return w < 0.5f ? fmaf(w, diff, a) : g - diff * omw;
}

template <int ALGO>
__global__ __launch_bounds__(UPD_THREADS) void optim_update_k(opt_table tab, opt_hyper hy, const float* __restrict__ lr_p,
                                                              const long long* __restrict__ step_p,
                                                              const int* __restrict__ mode_p, float* scalars) {
  __shared__ unsigned hist[256];
  __shared__ float s_sc[1];        // Adagrad: lr / (1 + (t-1) lr_decay);  Adamax: lr / (1 - beta1^t)
  __shared__ unsigned s_sel[2];    // radix select: digits chosen so far, rank left among the elements that match them
  const int tid = threadIdx.x;
  const opt_seg sg = tab.seg[blockIdx.x];
  const int n = sg.n;
  float* p = sg.p;
  const float* g = sg.g;
  const float lr = lr_p[0];
  const long long step = step_p[0];
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

  if constexpr (ALGO == RMSPROP) {
    // f0 = alpha, f1 = 1 - alpha (the lerp weight), f2 = 1 - f1 in float, f3 = momentum
    float* v = sg.s0;
    float* b = sg.s1;
    float* a = sg.s2;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, g[i]);
      const float v0 = v[i];
      const float a0 = hy.centered ? a[i] : 0.f;
      const float b0 = hy.has_mom ? b[i] : 0.f;
      const float vi = fmaf(hy.f0, v0, hy.f1 * gi * gi);
      v[i] = vi;
      float rad = vi;
      if (hy.centered) {
        const float ai = lerp_torch(a0, gi, hy.f1, hy.f2);
        a[i] = ai;
        rad = fmaf(-ai, ai, vi);
      }
      float d = gi / (sqrtf(rad) + hy.eps);
      if (hy.has_mom) {
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
      const float gi = fmaf(hy.wd, pi, g[i]);
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
      const float gi = fmaf(hy.wd, pi, g[i]);
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
      const float gi = fmaf(hy.wd, pi, g[i]);
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
      const float gi = fmaf(hy.wd, pi, g[i]);
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
      const float gi = g[i], pi = p[i], s0 = ss[i];
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

template <int ALGO>
void launch(int cnt, const opt_table& tab, const opt_hyper& hy, const float* lr, const int64_t* step,
            const int32_t* iht_mode, float* scalars, hipStream_t s) {
  hipLaunchKernelGGL(optim_update_k<ALGO>, dim3(cnt), dim3(UPD_THREADS), 0, s, tab, hy, lr, (const long long*)step,
                     (const int*)iht_mode, scalars);
}

}  // namespace

int optim_update(const fastgrnn_optim_hyper& h, const fastgrnn_optim_seg* segs, int n_segs, const float* lr,
                 const int64_t* step, const int32_t* iht_mode, float* scalars, hipStream_t s) {
  opt_hyper hy = {};
  hy.wd = (float)h.weight_decay;
  switch (h.algo) {
    case RMSPROP:                                              // h = alpha, eps, momentum
      hy.f0 = (float)h.h[0];
      hy.f1 = (float)(1.0 - h.h[0]);
      hy.f2 = 1.f - hy.f1;
      hy.f3 = (float)h.h[2];
      hy.eps = (float)h.h[1];
      hy.centered = h.flags & 1;
      hy.has_mom = h.h[2] > 0.0;
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
  for (int s0 = 0; s0 < n_segs; s0 += FASTGRNN_UPDATE_MAX_SEGS) {
    const int cnt = n_segs - s0 < FASTGRNN_UPDATE_MAX_SEGS ? n_segs - s0 : FASTGRNN_UPDATE_MAX_SEGS;
    opt_table tab = {};
    for (int k = 0; k < cnt; ++k) {
      const fastgrnn_optim_seg& a = segs[s0 + k];
      opt_seg& d = tab.seg[k];
      d.p = reinterpret_cast<float*>(a.param);
      d.g = reinterpret_cast<const float*>(a.grad);
      d.s0 = reinterpret_cast<float*>(a.state[0]);
      d.s1 = reinterpret_cast<float*>(a.state[1]);
      d.s2 = reinterpret_cast<float*>(a.state[2]);
      d.sup = a.support;
      d.n = (int)a.n;
      d.keep_rank = (int)a.keep_rank;
      d.iht = a.iht != 0;
    }
    switch (h.algo) {
      case RMSPROP: launch<RMSPROP>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
      case ADAGRAD: launch<ADAGRAD>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
      case ADADELTA: launch<ADADELTA>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
      case ADAMAX: launch<ADAMAX>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
      case ASGD: launch<ASGD>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
      default: launch<RPROP>(cnt, tab, hy, lr, step, iht_mode, scalars, s); break;
    }
  }
  return launch_status();
}

}  // namespace fastgrnn
