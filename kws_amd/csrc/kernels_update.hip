// The end of a trainer iteration in one launch: optimizer.step() (trainClassifier.py:249) for every parameter tensor of
// a model, then the IHT phase on the W/U matrices (trainClassifier.py:251-259 -> utils.py:53-81).  gfx950 only.
// (No inline assembly of its own; lds_writes_landed() is common.h's one-instruction wait, which the second rule of
// DESIGN.md 4.0 asks for in any loop that mixes LDS operations with memory instructions.)
//   Adam:  torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay);  SGD: torch.optim.SGD with momentum,
//   dampening, nesterov, L2 weight decay.  fp32 operands, fp32 arithmetic; Adam's bias corrections in double.
//   IHT mode 1 (utils.hardThreshold): zero what lies strictly below the magnitude of 0-based rank keep_rank and record
//   the support; mode 2 (utils.supportBasedThreshold): zero what the recorded support excludes.
// One workgroup of UPD_THREADS per parameter tensor ("segment"), no communication between workgroups.  Thread t owns
// elements t, t + UPD_THREADS, ... in EVERY phase, so a thread only ever USES values it stored itself (the clamped loads
// of a ragged last iteration fetch element n-1, whoever owns it, and discard it).  lr, the step
// count and the IHT mode are device scalars: a captured graph of the call serves a whole training run.
// The threshold is found exactly by radix select on the magnitudes' bit patterns (for non-NaN fp32, bits & 0x7fffffff
// orders as an unsigned integer): four 8-bit passes from the top, each a 256-bin histogram in LDS of the elements that
// still match the digits chosen so far.  Integer LDS atomics: the counts do not depend on arrival order.
// Latency-bound byte work on at most 32 CUs (a model has 6-14 tensors of at most 256x256): what it saves is launches,
// not bandwidth.
// The threshold phase is iht_select.h: kernels_optim.hip (the other six rules of torch.optim) runs the same one.
#include "iht_select.h"

namespace fastgrnn {
namespace {

struct upd_seg {                 // one row of the table that rides in the kernel arguments (56 bytes; 32 rows: 1792)
  float* p;
  const float* g;
  float* s0;                     // Adam: exp_avg; SGD: momentum buffer
  float* s1;                     // Adam: exp_avg_sq
  unsigned char* sup;            // [n] bytes, IHT segments only
  int n, keep_rank, iht, pad;
};
struct upd_table { upd_seg seg[FASTGRNN_UPDATE_MAX_SEGS]; };

struct upd_hyper {
  double beta1, beta2;           // Adam: for the bias corrections
  float b1, omb1, b2, omb2;      // Adam: beta1, 1-beta1, beta2, 1-beta2;  SGD: b1 = momentum, omb1 = 1-dampening
  float eps, wd;
  int algo, nesterov;
};

__global__ __launch_bounds__(UPD_THREADS) void train_update_k(upd_table tab, upd_hyper hy, const float* __restrict__ lr_p,
                                                              const long long* __restrict__ step_p,
                                                              const int* __restrict__ mode_p) {
  __shared__ unsigned hist[256];
  __shared__ float s_bc[2];        // Adam: lr / (1 - beta1^t), sqrt(1 - beta2^t)
  __shared__ unsigned s_sel[2];    // radix select: digits chosen so far, rank left among the elements that match them
  const int tid = threadIdx.x;
  const upd_seg sg = tab.seg[blockIdx.x];
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
  if (hy.algo == 0) {
    if (tid == 0) {
      const double bc1 = 1.0 - ipow(hy.beta1, step), bc2 = 1.0 - ipow(hy.beta2, step);
      s_bc[0] = (float)((double)lr / bc1);
      s_bc[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    const float step_size = s_bc[0], bc2_sqrt = s_bc[1];
    float* m = sg.s0;
    float* v = sg.s1;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, g[i]);
      const float mi = fmaf(hy.b1, m[i], hy.omb1 * gi);
      const float vi = fmaf(hy.b2, v[i], hy.omb2 * gi * gi);
      const float denom = sqrtf(vi) / bc2_sqrt + hy.eps;
      float pn = fmaf(-step_size, mi / denom, pi);
      m[i] = mi;
      v[i] = vi;
      if (mask_now && sg.sup[i] == 0) pn = 0.f;
      p[i] = pn;
      if (sup_now) sg.sup[i] = pn != 0.f ? 1 : 0;
    }
  } else {
    float* b = sg.s0;
    const bool first = step <= 1, has_mom = hy.b1 != 0.f;
    for (int i = tid; i < n; i += UPD_THREADS) {
      const float pi = p[i];
      const float gi = fmaf(hy.wd, pi, g[i]);
      float d = gi;
      if (has_mom) {                                           // (torch keeps no buffer, and ignores dampening, without momentum)
        const float bi = first ? gi : fmaf(hy.b1, b[i], hy.omb1 * gi);
        b[i] = bi;
        d = hy.nesterov ? fmaf(hy.b1, bi, gi) : bi;
      }
      float pn = fmaf(-lr, d, pi);
      if (mask_now && sg.sup[i] == 0) pn = 0.f;
      p[i] = pn;
      if (sup_now) sg.sup[i] = pn != 0.f ? 1 : 0;
    }
  }
  if (mode != 1 || sg.keep_rank <= 0) return;                  // (uniform over the workgroup: the barriers below are safe)

  // ---- b. hard threshold: strictly below the magnitude of 0-based rank keep_rank goes, the support is recorded
  iht_threshold(p, sg.sup, n, sg.keep_rank, hist, s_sel);
}

}  // namespace

int train_update(const fastgrnn_update_hyper& h, const fastgrnn_update_seg* segs, int n_segs, const float* lr,
                 const int64_t* step, const int32_t* iht_mode, hipStream_t s) {
  upd_hyper hy;
  hy.beta1 = h.beta1_or_momentum;
  hy.beta2 = h.beta2_or_dampening;
  hy.b1 = (float)h.beta1_or_momentum;
  hy.omb1 = (float)(1.0 - (h.algo == 0 ? h.beta1_or_momentum : h.beta2_or_dampening));
  hy.b2 = (float)h.beta2_or_dampening;
  hy.omb2 = (float)(1.0 - h.beta2_or_dampening);
  hy.eps = (float)h.eps;
  hy.wd = (float)h.weight_decay;
  hy.algo = h.algo;
  hy.nesterov = h.nesterov;
  for (int s0 = 0; s0 < n_segs; s0 += FASTGRNN_UPDATE_MAX_SEGS) {
    const int cnt = n_segs - s0 < FASTGRNN_UPDATE_MAX_SEGS ? n_segs - s0 : FASTGRNN_UPDATE_MAX_SEGS;
    upd_table tab = {};
    for (int k = 0; k < cnt; ++k) {
      const fastgrnn_update_seg& a = segs[s0 + k];
      upd_seg& d = tab.seg[k];
      d.p = reinterpret_cast<float*>(a.param);
      d.g = reinterpret_cast<const float*>(a.grad);
      d.s0 = reinterpret_cast<float*>(a.state0);
      d.s1 = reinterpret_cast<float*>(a.state1);
      d.sup = a.support;
      d.n = (int)a.n;
      d.keep_rank = (int)a.keep_rank;
      d.iht = a.iht != 0;
    }
    hipLaunchKernelGGL(train_update_k, dim3(cnt), dim3(UPD_THREADS), 0, s, tab, hy, lr, (const long long*)step,
                       (const int*)iht_mode);
  }
  return launch_status();
}

}  // namespace fastgrnn
