// The guard between backward and the optimizer step: the global gradient norm, the clipping coefficient of
// torch.nn.utils.clip_grad_norm_ and the rejection of a step with a non-finite gradient, all on the device, and the
// eight update rules under it (fastgrnn_hip_grad_guard, fastgrnn_hip_train_update_guarded,
// fastgrnn_hip_optim_update_guarded; include/fastgrnn_hip.h spells the semantics out).  gfx950 only; no inline assembly.
//   grad_sumsq_k          one workgroup of GRD_THREADS per gradient tensor ("segment"), the segment table in the kernel
//                         arguments, one launch per FASTGRNN_UPDATE_MAX_SEGS segments as update_k: the segment's sum of
//                         g^2 in double (the square of an fp32 value is exact in double, so a product-and-add and a
//                         fused one round alike), one double per segment into the workspace.
//   guard_finish_k        one workgroup: adds the partials in index order, forms norm, coef and skip, adds one to
//                         `applied` or to `skipped` and writes the 32-byte state.
//   guarded_update_k<A>   kernels_update.hip's kernel with UPDATE_GUARD 1: update_k's rule on g * coef at step `applied`, or the
//                         identity on a skipped step.
// The order of every sum is a function of the shapes alone -- thread t adds elements t, t + 1024, ... four at a time
// (the last round's loads are clamped to element n-1 and their squares replaced by 0: no branch around a load), a
// wave adds its 64 lanes as a shuffle tree, thread 0 adds the 16 wave sums and, in the second kernel, the segments in
// index order -- and nothing is accumulated with atomics: the same gradients give the same bits.
// Both rules of DESIGN.md 4.0: there is no MFMA here, and the only LDS writes (the 16 wave sums; the update kernel's, as in
// update_k) are followed by a workgroup barrier before any branch that has a memory instruction behind it.
#define UPDATE_GUARD 1
#include "kernels_update.hip"

namespace fastgrnn {
namespace {

constexpr int GRD_THREADS = 1024;

struct grd_seg {                 // one row of the table in the kernel arguments (16 bytes; 32 rows: 512)
  const float* g;
  int n, pad;
};
struct grd_table { grd_seg seg[FASTGRNN_UPDATE_MAX_SEGS]; };

__global__ __launch_bounds__(GRD_THREADS) void grad_sumsq_k(grd_table tab, double* __restrict__ partial) {
  __shared__ double s_wave[GRD_THREADS / 64];
  const int tid = threadIdx.x;
  const grd_seg sg = tab.seg[blockIdx.x];
  const int n = sg.n;
  const float* __restrict__ g = sg.g;
  double a = 0.0;
  for (int i0 = tid; i0 < n; i0 += 4 * GRD_THREADS) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = g[min(i0 + j * GRD_THREADS, n - 1)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)v[j];
      a += i0 + j * GRD_THREADS < n ? d * d : 0.0;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d);   // lane 0: the wave's sum, as a fixed tree
  if ((tid & 63) == 0) s_wave[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < GRD_THREADS / 64; ++w) t += s_wave[w];
    partial[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void guard_finish_k(const double* __restrict__ partial, int n_segs, double max_norm,
                                                     int skip_nonfinite, fastgrnn_guard_state* state) {
  if (threadIdx.x != 0) return;
  double S = 0.0;
  for (int k = 0; k < n_segs; ++k) S += partial[k];
  const double norm = sqrt(S);
  const bool skip = skip_nonfinite && !isfinite(S);            // (S is non-finite iff some gradient element is)
  float coef = 1.f;
  if (max_norm < INFINITY) {
    // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0), which keeps a NaN
    const double c = max_norm / (norm + 1e-6);
    coef = (float)(c > 1.0 ? 1.0 : c);
  }
  const long long applied = state->applied, skipped = state->skipped;
  state->norm = (float)norm;
  state->coef = skip ? 0.f : coef;
  state->skip = skip ? 1 : 0;
  state->reserved = 0;
  state->applied = applied + (skip ? 0 : 1);
  state->skipped = skipped + (skip ? 1 : 0);
}

}  // namespace

size_t grad_guard_ws_bytes(int n_segs) {
  return n_segs < 1 ? 0 : ((size_t)n_segs * sizeof(double) + 255) / 256 * 256;
}

int grad_guard_run(const fastgrnn_guard_seg* segs, int n_segs, double max_norm, int flags, fastgrnn_guard_state* state,
                   void* workspace, hipStream_t s) {
  double* partial = reinterpret_cast<double*>(workspace);
  for (int s0 = 0; s0 < n_segs; s0 += FASTGRNN_UPDATE_MAX_SEGS) {
    const int cnt = n_segs - s0 < FASTGRNN_UPDATE_MAX_SEGS ? n_segs - s0 : FASTGRNN_UPDATE_MAX_SEGS;
    grd_table tab = {};
    for (int k = 0; k < cnt; ++k) {
      tab.seg[k].g = reinterpret_cast<const float*>(segs[s0 + k].grad);
      tab.seg[k].n = (int)segs[s0 + k].n;
    }
    hipLaunchKernelGGL(grad_sumsq_k, dim3(cnt), dim3(GRD_THREADS), 0, s, tab, partial + s0);
  }
  hipLaunchKernelGGL(guard_finish_k, dim3(1), dim3(64), 0, s, (const double*)partial, n_segs, max_norm,
                     flags & FASTGRNN_GUARD_SKIP_NONFINITE, state);
  return launch_status();
}

template <typename Hyper, typename Seg>
int update_step_guarded(const Hyper& h, const Seg* segs, int n_segs, const float* lr, const fastgrnn_guard_state* guard,
                        const int32_t* iht_mode, float* scalars, hipStream_t s) {
  update_launches(h, segs, n_segs, [&](auto algo, int cnt, const upd_table& tab, const upd_hyper& hy) {
    hipLaunchKernelGGL(guarded_update_k<decltype(algo)::value>, dim3(cnt), dim3(UPD_THREADS), 0, s, tab, hy, lr, guard,
                       (const int*)iht_mode, scalars);
  });
  return launch_status();
}

template int update_step_guarded(const fastgrnn_update_hyper&, const fastgrnn_update_seg*, int, const float*,
                                 const fastgrnn_guard_state*, const int32_t*, float*, hipStream_t);
template int update_step_guarded(const fastgrnn_optim_hyper&, const fastgrnn_optim_seg*, int, const float*,
                                 const fastgrnn_guard_state*, const int32_t*, float*, hipStream_t);

}  // namespace fastgrnn
