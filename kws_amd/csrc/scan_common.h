// What the scans of kernel paths 1 and 2 and the GEMMs around them share and that has nothing to do with the bf16 / fp16
// plane split (split_common.h): the activations, the 16-byte accesses, the LDS barrier, and the fixed-order reduction
// that ends every backward.  gfx950 only.
#pragma once
#include "common.h"

namespace fastgrnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float LOG2E = 1.4426950408889634f;

// v_exp_f32 / v_rcp_f32 are 1-ulp; absolute error of these forms is < 3e-7 (the parity
// bar is 1e-5).  Saturation is exact: exp2(+inf) -> rcp(inf) = 0.
__device__ __forceinline__ float fsigmoid(float a) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * a));
}
__device__ __forceinline__ float ftanh(float a) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f((2.0f * LOG2E) * a));
}
// gate nonlinearities: the reference's GPU table {sigmoid, relu, tanh} (rnn.py:478) and, on the 8-wave dense
// kernels, the CPU cell's quantised family (rnn.py:53-60); derivatives through the output as in
// common.h / .cu:27-40
template <int GATE> __device__ __forceinline__ float gate_act(float a) {
  if (GATE == FASTGRNN_NL_SIGMOID) return fsigmoid(a);
  if (GATE == FASTGRNN_NL_RELU) return a > 0.0f ? a : 0.0f;
  if (GATE == FASTGRNN_NL_QUANT_TANH) return fminf(fmaxf(a, -1.0f), 1.0f);
  if (GATE == FASTGRNN_NL_QUANT_SIGM) return fminf(fmaxf((a + 1.0f) * 0.5f, 0.0f), 1.0f);
  if (GATE == FASTGRNN_NL_QUANT_SIGM4) return fminf(fmaxf((a + 2.0f) * 0.25f, 0.0f), 1.0f);
  return ftanh(a);
}
template <int GATE> __device__ __forceinline__ float gate_dact(float y) {
  if (GATE == FASTGRNN_NL_SIGMOID) return (1.0f - y) * y;
  if (GATE == FASTGRNN_NL_RELU) return y > 0.0f ? 1.0f : 0.0f;
  if (GATE == FASTGRNN_NL_QUANT_TANH) return (y < 1.0f && y > -1.0f) ? 1.0f : 0.0f;
  if (GATE == FASTGRNN_NL_QUANT_SIGM) return (y < 1.0f && y > 0.0f) ? 0.5f : 0.0f;
  if (GATE == FASTGRNN_NL_QUANT_SIGM4) return (y < 1.0f && y > 0.0f) ? 0.25f : 0.0f;
  return 1.0f - y * y;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// Workgroup barrier for LDS hand-offs only.  __syncthreads() would also emit
// s_waitcnt vmcnt(0) and drain every in-flight global load/store each step; here only this
// wave's LDS traffic is waited for, so prefetches and stores stay in flight across steps.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- the fixed-order reduction -------------------------------------------------------------------------
// out[idx] = sum over k < n of *src(k, idx) for idx < ntot, the same bits on every run: the body of every kernel that
// adds up per-workgroup or per-chunk partial sums.  A block of 1024 threads owns 64 consecutive outputs; its 16
// wave-sized groups split the n partials 16 ways (group g takes k = g, g + 16, ...), W loads in flight per round, added
// as a balanced pairwise tree (the last round is guarded load by load); then 64 threads add the 16 group sums in the
// order of the groups and hand each total to put(idx, t).  W is part of every sum's bits: a caller keeps its W.
// What differs between the callers -- where partial k of output idx lies, where the total goes -- is in the two
// lambdas.
template <int W> __device__ __forceinline__ float pairwise_tree(const float* v) {
  if constexpr (W == 1) return v[0];
  else return pairwise_tree<W / 2>(v) + pairwise_tree<W / 2>(v + W / 2);
}
template <int W, typename Src, typename Put>
__device__ __forceinline__ void fixed_order_sum(int n, int ntot, Src src, Put put) {
  static_assert(W == 4 || W == 8, "a power of two: the tree is balanced");
  __shared__ float sm[16][64];
  const int o = threadIdx.x & 63, pid = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + o;
  float a = 0.f;
  if (idx < ntot) {
    for (int k0 = pid; k0 < n; k0 += 16 * W) {
      float v[W];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int k = k0 + 16 * j;
        v[j] = k < n ? *src(k, idx) : 0.f;
      }
      a += pairwise_tree<W>(v);
    }
  }
  sm[pid][o] = a;
  __syncthreads();
  if (pid == 0 && idx < ntot) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) t += sm[j][o];
    put(idx, t);
  }
}

// The chain rule of a raw scalar (.cu:116-117,544-545): the cell uses s = sigmoid(raw) = 1 / (1 + expf(-zeta[0])), and
// likewise for nu; t is the gradient with respect to s.
__device__ __forceinline__ float raw_scalar_grad(float t, const float* raw) {
  const float s = sigmoid_acc<float>(raw[0]);
  return t * s * (1.0f - s);
}

}  // namespace
}  // namespace fastgrnn
