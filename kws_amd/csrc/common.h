// Shared device helpers and internal launcher declarations for libfastgrnn_hip.so.
// gfx950 only; see include/fastgrnn_hip.h for the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/fastgrnn_hip.h"

namespace fastgrnn {

// ---- nonlinearities (reference table: rnn.py:40-67; device forms .cu:17-40) -------------
template <typename T> __device__ __forceinline__ T sigmoid_acc(T a);
template <> __device__ __forceinline__ float sigmoid_acc<float>(float a) { return 1.0f / (1.0f + expf(-a)); }
template <> __device__ __forceinline__ double sigmoid_acc<double>(double a) { return 1.0 / (1.0 + exp(-a)); }
template <typename T> __device__ __forceinline__ T tanh_acc(T a);
template <> __device__ __forceinline__ float tanh_acc<float>(float a) { return tanhf(a); }
template <> __device__ __forceinline__ double tanh_acc<double>(double a) { return tanh(a); }

template <typename T> __device__ __forceinline__ T act(T a, int nl) {
  switch (nl) {
    case FASTGRNN_NL_SIGMOID: return sigmoid_acc<T>(a);
    case FASTGRNN_NL_RELU: return a > T(0) ? a : T(0);
    case FASTGRNN_NL_TANH: return tanh_acc<T>(a);
    case FASTGRNN_NL_QUANT_TANH: return a > T(1) ? T(1) : (a < T(-1) ? T(-1) : a);
    case FASTGRNN_NL_QUANT_SIGM: { T v = (a + T(1)) / T(2); return v > T(1) ? T(1) : (v < T(0) ? T(0) : v); }
    default: { T v = (a + T(2)) / T(4); return v > T(1) ? T(1) : (v < T(0) ? T(0) : v); }
  }
}

// derivative expressed through the OUTPUT y, as the reference kernels do (.cu:27-40).
// tanh uses 1-y^2 (the reference's unrolled tanh-gate backward wrongly uses d_sigmoid,
// .cu:519-521; not reproduced).  relu tests y > 0 (== .cu:33-35 where differentiable).
template <typename T> __device__ __forceinline__ T dact(T y, int nl) {
  switch (nl) {
    case FASTGRNN_NL_SIGMOID: return (T(1) - y) * y;
    case FASTGRNN_NL_RELU: return y > T(0) ? T(1) : T(0);
    case FASTGRNN_NL_TANH: return T(1) - y * y;
    case FASTGRNN_NL_QUANT_TANH: return (y < T(1) && y > T(-1)) ? T(1) : T(0);
    case FASTGRNN_NL_QUANT_SIGM: return (y < T(1) && y > T(0)) ? T(0.5) : T(0);
    default: return (y < T(1) && y > T(0)) ? T(0.25) : T(0);
  }
}

static inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
// bytes per element of the sequences x / hs / grad_hs / d_x
static inline size_t seq_esz(const fastgrnn_desc& d) { return d.dtype == FASTGRNN_BF16_IO ? 2 : 4; }

// the status of a launcher that has enqueued its kernels
static inline int launch_status() { return hipGetLastError() == hipSuccess ? FASTGRNN_OK : FASTGRNN_ERR_LAUNCH; }

// Every call with a workspace has ONE layout function that walks its regions with a Carve (256-byte aligned each):
// given NULL it yields the byte count (off) and NULL pointers, given the caller's pointer the typed pointers.  The size
// query and the launcher both call it; nobody else computes an offset.
struct Carve {
  char* base;
  size_t off = 0;
  explicit Carve(void* b) : base((char*)b) {}
  template <typename T> T* take(size_t n) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(n * sizeof(T));
    return r;
  }
};

// ---- internal launchers (implemented in kernels_generic.hip / kernels_mfma.hip) ---------
size_t generic_forward_ws(const fastgrnn_desc& d);
size_t generic_backward_ws(const fastgrnn_desc& d);
// the generic scan of d in that direction (0 forward, 1 backward) fits its dynamic LDS; where it does not, no kernel
// runs d in that direction (kernel path -1) and the launcher refuses before it launches anything
bool generic_lds_fits(const fastgrnn_desc& d, int direction);
// sg, sc (FASTGRNN_FLAG_PREACT_AFFINE): [H] per-unit scales of the pre-activation in front of the gate and the
// update nonlinearity, in the parameter dtype; NULL for the plain cell
int generic_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0,
                    void* hs, void* zs, void* cs, void* ws, hipStream_t s, const void* sg = nullptr,
                    const void* sc = nullptr);
int generic_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x,
                     const void* hs, const void* zs, const void* cs, const void* h0,
                     const fastgrnn_grads& g, void* ws, hipStream_t s);

// C[M,N] = A[:, :M]^T . B[:, :N] over R rows (deterministic split-K); rows of B below shiftB come from
// B0, the rest from B1.  part: tn_gemm_f32_ws(R, M, N) bytes of workspace.
size_t tn_gemm_f32_ws(size_t R, int M, int N);
void tn_gemm_f32(size_t R, int M, int N, const float* A, int lda, const float* B0, const float* B1, size_t shiftB,
                 int ldb, float* part, float* C, hipStream_t s);

bool mfma_supported(const fastgrnn_desc& d, int direction);
size_t mfma_forward_ws(const fastgrnn_desc& d);
size_t mfma_backward_ws(const fastgrnn_desc& d);
int mfma_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0,
                 void* hs, void* zs, void* cs, void* ws, hipStream_t s);
int mfma_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x,
                  const void* hs, const void* zs, const void* cs, const void* h0,
                  const fastgrnn_grads& g, void* ws, hipStream_t s);

// split-precision (3 x bf16 planes, 6 MFMA terms) scans on the bf16 matrix pipe: kernel path 2.  Its cell families are
// the rows of ONE ordered table (family_of, kernels_split.hip: the first row whose shape holds, NULL where path 2 has
// none); every query and call below is a lookup in that row.
// fastgrnn_hip_forward_windows: utterance b is the T consecutive rows from row start[b] of a frame pool [rows, F]
// (x then points at the pool); start: [B] int32 on the device, 0 <= start[b] <= rows - T
struct window_src { const int32_t* start; size_t rows; };
struct family {
  bool (*shape)(const fastgrnn_desc& d);
  bool (*supported)(const fastgrnn_desc& d, int direction);
  size_t (*forward_ws)(const fastgrnn_desc& d);
  size_t (*backward_ws)(const fastgrnn_desc& d);
  // sg, sc: FASTGRNN_FLAG_PREACT_AFFINE (affine_supported); win: the windowed calls (windows_supported)
  int (*forward)(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0, void* hs, void* zs,
                 void* cs, void* ws, hipStream_t s, const float* sg, const float* sc, const window_src* win);
  int (*backward)(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x, const void* hs,
                  const void* zs, const void* cs, const void* h0, const fastgrnn_grads& g, void* ws, hipStream_t s);
  size_t (*windows_ws)(const fastgrnn_desc& d, size_t pool_rows);   // NULL: the windowed forward needs no workspace
  bool forward_ws_optional;   // the forward workspace is only used when z_s is NULL
  bool dx_optional;           // d_x is a GEMM of its own behind the scan: the backward accepts d_x == NULL
};
const family* family_of(const fastgrnn_desc& d);
// dense H = 256 with F = 32 / 64 / 128 (kernels_h256.hip); H = 256 / F = 32 with both ranks in 1..16 (kernels_lowrank.hip);
// every other factorised cell on a dense shape, multiplied out per call (kernels_densify.hip); the two dense H = 128
// rows, F = 64 / 128 / 256 and F = 32, are kernels_split.hip's own
const family& h256_family();
const family& lowrank_family();
const family& densified_family();

bool split_supported(const fastgrnn_desc& d, int direction);
size_t split_forward_ws(const fastgrnn_desc& d);
size_t split_backward_ws(const fastgrnn_desc& d);
bool split_dx_skippable(const fastgrnn_desc& d);          // d_x == NULL under FASTGRNN_FLAG_NO_INPUT_GRAD (beyond family::dx_optional)
// the per-unit scaled forward (sg, sc non-NULL, zs = cs = NULL) on the shapes affine_supported() admits
bool affine_supported(const fastgrnn_desc& d);
bool windows_supported(const fastgrnn_desc& d);                  // the windowed scans hold this cell (path 2 only)
size_t windows_ws(const fastgrnn_desc& d, size_t pool_rows);
// fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows: d carries FASTGRNN_FLAG_BATCH_MAJOR and (backward)
// FASTGRNN_FLAG_GRAD_LAST at most; the calls run it with FASTGRNN_FLAG_SAVE_PREACT added.  Where no scan reads the pool
// in place (every backward; the H = 128 forward) the windows are gathered into the call's workspace and the existing
// route runs on that copy.
bool train_windows_supported(const fastgrnn_desc& d);
size_t train_windows_forward_ws(const fastgrnn_desc& d, size_t pool_rows);
size_t train_windows_backward_ws(const fastgrnn_desc& d);
int split_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* x, const void* h0,
                  void* hs, void* zs, void* cs, void* ws, hipStream_t s, const void* sg = nullptr,
                  const void* sc = nullptr, const window_src* win = nullptr);
int split_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const void* ghs, const void* x,
                   const void* hs, const void* zs, const void* cs, const void* h0,
                   const fastgrnn_grads& g, void* ws, hipStream_t s, const window_src* win = nullptr);

// batched split-precision GEMMs around the scans (kernels_gemm.hip)
//   rows_gemm:   C[R,N] = A[R,K] . Wt^T, Wt[n][k] = trans_w ? W[k*N + n] : W[n*K + k]; A / C may be bf16 sequences
//   tn_gemm_big: C[M,N] (row stride ldc) = A[R,M]^T . B[R,N]; rows of B below shiftB come from B0, the rest from B1
//                shifted down by shiftB rows; part: tn_gemm_big_ws(R, M, N) bytes (bf_b with 0 < shiftB < R:
//                tn_gemm_big_ws(R, M, N, shiftB) -- the head and the body are cut into chunks independently).  The query
//                and both runs cut the rows with one plan (tnb_plan).
bool rows_gemm_supported(int N, int K, bool trans_w);
int rows_gemm(size_t R, int N, int K, bool trans_w, const void* A, const float* W, void* C, bool bf_in, bool bf_out,
              hipStream_t s);
// ... with A the data loader's [B,K,T] frames read in place (fp32; N = 128 / 256 of the wide layers) and row (b, t) of C
// stored at row t * cT + b * cB: the same bits as rows_gemm on the time-major copy
int rows_gemm_bft(int B, int T, int N, int K, const float* A, const float* W, float* C, size_t cT, size_t cB, hipStream_t s);
// the windows of a frame pool as a copy of x (fastgrnn_hip_backward_windows): row (t, b) = pool row start[b] + t, out
// [T,B,F] or, batch_major, [B,T,F]; F = 32 / 64
int gather_windows(int T, int B, int F, bool batch_major, const float* pool, const int32_t* start, float* out,
                   hipStream_t s);
size_t tn_gemm_big_ws(size_t R, int M, int N, size_t bf_shiftB = 0);
int tn_gemm_big_run(size_t R, int M, int N, const float* A, int lda, const float* B0, const void* B1, size_t shiftB,
                    int ldb, float* part, float* C, int ldc, hipStream_t s, bool bf_b = false);   // bf_b: B1 holds bf16
// ... with row r of B = B0[r / period] where r is a multiple of period, else B1[r - 1] (N = 256 only)
int tn_gemm_big_run_periodic(size_t R, int M, int N, const float* A, int lda, const float* B0, const void* B1, size_t period,
                             int ldb, float* part, float* C, int ldc, hipStream_t s, bool bf_b = false);
// [B,F,T] frames (FASTGRNN_FLAG_X_BFT) <-> time-major [T,B,F] rows (kernels_lowrank.hip): F = 32 with 2- or 4-byte
// elements, F = 64 / 128 / 256 with 4-byte ones
int bft_transpose_run(int B, int T, int F, size_t esize, const void* src, void* dst, bool to_time_major, hipStream_t s);

// A backward whose scan leaves d_pre[T*B, H] behind (dense H = 128 with a wide input, dense H = 256).  Workspace: the
// workgroups' slabs, d_pre + 16 sink rows for the lanes beyond a ragged batch, the partial sums of the weight-gradient
// GEMMs (du_gemm: dU is one; bf16 sequences split it at the B rows of h0), under FASTGRNN_FLAG_X_BFT a time-major copy
// of x.  dpre_bwd_tail: dW = d_pre^T . X, where g.d_x is wanted d_x = d_pre . W, the [B,F,T] transposes around them.
struct DpreBwdWs { float *part, *dpre, *tn, *xtm; size_t bytes; };
DpreBwdWs dpre_bwd_ws(const fastgrnn_desc& d, size_t slab_floats, bool du_gemm, void* base);
int dpre_bwd_tail(const fastgrnn_desc& d, const float* dpre, float* tn, float* xtm, const void* x, const void* w,
                  const fastgrnn_grads& g, hipStream_t s);

// FASTGRNN_FLAG_ZERO_EXTEND (kernels_zext.hip): the cell d run as the padded cell e (e.H, e.F = Hp, Fp; a path-2
// descriptor) -- padded copies of the operands, the split-precision code on them, the results compacted back
size_t zext_forward_ws(const fastgrnn_desc& d, const fastgrnn_desc& e);
size_t zext_backward_ws(const fastgrnn_desc& d, const fastgrnn_desc& e);
size_t zext_saved_bytes(const fastgrnn_desc& d, const fastgrnn_desc& e);
int zext_forward(const fastgrnn_desc& d, const fastgrnn_desc& e, const fastgrnn_params& p, const void* x,
                 const void* h0, void* hs, void* zs, void* ws, hipStream_t s);
int zext_backward(const fastgrnn_desc& d, const fastgrnn_desc& e, const fastgrnn_params& p, const void* ghs,
                  const void* x, const void* hs, const void* zs, const void* h0, const fastgrnn_grads& g, void* ws,
                  hipStream_t s);

// classifier head on the last state: Linear + log_softmax + NLL, forward and backward (kernels_head.hip)
bool head_supported(int B, int H, int C);
size_t head_ws_bytes(int B, int H, int C);
int head_xent(int B, int H, int C, const void* h_last, const void* fc_w, const void* fc_b, const void* labels,
              void* loss, void* logp, void* d_h, void* d_w, void* d_b, void* ws, hipStream_t s);
// ... its inference counterpart: scores (logp may be NULL), pred = argmax of the logits, and with labels the count of
// pred == labels in n_correct[1] (labels NULL: neither ws nor n_correct is touched); the detector's majority vote
size_t head_predict_ws_bytes(int B);
int head_predict(int B, int H, int C, const void* h_last, const void* fc_w, const void* fc_b, const void* labels,
                 void* logp, int32_t* pred, int32_t* n_correct, void* ws, hipStream_t s);
bool vote_supported(int K);
int vote_windows(int S, int Nw, int K, int M, const int32_t* pred, int32_t* majority, int32_t* event, hipStream_t s);

// optimizer step + IHT phase for every parameter tensor (kernels_update.hip), for either public pair of structures:
// fastgrnn_update_hyper / _seg (Adam, SGD) or fastgrnn_optim_hyper / _seg (the other six rules; scalars is ASGD's).
// Arguments already checked, segs on the host
template <typename Hyper, typename Seg>
int update_step(const Hyper& h, const Seg* segs, int n_segs, const float* lr, const int64_t* step,
                const int32_t* iht_mode, float* scalars, hipStream_t s);

// the gradient guard (kernels_guard.hip): the global norm, the clipping coefficient and the skip decision into *state,
// and update_step under it -- the step count, the coefficient and the decision are read from *guard.  Arguments
// already checked, segs on the host
size_t grad_guard_ws_bytes(int n_segs);
int grad_guard_run(const fastgrnn_guard_seg* segs, int n_segs, double max_norm, int flags, fastgrnn_guard_state* state,
                   void* workspace, hipStream_t s);
template <typename Hyper, typename Seg>
int update_step_guarded(const Hyper& h, const Seg* segs, int n_segs, const float* lr, const fastgrnn_guard_state* guard,
                        const int32_t* iht_mode, float* scalars, hipStream_t s);

// MFCC + delta features from raw audio (kernels_mfcc.hip); arguments already checked
size_t mfcc_tables_bytes();
int mfcc_init_tables(void* tables, hipStream_t s);
int mfcc_run(const fastgrnn_mfcc_desc& d, const void* audio, const int32_t* lengths, const void* tables, const float* mean,
             const float* stdv, void* feats, hipStream_t s);
// ... for the overlapping clips of one recording, its frames computed once (kernels_mfcc_stream.hip)
size_t mfcc_stream_ws_bytes(const fastgrnn_mfcc_stream_desc& d);
int mfcc_stream_frames_run(const fastgrnn_mfcc_stream_desc& d, const void* audio, const void* tables, void* ws,
                           hipStream_t s);
int mfcc_stream_clips_run(const fastgrnn_mfcc_stream_desc& d, const void* audio, const void* tables, void* ws,
                          const float* mean, const float* stdv, void* feats, hipStream_t s);
// ... reading an audio bank through augmentation records, and the records' draw (kernels_augment.hip)
int mfcc_augment_run(const fastgrnn_mfcc_desc& d, const fastgrnn_mfcc_bank& bank, const void* audio, const int32_t* lengths,
                     const void* noise, const int32_t* noise_lengths, const fastgrnn_mfcc_aug* aug, const void* tables,
                     const float* mean, const float* stdv, void* feats, hipStream_t s);
int augment_draw_run(int B, uint64_t seed, const int64_t* step, const int32_t* index, const fastgrnn_augment_ranges& r,
                     int n_noise, int noise_len_max, const int32_t* noise_lengths, fastgrnn_mfcc_aug* aug, hipStream_t s);

// the batch, the learning rate and the IHT phase of an iteration from the step count (kernels_schedule.hip);
// arguments already checked
int train_schedule_run(const fastgrnn_schedule_desc& d, const int64_t* step, int32_t* index, float* lr,
                       int32_t* iht_mode, int64_t* where, hipStream_t s);

// the same with the rolling position, and the hidden-state bags' scatter and gather of an iteration
// (kernels_rolling.hip); arguments already checked
int train_schedule_rolling_run(const fastgrnn_schedule_desc& d, const fastgrnn_rolling_desc& r, const int64_t* step,
                               int32_t* index, float* lr, int32_t* iht_mode, int64_t* where, hipStream_t s);
int rolling_exchange_run(const fastgrnn_schedule_desc& d, const fastgrnn_rolling_desc& r, const int64_t* step,
                         const float* const state[3], float* const bag[3], float* const h0[3], hipStream_t s);

// training-mode BatchNorm cell (kernels_bn_train.hip): FASTGRNN_FLAG_BN_TRAIN
bool bn_train_supported(const fastgrnn_desc& d);
size_t bn_train_forward_ws(const fastgrnn_desc& d);
size_t bn_train_backward_ws(const fastgrnn_desc& d);
int bn_train_forward(const fastgrnn_desc& d, const fastgrnn_params& p, const fastgrnn_bn_params& bn, const void* x,
                     const void* h0, void* hs, void* saved, void* stats, void* ws, hipStream_t s);
int bn_train_backward(const fastgrnn_desc& d, const fastgrnn_params& p, const fastgrnn_bn_params& bn,
                      const void* ghs, const void* x, const void* hs, const void* saved, const void* stats,
                      const void* h0, const fastgrnn_grads& g, const fastgrnn_bn_grads& bg, void* ws, hipStream_t s);

// test hook (kernels_debug.hip): fill every CU's LDS and vector registers with a bit pattern
int debug_poison(unsigned pattern, hipStream_t s);

namespace {
// Completion read (operand rule): ONE vector instruction the compiler cannot drop reads `v` -- an
// element of the youngest accumulator, or a sum of several: MFMAs retire in order, so once it has executed every MFMA
// issued before it has read its operands.  v_readfirstlane into a scalar register that an empty asm consumes: no
// branch, no memory instruction (the first form, `if (v == <never>) <store>`, put a conditional store into scan loops:
// second rule of 4.0).
__device__ __forceinline__ void completion_read(float v) {
  const int s = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v));
  asm volatile("" :: "s"(s));
}

// Second rule of DESIGN.md 4.0, by construction: no LDS write is pending when a conditional branch -- exec-masked or
// wave-uniform -- with a vector-memory instruction behind it is taken.  Placed in front of such regions where LDS
// writes precede them in the same loop iteration without a barrier in between.
__device__ __forceinline__ void lds_writes_landed() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

}  // namespace

}  // namespace fastgrnn
