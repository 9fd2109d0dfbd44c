/*
 * fastgrnn_hip.h -- C ABI of libfastgrnn_hip.so: the MI355X (gfx950) FastGRNN
 * recurrent cell, forward and backward, single-step and unrolled over T frames.
 *
 * This is the drop-in boundary for the reference's native operator module
 * `fastgrnn_cuda` (/root/reference cuda/fastgrnn_cuda.cpp:235-240), whose four
 * entry points -- forward, backward, forward_unroll, backward_unroll -- are the
 * only native calls on the hot path (called from rnn.py:894,903,910,955).
 *
 * Conventions (all taken from the reference boundary, file:line cited per item):
 *   - plain device pointers + sizes; no torch types; the library allocates
 *     NOTHING and never synchronises: the caller passes outputs and a workspace
 *     (size from the *_workspace_bytes queries) and a hipStream_t.  Kernels are
 *     launched on that stream; the stream's device must be current.
 *   - every tensor is dense row-major ("contiguous", fastgrnn_cuda.cpp:69-71).
 *   - weight layout is the CUDA classes' [out,in] (rnn.py:783-798):
 *       w:[H,F]  u:[H,H]  w1:[w_rank,F]  w2:[H,w_rank]  u1:[u_rank,H]  u2:[H,u_rank]
 *       pre = x . w^T + h . u^T            (.cu:356,361,368)
 *     low-rank is evaluated FACTORISED, (x.w1^T).w2^T + (h.u1^T).u2^T, the CPU
 *     cell's association order (rnn.py:280-287); w_rank/u_rank == 0 means dense
 *     and the unused pointers may be NULL (reference: torch.empty(0),
 *     rnn.py:783-798, .cu:138-139).
 *   - zeta and nu are RAW device scalars; sigmoid is applied inside
 *     (.cu:148-149,364-365) and d_zeta/d_nu are w.r.t. the raw values
 *     (.cu:116-117).
 *   - gate code table {sigmoid:0, relu:1, tanh:2} is rnn.py:478,751; codes 3..5
 *     add the CPU cell's quantTanh/quantSigm/quantSigm4 (rnn.py:53-60; kernel path 2 under
 *     FASTGRNN_FLAG_SAVE_PREACT for the dense H=128/F=32 shape, the generic scan otherwise).  The
 *     reference's CUDA path fixes the update nonlinearity to tanh (.cu:57);
 *     update_nl is exposed because the CPU cell allows it (rnn.py:292-293).
 *   - every function returns a fastgrnn_status; nonzero means nothing useful
 *     was launched (argument errors) or the launch itself failed.
 *   - re-entrant, no global mutable state; safe from the autograd worker thread.
 */
#ifndef FASTGRNN_HIP_H
#define FASTGRNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASTGRNN_HIP_ABI_VERSION 1

typedef enum fastgrnn_status {
  FASTGRNN_OK = 0,
  FASTGRNN_ERR_NULL_POINTER = 1,   /* a required pointer is NULL */
  FASTGRNN_ERR_BAD_SHAPE = 2,      /* T,B,F,H < 1, rank < 0, rank > dims, or size overflow */
  FASTGRNN_ERR_BAD_NONLINEARITY = 3,
  FASTGRNN_ERR_BAD_DTYPE = 4,
  FASTGRNN_ERR_WORKSPACE = 5,      /* workspace NULL/too small/misaligned (needs 256 B) */
  FASTGRNN_ERR_LAUNCH = 6,         /* hipGetLastError() != hipSuccess after a launch */
  FASTGRNN_ERR_UNSUPPORTED = 7
} fastgrnn_status;

typedef enum fastgrnn_dtype {
  FASTGRNN_F32 = 0,                /* mandatory type of the reference (AT_DISPATCH_FLOATING_TYPES, .cu:158) */
  FASTGRNN_F64 = 1,                /* gradcheck type of the reference dispatch */
  /* BASELINE config "bf16 with fp32 master grads" (new; the reference has no such type): the SEQUENCES
   * x, hs, grad_hs and d_x are bf16 (2 bytes per element); parameters, h0 / d_h0, the saved
   * pre-activation and every parameter gradient stay fp32, and so does all arithmetic (the state is
   * carried in fp32 and only its stored copy is rounded, to nearest even).  Kernel path 2 only, on the
   * shapes its table under fastgrnn_hip_kernel_path lists for bf16 sequences (dense H=128 with F=32/64/128/256,
   * dense H=256 with F=32/64/128, the low-rank H=256 scans); forward without gates or with
   * FASTGRNN_FLAG_SAVE_PREACT, backward with FASTGRNN_FLAG_SAVE_PREACT; anything else answers
   * FASTGRNN_ERR_UNSUPPORTED. */
  FASTGRNN_BF16_IO = 2
} fastgrnn_dtype;

typedef enum fastgrnn_nonlinearity {
  FASTGRNN_NL_SIGMOID = 0, FASTGRNN_NL_RELU = 1, FASTGRNN_NL_TANH = 2,       /* rnn.py:478 */
  FASTGRNN_NL_QUANT_TANH = 3, FASTGRNN_NL_QUANT_SIGM = 4, FASTGRNN_NL_QUANT_SIGM4 = 5 /* rnn.py:53-60 */
} fastgrnn_nonlinearity;

/* flags */
#define FASTGRNN_FLAG_FORCE_GENERIC 1u   /* bypass the MFMA-tiled kernels (testing / A-B) */
#define FASTGRNN_FLAG_FORCE_F32_MFMA 2u  /* use the fp32-MFMA scan instead of the split-precision one */
/* Training-only contract between forward_unroll and backward_unroll (kernel path 2 only): the
 * forward writes ONE auxiliary tensor, the pre-activation W.x_t + U.h_{t-1} (no bias), into z_s and
 * ignores c_s; the backward reads it from z_s (c_s ignored, may be NULL), recomputes z_t and
 * h_prime_t from it and therefore needs params->bias_gate / bias_update.  Saves one [T,B,H] write
 * and one read per step against the reference operator's (z_s, h_prime_s) pair. */
#define FASTGRNN_FLAG_SAVE_PREACT 4u
/* A/B only: run the dense H=128/F=32 split-precision forward in its older 4-wave shape (one wave per SIMD, two
 * row tiles per wave) instead of the default 8-wave one.  Same results to fp32 rounding.  Ignored by the other
 * shapes of kernel path 2. */
#define FASTGRNN_FLAG_FWD_4WAVE 8u
/* A/B only: run the dense H=128/F=32 backward without input gradient (FASTGRNN_FLAG_NO_INPUT_GRAD, d_x == NULL) in
 * its older 8-wave shape instead of the default 12-wave one (a helper wave per SIMD for the weight gradients; fp32
 * sequences, sigmoid / relu / tanh gate, tanh update).  The same bits in every output.  Ignored by every other call. */
#define FASTGRNN_FLAG_BWD_8WAVE 32u
/* Batch-major sequences (the trainer's batch_first layout, rnn.py:812-813,823-825): x, hs, z_s, c_s,
 * grad_hs and d_x are [B,T,.] instead of [T,B,.]; h0/d_h0 stay [B,H].  Kernel path 2 (dense H=128, dense H=256
 * with the limits of its table entry -- no bf16 backward -- and the low-rank H=256 scans) -- anything else answers
 * FASTGRNN_ERR_UNSUPPORTED and the caller transposes as the reference does.  Removes the transpose(0,1).contiguous() copies around the operator. */
#define FASTGRNN_FLAG_BATCH_MAJOR 16u
/* x and d_x are [B,F,T]: what the trainer's data loader delivers and permute(2,0,1)s into a [T,B,F] VIEW
 * (trainClassifier.py:204,299) that the reference then copies with .contiguous() (rnn.py:910).  Independent
 * of FASTGRNN_FLAG_BATCH_MAJOR (which then only governs hs, the saved tensor and grad_hs).  Kernel path 2:
 * dense H=128/F=32 (read and written in place; backward under FASTGRNN_FLAG_SAVE_PREACT); dense H=256/F=32 and the
 * low-rank H=256/F=32 scans through a time-major copy in the workspace (what the reference's .contiguous() makes,
 * without the tensor it keeps alive for the backward; low-rank backward under FASTGRNN_FLAG_SAVE_PREACT); the layers
 * whose frame product X.W^T is a GEMM of its own -- dense H=256 with F=64/128, dense H=128 with F=64/128/256, fp32
 * sequences, and the factorised cells multiplied out onto them: the forward's frame GEMM reads [B,F,T] in place (no
 * copy of x, no workspace for one; the same bits as on time-major frames), the backward takes a time-major copy of x
 * in its workspace (align256(T*B*F*4) bytes more) for the dW GEMM and transposes d_x, where wanted, back into the
 * caller's [B,F,T] tensor.  The backward with BOTH this flag and FASTGRNN_FLAG_BATCH_MAJOR is not on path 2 on the
 * H=256 and the wide H=128 shapes. */
#define FASTGRNN_FLAG_X_BFT 128u
/* A/B only: keep the forward's state product U.h on three bf16 planes (6 MFMAs per K-step) instead of the
 * default fp16 two-plane operands with a per-wave power-of-two scale of U (3 MFMAs per K-step). */
#define FASTGRNN_FLAG_FWD_BF16X3 64u
/* SURVEY 8(f) N2 -- the classifier's view of the LAST layer (model.py:227 reads hs[T-1] alone):
 *   GRAD_LAST  backward_unroll: grad_hs is [B,H], the gradient of the last state; every other step's is zero and
 *              is neither materialised nor read (a dense zero [T,B,H] is what autograd would otherwise write and the
 *              kernel read: 2 x 208 MB at B=4096).  hs, the saved tensors and every output keep their shapes.
 *   HS_LAST    forward_unroll (inference: z_s must be NULL): hs is [B,H] and receives h_T only (a separately
 *              compiled kernel variant: equal to the last row of the full forward to fp32 rounding).
 * Both: dense H=128 (F = 32 and the wide-input layers) and low-rank H=256/F=32, any sequence layout;
 * FASTGRNN_ERR_UNSUPPORTED otherwise. */
#define FASTGRNN_FLAG_GRAD_LAST 256u
#define FASTGRNN_FLAG_HS_LAST 512u
/* Eval-mode BatchNorm cell (the reference's FastGRNNBatchNorm, rnn.py:316-452, with its running statistics): a
 * per-unit scale of the pre-activation in front of each nonlinearity,
 *   z = gate(gate_scale . pre + bias_gate),  h' = update(update_scale . pre + bias_update),  pre = w.x + u.h
 * (elementwise scales, the four BatchNorm1d layers folded into w, u and the biases by the caller).  Only
 * fastgrnn_hip_forward_unroll_affine runs it; with this flag set fastgrnn_hip_kernel_path(d, 0) and
 * fastgrnn_hip_forward_workspace_bytes answer for that call, fastgrnn_hip_kernel_path(d, 1) is -1 (there is no
 * backward) and every other entry point answers FASTGRNN_ERR_UNSUPPORTED. */
#define FASTGRNN_FLAG_PREACT_AFFINE 1024u
/* Training-mode BatchNorm cell (the reference's FastGRNNBatchNorm, rnn.py:316-452, every BatchNorm1d in training
 * mode: batch statistics per frame, running statistics updated T times per call in frame order).  Only the
 * fastgrnn_hip_bn_train_* entry points below run it and they require this flag; every other entry point answers
 * FASTGRNN_ERR_UNSUPPORTED for a descriptor that carries it, fastgrnn_hip_kernel_path answers -1 and the two older
 * workspace queries answer 0.  Kernels: one launch per frame, workgroups split the batch and the last one to arrive
 * combines their per-unit partial sums in a fixed order (no float atomics: bitwise repeatable; no workgroup waits
 * for another); two reductions per frame in the forward (the statistics of uC, then of the sum that bn_gate and
 * bn_update normalise), one in the backward; fp32 operands, fp64 accumulation and statistics.  fastgrnn_hip_bn_train_supported lists the shapes. */
#define FASTGRNN_FLAG_BN_TRAIN 2048u
/* Zero-extension onto kernel path 2 (kernels_zext.hip).  A permission, not a demand: it takes effect only for a
 * descriptor that answers path 0 without it and whose padded form (below) answers path 2 -- for the backward, and for
 * a forward under FASTGRNN_FLAG_SAVE_PREACT, in both directions (the backward always runs under SAVE_PREACT on this
 * route).  In every other case the call behaves bit for bit as without the flag, and no call is refused because of it:
 * shapes already on path 2, fp32 H=64/F=32 (path 1), fp64, H or F beyond what the padding reaches,
 * FASTGRNN_FLAG_FORCE_GENERIC / FORCE_F32_MFMA / X_BFT / PREACT_AFFINE / BN_TRAIN, and a forward that passes the
 * reference's (z_s, h_prime_s) pair without FASTGRNN_FLAG_SAVE_PREACT.
 *   Padded shape: Hp = 128 for H <= 128, 256 for 129 <= H <= 256; Fp = the smallest of 32/64/128/256 that is >= F
 *   and puts the padded descriptor on path 2.  Ranks, gates, dtype (fp32 or bf16 sequences), BATCH_MAJOR, GRAD_LAST
 *   and HS_LAST carry over; factorised cells are padded factor by factor (W1 [r,Fp], W2 [Hp,r], U1 [r,Hp], U2 [Hp,r]).
 *   W, U, the biases, h0, x and grad_hs are copied into zero-filled padded buffers in the workspace, the path-2
 *   kernels run on them, and hs, d_x, d_h0 and the parameter gradients are compacted back.  A padded unit has
 *   pre-activation 0 at every step and contributes exact zeros to every gradient, so the real units get exactly what
 *   the library computes for the explicitly padded problem.
 *   Every caller-visible tensor keeps its unpadded shape and layout, with one exception: under
 *   FASTGRNN_FLAG_SAVE_PREACT the forward's z_s is an OPAQUE 256-B aligned buffer of
 *   fastgrnn_hip_zero_extend_plan()'s saved_bytes (the padded pre-activation, the padded hidden-state sequence when
 *   H != Hp, and the low-rank scans' rank-space vector where the padded cell runs on them); c_s is ignored, the
 *   backward reads the buffer back through z_s (c_s ignored, may be NULL) and on this route z_s must not be NULL.
 *   fastgrnn_hip_kernel_path and both workspace queries answer for the padded route where it applies.  d_x may be
 *   NULL when the padded shape allows it (the plan's dx_optional).
 *   Not covered: PREACT_AFFINE and BN_TRAIN cells, fp64, X_BFT frames, H > 256, F > 256 and H > 128 with F > 128. */
#define FASTGRNN_FLAG_ZERO_EXTEND 4096u
/* The caller does not want the input's gradient: fastgrnn_hip_backward_unroll then also accepts d_x == NULL on kernel
 * path 2 for dense H=128/F=32 -- every gate, both saved-tensor contracts, quantTanh, fp32 and bf16 sequences, every
 * layout flag that shape runs with -- and runs a scan variant without the d_x product (every other output bit for
 * bit as with d_x given).  With FASTGRNN_FLAG_ZERO_EXTEND the same holds where the padded shape is dense H=128/F=32
 * (the plan's dx_optional is 1 then).  Where d_x == NULL is already accepted (dense H=256, dense H=128 with F > 32)
 * the flag changes nothing.  A permission only: with d_x given the call runs as without the flag, and no descriptor
 * is refused because of it.  Per entry point: backward_unroll as above; fastgrnn_hip_kernel_path, both workspace
 * queries, fastgrnn_hip_zero_extend_plan (apart from dx_optional), forward_unroll, forward_unroll_affine, the
 * single-step forward and backward, and every fastgrnn_hip_bn_train_* entry point ignore it (answer and behave as
 * without it; the single-step backward always requires d_x). */
#define FASTGRNN_FLAG_NO_INPUT_GRAD 8192u

/* Problem descriptor.  T = 1 for the single-step operators. */
typedef struct fastgrnn_desc {
  int32_t T, B, F, H;       /* frames, utterances, features per frame, hidden units */
  int32_t w_rank, u_rank;   /* 0 = dense */
  int32_t gate_nl;          /* fastgrnn_nonlinearity */
  int32_t update_nl;        /* fastgrnn_nonlinearity; the reference CUDA boundary means TANH */
  int32_t dtype;            /* fastgrnn_dtype */
  uint32_t flags;
} fastgrnn_desc;

/* Parameters (device pointers, boundary layout above). */
typedef struct fastgrnn_params {
  const void *w, *u;                 /* dense matrices or NULL */
  const void *w1, *w2, *u1, *u2;     /* factors or NULL */
  const void *bias_gate;             /* [1,H]  (bias_z) */
  const void *bias_update;           /* [1,H]  (bias_h_prime) */
  const void *zeta, *nu;             /* [1,1] raw */
} fastgrnn_params;

/* Gradient outputs, the 12-tuple of .cu:556 in that order.  d_w/d_u are written
 * for dense operands, d_w1,d_w2 / d_u1,d_u2 for factorised ones; the others are
 * ignored and may be NULL (reference returns torch::empty(0), .cu:221-224). */
typedef struct fastgrnn_grads {
  void *d_x;            /* [T,B,F]; may be NULL on kernel path 2 for dense H=256 and dense H=128 with F > 32 (the
                           input's gradient is then not computed: one GEMM less -- a model's first layer), and
                           for dense H=128/F=32 under FASTGRNN_FLAG_NO_INPUT_GRAD */
  void *d_bias_gate;    /* [1,H] */
  void *d_bias_update;  /* [1,H] */
  void *d_zeta;         /* [1,1] */
  void *d_nu;           /* [1,1] */
  void *d_h0;           /* [B,H]  (d_old_h) */
  void *d_w, *d_u;      /* [H,F], [H,H] */
  void *d_w1, *d_w2;    /* [w_rank,F], [H,w_rank] */
  void *d_u1, *d_u2;    /* [u_rank,H], [H,u_rank] */
} fastgrnn_grads;

int fastgrnn_hip_abi_version(void);
const char *fastgrnn_hip_status_string(int status);

/* Which kernel family a descriptor dispatches to: 0 = generic LDS/VALU scan,
 * 1 = fp32-MFMA scan (v_mfma_f32_16x16x4_f32; 16 utterances per workgroup, U in registers),
 * 2 = split-precision scan: every fp32 operand as three exact bf16 planes, six
 *     v_mfma_f32_16x16x32_bf16 terms per product, fp32 accumulation (error O(2^-24)).
 * direction: 0 forward, 1 backward.  Pure function of the descriptor.
 *
 * Shapes on path 2 (fp32 or bf16 sequences unless noted; everything else runs on paths 1 / 0, 20-30x slower at
 * B = 4096 -- ask this function before assuming):
 *   dense  H=128, F=32            every gate; update tanh or quantTanh (quantTanh: fp32, SAVE_PREACT backward);
 *                                 all layout flags.  Backward with the reference's (z_s, h_prime_s) tensors for the
 *                                 sigmoid / relu / tanh gates, otherwise under FASTGRNN_FLAG_SAVE_PREACT.
 *   dense  H=128, F=64/128/256    (the reference's second layer) time- or batch-major; last-state flags (fp32);
 *                                 x in the sequences' layout or, fp32, the loader's [B,F,T] (FASTGRNN_FLAG_X_BFT:
 *                                 read in place by the forward's frame GEMM, every forward contract and layout;
 *                                 the backward on a time-major workspace copy, time-major sequences only).
 *                                 bf16 sequences: gates sigmoid / relu / tanh, no last-state flags, no [B,F,T]
 *                                 frames, backward under FASTGRNN_FLAG_SAVE_PREACT.
 *   dense  H=256, F=32            (the reference's first layer) time- or batch-major (two-stride rows in
 *                                 both scans, the dU GEMM pairs row b*T+t with hs row b*T+t-1 and every T-th row
 *                                 with h0); x in the sequences' layout or the
 *                                 loader's [B,F,T] (FASTGRNN_FLAG_X_BFT: transposed into the workspace by both
 *                                 calls, 25 us at B = 4096; d_x comes back as [B,F,T]; the backward with BOTH
 *                                 FASTGRNN_FLAG_X_BFT and FASTGRNN_FLAG_BATCH_MAJOR is not on path 2); last-state
 *                                 flags; gates sigmoid / relu / tanh with the reference's (z_s, h_prime_s)
 *                                 tensors, every gate under FASTGRNN_FLAG_SAVE_PREACT.  bf16 sequences: gates
 *                                 sigmoid / relu / tanh; forward with hs alone or under FASTGRNN_FLAG_SAVE_PREACT
 *                                 (time- or batch-major), backward under it (time-major); no [B,F,T] frames, no
 *                                 FASTGRNN_FLAG_HS_LAST.
 *   dense  H=256, F=64/128        (F = 64: the reference's DEFAULT first layer, feature_type='delta' = 32 MFCCs + 32
 *                                 deltas, trainingConfig.py:36, mfccProcessor.py:27-28) time- or batch-major; as F=32:
 *                                 the frame product X.W^T is one batched GEMM into the workspace (T*B*256*4 bytes
 *                                 more of it) in front of the scan.  FASTGRNN_FLAG_X_BFT (fp32): that GEMM reads
 *                                 the [B,F,T] frames in place -- the forward's workspace is the same with and
 *                                 without the flag -- and the backward transposes x into its workspace as F=32 does.
 *   low-rank H=256, F=32, both W and U factorised with 1 <= rank <= 16 (the two ranks may differ; ranks are
 *                                 zero-extended to 16 inside the kernels): gates sigmoid / relu / tanh; all layout
 *                                 flags; backward under FASTGRNN_FLAG_SAVE_PREACT only.
 *   every other factorised cell on one of the dense shapes above (H=128 with any ranks; H=256: F=32 with a rank of
 *                                 17..256 or with only one of W, U factorised, F=64/128 with any ranks:
 *                                 rnn.py:783-798): the factors are
 *                                 multiplied out per call, the dense kernels run, the dense gradients are
 *                                 projected onto the factors (as the reference's CUDA operator does for every
 *                                 low-rank cell, .cu:353-362,546-555); the dense shape's limits and flags apply.
 *                                 No rank-space vector is saved (c_s is ignored under FASTGRNN_FLAG_SAVE_PREACT).
 *   FASTGRNN_FLAG_PREACT_AFFINE (forward only): fp32 sequences, gates sigmoid / relu / tanh, update tanh, dense
 *                                 H=128 with F=32/64/128/256 and dense H=256 with F=32/64/128; time- or batch-major,
 *                                 FASTGRNN_FLAG_HS_LAST; FASTGRNN_FLAG_X_BFT where F > 32 (the frame GEMM reads the
 *                                 [B,F,T] frames in place; F=32 cells take time-major frames only).  Every other fp32 / fp64 cell (other shapes, quantised
 *                                 nonlinearity codes) runs on path 0, time-major without FASTGRNN_FLAG_HS_LAST.
 *   FASTGRNN_FLAG_ZERO_EXTEND     every other fp32 / bf16-sequence cell with H <= 256 whose zero-padded shape (Hp, Fp)
 *                                 is one of the above: run as that shape (copies around the scans, see the flag).
 *   fastgrnn_hip_forward_windows  (inference; utterances are windows of a shared frame pool, see below) fp32, dense,
 *                                 gates sigmoid / relu / tanh, update tanh, plain or FASTGRNN_FLAG_PREACT_AFFINE:
 *                                 H=128 with F=32, H=256 with F=32, H=256 with F=64; hs time-major, batch-major or
 *                                 (FASTGRNN_FLAG_HS_LAST) h_T alone.  Nothing else: ask fastgrnn_hip_windows_supported.
 *   fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows  (training on windows of a frame pool, see below)
 *                                 the plain cells of fastgrnn_hip_forward_windows -- fp32, dense, gates sigmoid / relu /
 *                                 tanh, update tanh, H=128 with F=32, H=256 with F=32 / 64 -- under the one-saved-tensor
 *                                 contract; time- or batch-major, the backward with FASTGRNN_FLAG_GRAD_LAST as well; no
 *                                 input gradient.  Nothing else: ask fastgrnn_hip_train_windows_supported.
 * Under FASTGRNN_FLAG_SAVE_PREACT a factorised forward with both ranks in 1..16 also writes, through c_s, the rank-space vector
 * [U1.h_{t-1} | W1.x_t] as a time-major fp32 [T*B, 32] tensor (each half zero-extended to 16 columns) that the
 * backward takes back through c_s (with z_s, the pre-activation): its factor gradients are contracted inside the
 * scan, d_u2|d_w2 against exactly this vector.  (Round 2's option of passing z_s = NULL and having the backward
 * recompute the pre-activation from c_s is gone: the scan that also contracts the factor gradients has neither the
 * registers nor the LDS for a second copy of [U2|W2]; z_s = NULL is FASTGRNN_ERR_NULL_POINTER again.) */
int fastgrnn_hip_kernel_path(const fastgrnn_desc *d, int direction);

/* FASTGRNN_FLAG_ZERO_EXTEND: what the flag does for a descriptor.  forward / backward: 1 where forward_unroll /
 * backward_unroll take the padded route (backward only under FASTGRNN_FLAG_SAVE_PREACT); Hp, Fp: the padded shape
 * (0 where the route does not apply); dx_optional: 1 where the backward accepts d_x == NULL; saved_bytes: the size
 * of the opaque z_s buffer under FASTGRNN_FLAG_SAVE_PREACT (0 otherwise).  Returns FASTGRNN_OK, or
 * FASTGRNN_ERR_NULL_POINTER / a descriptor error (out zeroed). */
typedef struct fastgrnn_zext_plan {
  int32_t forward, backward;
  int32_t Hp, Fp;
  int32_t dx_optional, reserved;
  size_t saved_bytes;
} fastgrnn_zext_plan;
int fastgrnn_hip_zero_extend_plan(const fastgrnn_desc *d, fastgrnn_zext_plan *out);

/* Everything the library decides from a descriptor alone, in one query: what the calls of d run on and what that route
 * needs from the caller.  fastgrnn_hip_kernel_path, the two workspace queries and fastgrnn_hip_zero_extend_plan each
 * answer one field of it.
 *   path[direction]         fastgrnn_hip_kernel_path(d, direction)
 *   workspace_bytes[0 / 1]  fastgrnn_hip_forward_workspace_bytes(d) / fastgrnn_hip_backward_workspace_bytes(d)
 *   forward_ws_optional     1 where forward_unroll accepts workspace == NULL when z_s is passed (path 2, dense H=128
 *                           with F > 32: the frame product is parked in z_s / c_s; never on the padded route)
 *   dx_optional             1 where backward_unroll accepts g->d_x == NULL, on the padded route (zext.dx_optional then)
 *                           or off it (fastgrnn_grads.d_x; the only field FASTGRNN_FLAG_NO_INPUT_GRAD changes)
 *   rank_space_cols         32 where a forward under FASTGRNN_FLAG_SAVE_PREACT writes the rank-space vector through
 *                           c_s as [T*B, 32] and the backward reads it back (path 2, low-rank H=256/F=32 with both
 *                           ranks in 1..16; never on the padded route, whose z_s buffer holds it); 0 otherwise
 *   zext                    fastgrnn_hip_zero_extend_plan(d)
 * Returns FASTGRNN_OK, or FASTGRNN_ERR_NULL_POINTER / a descriptor error (out zeroed). */
typedef struct fastgrnn_plan {
  int32_t path[2];
  int32_t forward_ws_optional, dx_optional;
  int32_t rank_space_cols, reserved;
  size_t workspace_bytes[2];
  fastgrnn_zext_plan zext;
} fastgrnn_plan;
int fastgrnn_hip_plan(const fastgrnn_desc *d, fastgrnn_plan *out);

/* Workspace sizes in bytes (0 is a valid answer).  Workspace must be 256-B aligned.  The forward answer covers a
 * call without auxiliary outputs; dense H=128 layers with F > 32 park the frame product X.W^T in z_s / c_s when
 * the caller passes them and then accept workspace == NULL. */
size_t fastgrnn_hip_forward_workspace_bytes(const fastgrnn_desc *d);
size_t fastgrnn_hip_backward_workspace_bytes(const fastgrnn_desc *d);

/* forward_unroll -- replaces fastgrnn_unroll_forward (fastgrnn_cuda.cpp:147-180 ->
 * .cu:320-415).  x:[T,B,F], h0:[B,H] -> hs:[T,B,H]; z_s,c_s:[T,B,H] are the
 * reference's z_s / h_prime_s outputs and may be NULL when the caller does not
 * need them (forward-only use).
 * The generic scan (path 0) holds its state tiles in up to 160 KiB of LDS: (16 H + 8 F + 8 w_rank + 8 u_rank) elements
 * in forward_unroll, (18 H + 8 u_rank + 512) in backward_unroll.  A direction that does not fit -- on no other path
 * either -- has fastgrnn_hip_kernel_path -1 and workspace 0, and its call returns FASTGRNN_ERR_UNSUPPORTED before the
 * workspace check and before anything is launched.  The backward's limit is the lower one: ask the plan for both
 * directions before training at such a size. */
int fastgrnn_hip_forward_unroll(const fastgrnn_desc *d, const fastgrnn_params *p,
                                const void *x, const void *h0,
                                void *hs, void *z_s, void *c_s,
                                void *workspace, size_t workspace_bytes, void *stream);

/* forward_unroll_affine -- inference forward of the eval-mode BatchNorm cell (FASTGRNN_FLAG_PREACT_AFFINE above,
 * which d->flags must carry).  gate_scale, update_scale: [H] in the parameter dtype; p->bias_gate / p->bias_update
 * hold the folded biases, p->w / p->u the folded (dense) matrices.  x:[T,B,F], h0:[B,H] -> hs:[T,B,H] (or the
 * layouts of FASTGRNN_FLAG_BATCH_MAJOR / FASTGRNN_FLAG_HS_LAST on kernel path 2).  No z_s / h_prime_s: nothing is
 * saved for a backward.  With FASTGRNN_FLAG_X_BFT (kernel path 2, F = 64 / 128 / 256) x is the loader's [B,F,T].
 * fp32 or fp64; bf16 sequences, FASTGRNN_FLAG_X_BFT on 32-feature cells, FASTGRNN_FLAG_SAVE_PREACT, factorised
 * operands and the layout flags off path 2 answer FASTGRNN_ERR_UNSUPPORTED. */
int fastgrnn_hip_forward_unroll_affine(const fastgrnn_desc *d, const fastgrnn_params *p,
                                       const void *gate_scale, const void *update_scale,
                                       const void *x, const void *h0, void *hs,
                                       void *workspace, size_t workspace_bytes, void *stream);

/* forward_windows -- inference forward over OVERLAPPING utterances: utterance b is the d->T consecutive rows that
 * start at row x_start[b] of a shared frame pool x_pool:[pool_rows, F] (fp32, contiguous); at step t it reads pool row
 * x_start[b] + t.  This is how the reference's detector uses the model (inferencetry.py:165-227: a 99-frame window
 * slid over continuous audio, every window scored from a zero state): d->B windows at hop h are x_start[w] = w * h,
 * with no T/h-fold copy of the stream.  Starts may overlap, repeat and come in any order (random crops of longer
 * clips are the same call).  x_start: [B] int32 on the device; the library cannot look at its contents:
 *   0 <= x_start[b] <= pool_rows - T  for every b  IS THE CALLER'S OBLIGATION (a start outside reads outside the pool).
 * h0:[B,H]; hs follows d->flags as in forward_unroll_affine: [T,B,H], [B,T,H] (FASTGRNN_FLAG_BATCH_MAJOR) or [B,H]
 * (FASTGRNN_FLAG_HS_LAST).  Nothing is saved for a backward: this is the inference call; training on windows is
 * fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows below (no gradient w.r.t. the pool).  gate_scale / update_scale: both NULL for the plain cell; both non-NULL ([H] fp32) for the
 * eval-mode BatchNorm arithmetic, and d->flags must then carry FASTGRNN_FLAG_PREACT_AFFINE (and only then).
 * Cells (fastgrnn_hip_windows_supported answers 1): fp32, dense, gate sigmoid / relu / tanh, update tanh, and
 *   H=128 with F=32;  H=256 with F=32;  H=256 with F=64
 * with no flag other than BATCH_MAJOR, HS_LAST and PREACT_AFFINE.  F=32: the scans read the pool in place.  F=64: the
 * frame product X.W^T is computed ONCE per pool row, P_pool[pool_rows, 256] in the workspace (pool_rows*1024 bytes
 * instead of T*B*1024), and the scan reads row x_start[b] + t of it.  Everything else -- other shapes, bf16
 * sequences, fp64, factorised operands, quantised codes, FASTGRNN_FLAG_SAVE_PREACT / X_BFT / ZERO_EXTEND / BN_TRAIN /
 * FORCE_* and the remaining flags -- answers FASTGRNN_ERR_UNSUPPORTED (gather the windows and call forward_unroll).
 * Errors otherwise: FASTGRNN_ERR_NULL_POINTER (x_pool, x_start, h0, hs, a parameter; exactly one scale NULL; the flag
 * without scales), FASTGRNN_ERR_BAD_SHAPE (pool_rows < T, pool_rows >= 2^31, size overflow), FASTGRNN_ERR_WORKSPACE.
 * Workspace: fastgrnn_hip_forward_windows_workspace_bytes(d, pool_rows) -- 0 for H=128; for H=256 512 KB of flag
 * words (one per workgroup of the largest batch the shape takes) plus, for F=64, P_pool: a function of pool_rows
 * alone, not of d->B or d->T, so one allocation serves every set of windows cut from a pool; 0 for an unsupported
 * descriptor. */
int fastgrnn_hip_windows_supported(const fastgrnn_desc *d);            /* 1 / 0 */
size_t fastgrnn_hip_forward_windows_workspace_bytes(const fastgrnn_desc *d, size_t pool_rows);
int fastgrnn_hip_forward_windows(const fastgrnn_desc *d, const fastgrnn_params *p,
                                 const void *gate_scale, const void *update_scale,
                                 const void *x_pool, size_t pool_rows, const int32_t *x_start,
                                 const void *h0, void *hs,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* forward_windows_train / backward_windows -- TRAINING on windows of a frame pool: the layer that reads the pool is a
 * model's first layer, nobody wants its input gradient, and without d_x the backward over windows needs no scatter-add,
 * only the gather of x the forward does.  x_pool, pool_rows and x_start are those of fastgrnn_hip_forward_windows
 * (x_pool 16-byte aligned), and so is the range of the starts:
 *   0 <= x_start[b] <= pool_rows - T  for every b  IS THE CALLER'S OBLIGATION (a start outside reads outside the pool).
 * Both calls ALWAYS run under the one-saved-tensor contract of FASTGRNN_FLAG_SAVE_PREACT: `saved` is the fp32
 * pre-activation W.x_t + U.h_{t-1} (no bias) in the sequences' layout, [T,B,H] or (FASTGRNN_FLAG_BATCH_MAJOR) [B,T,H] --
 * what forward_unroll writes to z_s under that flag, bit for bit, on the gathered windows.  The caller does NOT pass
 * FASTGRNN_FLAG_SAVE_PREACT: a descriptor that carries it is refused (FASTGRNN_ERR_UNSUPPORTED, supported query 0)
 * like every other flag the two calls do not know, so that the flag keeps one meaning per entry point and
 * fastgrnn_hip_windows_supported / fastgrnn_hip_forward_windows go on refusing it.  hs is always the full sequence
 * (training saves it): there is no FASTGRNN_FLAG_HS_LAST.
 * Cells (fastgrnn_hip_train_windows_supported answers 1): fp32, dense, gate sigmoid / relu / tanh, update tanh, and
 *   H=128 with F=32;  H=256 with F=32;  H=256 with F=64.
 * Flags: FASTGRNN_FLAG_BATCH_MAJOR in both calls and the queries; FASTGRNN_FLAG_GRAD_LAST in the backward, its workspace
 * query and the supported query (grad_hs is [B,H]; the forward and its workspace query refuse / answer 0).  Any other
 * flag, bf16 sequences, fp64, factorised operands, quantised codes and other shapes answer FASTGRNN_ERR_UNSUPPORTED /
 * 0 (gather the windows and call forward_unroll / backward_unroll).
 *   forward:  x_pool, x_start, h0:[B,H] -> hs, saved.  H=256 reads the pool in place; workspace as
 *             fastgrnn_hip_forward_windows: the flag words plus, for F=64, P_pool[pool_rows,256] -- a function of
 *             pool_rows alone.  H=128 gathers the windows into a copy of x in the workspace (align256(T*B*F*4) bytes,
 *             the backward's kernel) and runs the scan of forward_unroll on it: a windowed scan that saves the
 *             pre-activation is not built for H=128.
 *   backward: grad_hs (the layout of hs, or [B,H]), x_pool, x_start, hs, saved, h0 -> g->d_h0, d_w, d_u, d_bias_gate,
 *             d_bias_update, d_zeta, d_nu (overwritten): bit for bit what backward_unroll writes for the gathered
 *             windows with d_x == NULL (FASTGRNN_FLAG_SAVE_PREACT, on H=128 with FASTGRNN_FLAG_NO_INPUT_GRAD).
 *             g->d_x MUST BE NULL: the gradient with respect to the pool is a scatter-add over overlapping windows
 *             and is deliberately not built; a non-NULL d_x answers FASTGRNN_ERR_UNSUPPORTED.  The factor gradients
 *             are ignored.
 *             The windows are gathered into a copy of x, [T,B,F] or [B,T,F], in the LAST align256(T*B*F*4) bytes of
 *             the workspace (one small kernel) and the route of backward_unroll runs on it: workspace =
 *             fastgrnn_hip_backward_workspace_bytes(d) + align256(T*B*F*4) for every shape.  (A scan that reads the
 *             pool in place on H=128 is not built: DESIGN.md 4.1g.)
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (any pointer above, a parameter, a gradient output),
 * FASTGRNN_ERR_BAD_SHAPE (pool_rows < T, pool_rows >= 2^31, size overflow), FASTGRNN_ERR_UNSUPPORTED,
 * FASTGRNN_ERR_WORKSPACE (missing, short or not 256-byte aligned).  Both workspace queries answer 0 for an unsupported
 * descriptor and for pool_rows >= 2^31. */
int fastgrnn_hip_train_windows_supported(const fastgrnn_desc *d);      /* 1 / 0 */
size_t fastgrnn_hip_train_windows_forward_workspace_bytes(const fastgrnn_desc *d, size_t pool_rows);
size_t fastgrnn_hip_train_windows_backward_workspace_bytes(const fastgrnn_desc *d, size_t pool_rows);
int fastgrnn_hip_forward_windows_train(const fastgrnn_desc *d, const fastgrnn_params *p,
                                       const void *x_pool, size_t pool_rows, const int32_t *x_start,
                                       const void *h0, void *hs, void *saved,
                                       void *workspace, size_t workspace_bytes, void *stream);
int fastgrnn_hip_backward_windows(const fastgrnn_desc *d, const fastgrnn_params *p,
                                  const void *grad_hs, const void *x_pool, size_t pool_rows, const int32_t *x_start,
                                  const void *hs, const void *saved, const void *h0,
                                  const fastgrnn_grads *g,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* backward_unroll -- replaces fastgrnn_unroll_backward (fastgrnn_cuda.cpp:182-232 ->
 * .cu:417-557).  grad_hs:[T,B,H] is dL/d(hs[t]) for every t; z_s,c_s are the
 * forward's outputs.  Writes every applicable member of *g (overwrites, does not
 * accumulate). */
int fastgrnn_hip_backward_unroll(const fastgrnn_desc *d, const fastgrnn_params *p,
                                 const void *grad_hs, const void *x, const void *hs,
                                 const void *z_s, const void *c_s, const void *h0,
                                 const fastgrnn_grads *g,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* forward -- replaces fastgrnn_forward (fastgrnn_cuda.cpp:73-107 -> .cu:123-198).
 * x:[B,F], old_h:[B,H] -> new_h, z, c each [B,H].  d->T must be 1. */
int fastgrnn_hip_forward(const fastgrnn_desc *d, const fastgrnn_params *p,
                         const void *x, const void *old_h,
                         void *new_h, void *z, void *c,
                         void *workspace, size_t workspace_bytes, void *stream);

/* backward -- replaces fastgrnn_backward (fastgrnn_cuda.cpp:109-145 -> .cu:200-318).
 * grad_h:[B,H]; g->d_x is [B,F], g->d_h0 is d_old_h.  d->T must be 1. */
int fastgrnn_hip_backward(const fastgrnn_desc *d, const fastgrnn_params *p,
                          const void *grad_h, const void *x, const void *old_h,
                          const void *z, const void *c,
                          const fastgrnn_grads *g,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- classifier head on the last state ------------------------------------------------------
 * head_xent -- replaces, for training, the three torch modules the reference chains after the last layer:
 *   keyword_scores = F.log_softmax(self.hidden2keyword(hs[T-1]), dim=1)     (model.py:86-88, 226-230)
 *   loss = nn.NLLLoss()(keyword_scores, labels)                              (trainClassifier.py:154,236; mean)
 * and their backward.  fp32.  h_last:[B,H] (e.g. the FASTGRNN_FLAG_HS_LAST / last_state output), fc_w:[C,H],
 * fc_b:[C] (nn.Linear layout), labels:[B] int64 in [0,C) or -100 (nn.NLLLoss's default ignore_index: such rows add
 * neither loss nor gradient and the mean runs over the others; any other out-of-range label makes the loss NaN,
 * where torch raises a device-side assert).  Writes loss[1], log_probs:[B,C] (may be NULL),
 * d_h_last:[B,H] = dLoss/dh_last, d_fc_w:[C,H], d_fc_b:[C] (overwritten).  Deterministic (fixed-order reduction).
 * H <= 256, C <= 64, else FASTGRNN_ERR_UNSUPPORTED.  workspace: fastgrnn_hip_head_workspace_bytes(B,H,C). */
size_t fastgrnn_hip_head_workspace_bytes(int32_t B, int32_t H, int32_t C);
int fastgrnn_hip_head_xent(int32_t B, int32_t H, int32_t C, const void *h_last, const void *fc_w,
                           const void *fc_b, const int64_t *labels, void *loss, void *log_probs,
                           void *d_h_last, void *d_fc_w, void *d_fc_b,
                           void *workspace, size_t workspace_bytes, void *stream);

/* head_predict -- the inference counterpart of head_xent: what the reference does with a batch of scores outside
 * training, in one call and without gradients:
 *   keyword_scores = F.log_softmax(self.hidden2keyword(hs[T-1]), dim=1)     (model.py:86-88, 226-230)
 *   predicted_index = torch.argmax(...)                                      (inferencetry.py:213-214)
 *   passed += (scores[i].argmax() == labels[i])  for every i                 (trainClassifier.py:54-65, batch_accuracy)
 * fp32, operands as in head_xent.  Writes log_probs:[B,C] (may be NULL: not stored) -- the same bits head_xent writes
 * for the same operands --, pred:[B] int32 = the argmax of the logits by torch.argmax's rules (the lowest index among
 * equal maxima; a NaN is the maximum and the first NaN wins), and, when labels:[B] int64 is given, n_correct[1] int32 =
 * the number of rows with pred[b] == labels[b] (required iff labels; a label of -100 or any other value outside [0,C)
 * never matches).  The count is an integer sum of per-workgroup counts: exact, repeatable, and the call may be captured
 * in a graph.  H <= 256, C <= 64, else FASTGRNN_ERR_UNSUPPORTED.
 * workspace: fastgrnn_hip_head_predict_workspace_bytes(B,H,C) when labels is given (it holds the per-workgroup counts);
 * without labels it is not used and may be NULL.  The largest heads (more than 64 KB of LDS, e.g. H = 256 with C = 64)
 * opt in to their LDS size with an attribute call in front of the launch, as head_xent does; that call is not a
 * stream operation and the whole call captures in a graph at those sizes too. */
size_t fastgrnn_hip_head_predict_workspace_bytes(int32_t B, int32_t H, int32_t C);
int fastgrnn_hip_head_predict(int32_t B, int32_t H, int32_t C, const void *h_last, const void *fc_w,
                              const void *fc_b, const int64_t *labels, void *log_probs, int32_t *pred,
                              int32_t *n_correct, void *workspace, size_t workspace_bytes, void *stream);

/* vote_windows -- the bookkeeping of the reference's detector (inferencetry.py:217-227) for S independent streams of Nw
 * consecutive window predictions, each from an empty vote list and no previous detection.  pred:[S,Nw] int32.  For
 * window w of stream s, votes = pred[s, max(0, w-K+1) .. w] (K = num_windows, NUM_WINDOWS = 10 in the reference), (m, f)
 * the most frequent value among them and its frequency -- on equal frequency the value whose first occurrence in votes
 * is earliest, which is Counter(votes).most_common(1) --, and with M = majority (MAJORITY = 5):
 *   majority_out[s,w] = m if f >= M else -1
 *   event_out[s,w]    = m if f >= M and m != previous else -1;  previous becomes m when an event fires
 * (the reference prints "Detected keyword" exactly where event_out >= 0).  A negative entry of pred is a vote for no
 * class: it holds its slot in the list and is never m.  1 <= M <= K, else FASTGRNN_ERR_BAD_SHAPE; K <= 64, else
 * FASTGRNN_ERR_UNSUPPORTED.  No workspace. */
int fastgrnn_hip_vote_windows(int32_t S, int32_t Nw, int32_t num_windows, int32_t majority, const int32_t *pred,
                              int32_t *majority_out, int32_t *event_out, void *stream);

/* train_update -- the end of a trainer iteration in one call: optimizer.step() (trainClassifier.py:249) for every
 * parameter tensor of a model, then the IHT phase of trainClassifier.py:251-259 on the tensors marked for it.  One
 * launch per FASTGRNN_UPDATE_MAX_SEGS tensors ("segments"), one workgroup per segment; the segment table travels in
 * the kernel arguments, so the call allocates nothing, copies nothing and never synchronises, and it may be captured
 * in a graph.  fp32 tensors, fp32 arithmetic:
 *   algo 0, torch.optim.Adam (amsgrad=False, maximize=False; weight_decay is L2, not AdamW), t = step[0]:
 *     g' = g + wd p;  m' = beta1 m + (1-beta1) g';  v' = beta2 v + (1-beta2) g'^2
 *     p' = p - (lr / (1-beta1^t)) m' / (sqrt(v') / sqrt(1-beta2^t) + eps)      (the bias corrections in double)
 *   algo 1, torch.optim.SGD, mu = momentum, tau = dampening:
 *     g' = g + wd p;  b' = g' if t == 1 else mu b + (1-tau) g';  d = g' + mu b' with nesterov, else b';  p' = p - lr d
 *     (mu = 0: d = g' and the buffer is left alone, as torch keeps none)
 * Then, on segments with iht != 0, by the device scalar iht_mode[0]:
 *   1: th = the element of 0-based rank keep_rank among the ascending |p'|, found exactly (radix select on the bit
 *      patterns); p' = 0 where |p'| < th -- ties with th survive, as numpy.percentile(..., 'higher') in utils.py:53-64
 *      leaves them; keep_rank = 0 zeroes nothing.  support[i] = (p'[i] != 0), one byte per element, is written for
 *      every such segment.
 *   2: p' = 0 where support[i] == 0 (utils.py:66-81); support is only read.
 *   0 or any other value: nothing.  The moments m, v, b are never masked (torch keeps updating them for zeroed entries).
 * NaN parameters: the update propagates them; their place in the threshold's order is not specified.
 * lr[1] (float), step[1] (int64: the 1-based number of THIS step, incremented by the caller, only read here) and
 * iht_mode[1] (int32; NULL = 0) are DEVICE scalars: a replayed graph picks up new values.  segs is a HOST array, read
 * before the call returns.  Repeatable bit for bit (the histogram's integer sums do not depend on order).
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (h, segs, lr, step; a segment's param, grad or state0;
 * state1 under Adam; support on a segment with iht != 0, and iht_mode when there is such a segment),
 * FASTGRNN_ERR_UNSUPPORTED (algo other than 0, 1), FASTGRNN_ERR_BAD_SHAPE (n_segs < 1; n outside 1..2^22; keep_rank
 * outside 0..n-1; beta1, beta2 or momentum outside [0,1); eps <= 0 under Adam; weight_decay < 0; nesterov with zero
 * momentum or non-zero dampening, torch's own rule).  No workspace. */
#define FASTGRNN_UPDATE_MAX_SEGS 32
#define FASTGRNN_UPDATE_MAX_N (1 << 22)
typedef struct fastgrnn_update_seg {
  void *param; const void *grad;      /* [n] fp32, device */
  void *state0, *state1;              /* Adam: exp_avg, exp_avg_sq; SGD: momentum buffer, NULL */
  uint8_t *support;                   /* [n], required iff iht != 0 */
  int64_t n;                          /* 1 .. 2^22 */
  int64_t keep_rank;                  /* 0 .. n-1: ceil((1-s)(n-1)), computed by the caller in double as
                                         numpy's percentile index; 0 = everything survives */
  int32_t iht, reserved;              /* 1: this tensor takes part in the IHT phases */
} fastgrnn_update_seg;

typedef struct fastgrnn_update_hyper {
  int32_t algo;                       /* 0 Adam, 1 SGD */
  int32_t nesterov;
  double beta1_or_momentum, beta2_or_dampening, eps, weight_decay;
} fastgrnn_update_hyper;

int fastgrnn_hip_train_update(const fastgrnn_update_hyper *h, const fastgrnn_update_seg *segs /* HOST array */,
                              int32_t n_segs, const float *lr, const int64_t *step, const int32_t *iht_mode,
                              void *stream);

/* optim_update -- train_update for the other six optimizers of the trainer's configure_optimizer
 * (trainClassifier.py:67-95), which keep up to three state tensors per parameter.  train_update's conventions hold
 * throughout: one launch per FASTGRNN_UPDATE_MAX_SEGS segments, one workgroup per segment, the segment table in the
 * kernel arguments; nothing allocated, nothing copied, never a synchronise, so the call may be captured in a graph;
 * lr, step (the 1-based number of THIS step, incremented by the caller) and iht_mode are DEVICE scalars that are only
 * read; segs is a HOST array; the IHT phase (mode 1: exact threshold + support; mode 2: support mask) follows the update
 * with train_update's semantics and the state tensors are never masked; repeatable bit for bit.
 * The rules are torch.optim's (torch 2.10, foreach=False, maximize=False, not differentiable): fp32 operands and
 * arithmetic, what depends on the step count in double.  t = step[0]; g' = g + wd p in every rule but Rprop;
 * lerp(a, b, w) = a + w (b - a), evaluated as torch does (b - (b - a)(1 - w) from w = 0.5 on).
 *   algo 2, RMSprop.  h = alpha, eps, momentum; flags bit 0: centered.  state = square_avg v, momentum_buffer b (read
 *     and written only with momentum > 0), grad_avg a (only when centered).
 *     v' = alpha v + (1-alpha) g'^2;  centered: a' = lerp(a, g', 1-alpha), d = sqrt(v' - a'^2) + eps;  else
 *     d = sqrt(v') + eps;  momentum > 0: b' = momentum b + g'/d, p' = p - lr b';  else p' = p - lr g'/d
 *   algo 3, Adagrad.  h = lr_decay, eps.  state = sum s (the caller fills it with initial_accumulator_value).
 *     clr = lr / (1 + (t-1) lr_decay);  s' = s + g'^2;  p' = p - clr g' / (sqrt(s') + eps)
 *   algo 4, Adadelta.  h = rho, eps.  state = square_avg v, acc_delta a.
 *     v' = rho v + (1-rho) g'^2;  D = sqrt(a + eps) / sqrt(v' + eps) g';  a' = rho a + (1-rho) D^2;  p' = p - lr D
 *   algo 5, Adamax.  h = beta1, beta2, eps.  state = exp_avg m, exp_inf u.
 *     m' = lerp(m, g', 1-beta1);  u' = max(beta2 u, |g'| + eps);  p' = p - (lr / (1 - beta1^t)) m' / u'
 *   algo 6, ASGD.  h = lambd, alpha, t0.  state = ax.  eta and mu are what the previous step left (step 1: eta = lr,
 *     mu = 1);  p' = p (1 - lambd eta) - eta g' (g' from the old p; 1 - lambd eta formed in double, rounded once);
 *     ax' = p' if mu == 1 else ax + mu (p' - ax);  then eta <- lr / (1 + lambd lr t)^alpha, mu <- 1 / max(1, t - t0),
 *     both rounded to fp32.  They live in scalars[4] (device, fp32), two pairs indexed by the step's parity: step t reads
 *     scalars[2((t-1)&1) .. +1] (t > 1) and writes scalars[2(t&1) .. +1], so no workgroup reads what another has replaced.
 *   algo 7, Rprop.  h = etaminus, etaplus, step_min, step_max.  state = prev, step_size (the caller fills it with the
 *     learning rate).  s = sign(g prev), the product rounded to fp32;  step' = clamp(step (etaplus if s > 0, etaminus if
 *     s < 0, else 1), step_min, step_max);  g'' = 0 where s < 0 else g;  p' = p - sign(g'') step';  prev' = g''.
 *     lr[0] and step[0] are not used; weight_decay must be 0.
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (h, segs, lr, step; a segment's param, grad or a state
 * tensor its rule needs; support on a segment with iht != 0, and iht_mode when there is such a segment; scalars under
 * ASGD), FASTGRNN_ERR_UNSUPPORTED (algo outside 2..7: Adam and SGD are train_update's), FASTGRNN_ERR_BAD_SHAPE
 * (n_segs < 1; n outside 1..2^22; keep_rank outside 0..n-1; weight_decay < 0; a hyper-parameter outside
 * torch.optim's constructor range -- alpha, momentum, lr_decay < 0; rho outside [0,1]; beta1, beta2 outside [0,1) --;
 * eps <= 0 under RMSprop, Adagrad, Adadelta, Adamax, where it divides; under Rprop weight_decay != 0, etaminus outside
 * (0,1), etaplus <= 1, step_min > step_max; any of them NaN).  No workspace. */
typedef struct fastgrnn_optim_seg {
  void *param; const void *grad;      /* [n] fp32, device */
  void *state[3];                     /* per rule, in the order listed above; those a rule does not use: NULL */
  uint8_t *support;                   /* [n], required iff iht != 0 */
  int64_t n, keep_rank;               /* as fastgrnn_update_seg */
  int32_t iht, reserved;
} fastgrnn_optim_seg;

typedef struct fastgrnn_optim_hyper {
  int32_t algo;                       /* 2 RMSprop, 3 Adagrad, 4 Adadelta, 5 Adamax, 6 ASGD, 7 Rprop */
  int32_t flags;                      /* RMSprop: bit 0 centered */
  double h[6];                        /* per rule, above; the rest ignored */
  double weight_decay;
} fastgrnn_optim_hyper;

int fastgrnn_hip_optim_update(const fastgrnn_optim_hyper *h, const fastgrnn_optim_seg *segs /* HOST array */,
                              int32_t n_segs, const float *lr, const int64_t *step, const int32_t *iht_mode,
                              float *scalars /* ASGD only: device [4] */, void *stream);

/* grad_guard -- the stage between backward and the update: the global gradient norm, the clipping coefficient of
 * torch.nn.utils.clip_grad_norm_ and the rejection of a step whose gradient is not finite, decided on the device.  It
 * runs on the gradient tensors ("segments") the update call is handed afterwards, with train_update's conventions: one
 * launch per FASTGRNN_UPDATE_MAX_SEGS segments, one workgroup per segment, the segment table in the kernel arguments,
 * then one single-workgroup launch; nothing allocated, nothing copied, never a synchronise, so the call may be
 * captured in a graph.
 *   S    = the sum over all elements of all segments of g^2, accumulated in double (the square of an fp32 value is
 *          exact in double; finite gradients cannot overflow it, so S is non-finite iff some element is).  The order
 *          of the additions is a function of n_segs and the n alone and no atomics are used: repeatable bit for bit.
 *   norm = (float)sqrt(S)
 *   skip = (flags & FASTGRNN_GUARD_SKIP_NONFINITE) && !isfinite(S)
 *   coef = 0 when skip;  1 when max_norm is +inf;  else (float)min(1, max_norm / (sqrt(S) + 1e-6)), formed in double
 *          and rounded once -- clip_grad_norm_'s rule with error_if_nonfinite=False, a NaN norm giving a NaN coef
 *   applied += 1 when !skip, skipped += 1 when skip: each call increments exactly one of the two.
 * state is DEVICE memory, zero-filled by the caller before the first step and otherwise only handed on to the guarded
 * update calls; segs is a HOST array, read before the call returns; workspace: at least
 * fastgrnn_hip_grad_guard_workspace_bytes(n_segs) bytes (one double per segment, rounded up to 256), 8-byte aligned.
 *
 * train_update_guarded / optim_update_guarded -- train_update / optim_update with `step` replaced by the state a
 * grad_guard call on the same stream has just written.  The rule (all eight of them) is the unguarded one with two
 * substitutions: g coef in place of g (one fp32 multiply before the weight-decay fmaf; Rprop: before the sign
 * product), and t = guard->applied in place of step[0] wherever the rule uses the step count (Adam's and Adamax's
 * bias corrections, Adagrad's decayed rate, SGD's first-step rule, ASGD's parity and its next eta / mu).  With
 * guard->skip set the rule is the identity p' = p: the update writes no parameter, no state tensor and no ASGD
 * scalar, and the IHT phase runs on p' with its usual meaning (mode 1 thresholds and records the support, mode 2
 * masks).  With max_norm = +inf and finite gradients the call is bit-identical to the unguarded call at
 * step[0] = applied (g 1.0f is exact).
 * Errors, all before any launch.  grad_guard: FASTGRNN_ERR_NULL_POINTER (segs, state, workspace, a segment's grad),
 * FASTGRNN_ERR_BAD_SHAPE (n_segs < 1; n outside 1..2^22; max_norm <= 0 or NaN), FASTGRNN_ERR_UNSUPPORTED (unknown
 * flag bits), FASTGRNN_ERR_WORKSPACE (too small or not 8-byte aligned).  The guarded updates: guard NULL is
 * FASTGRNN_ERR_NULL_POINTER; everything else as the unguarded call. */
#define FASTGRNN_GUARD_SKIP_NONFINITE 1
typedef struct fastgrnn_guard_seg {
  const void *grad;                   /* [n] fp32, device */
  int64_t n;                          /* 1 .. 2^22 */
} fastgrnn_guard_seg;

typedef struct fastgrnn_guard_state {   /* DEVICE, 32 bytes, zero-filled by the caller before the first step */
  float norm, coef; int32_t skip, reserved; int64_t applied, skipped;
} fastgrnn_guard_state;

size_t fastgrnn_hip_grad_guard_workspace_bytes(int32_t n_segs);   /* 0 for n_segs < 1 */
int fastgrnn_hip_grad_guard(const fastgrnn_guard_seg *segs /* HOST array */, int32_t n_segs, double max_norm,
                            int32_t flags, fastgrnn_guard_state *state, void *workspace, size_t workspace_bytes,
                            void *stream);
int fastgrnn_hip_train_update_guarded(const fastgrnn_update_hyper *h, const fastgrnn_update_seg *segs /* HOST array */,
                                      int32_t n_segs, const float *lr, const fastgrnn_guard_state *guard,
                                      const int32_t *iht_mode, void *stream);
int fastgrnn_hip_optim_update_guarded(const fastgrnn_optim_hyper *h, const fastgrnn_optim_seg *segs /* HOST array */,
                                      int32_t n_segs, const float *lr, const fastgrnn_guard_state *guard,
                                      const int32_t *iht_mode, float *scalars /* ASGD only: device [4] */,
                                      void *stream);

/* mfcc -- the reference's featuriser, librosa.feature.mfcc + librosa.feature.delta at librosa 0.10.2's defaults as
 * data_pipeline/mfccProcessor.py:43-58 calls them, then the pad / cut and the normalisation of preprocessing.py:79-88 and
 * inferencetry.py:165-200, from raw audio in one launch.  sr = 16000, n_fft = win_length = 400, hop = 160, n_mels = 128
 * are fixed.  Per clip y of len samples:
 *   1. fp32 samples, or int16 PCM times 2^-15; with FASTGRNN_MFCC_PEAK_NORMALIZE y /= max|y| (fp32) if that is > 0.
 *   2. center=True, pad_mode="constant": 200 zeros on each side, n = 1 + len / 160 frames, periodic Hann window.
 *   3. power |rfft|^2 (201 bins);  4. Slaney mel weights (fmin 0, fmax 8000, norm="slaney"; fp64 rounded to fp32).
 *   5. dB = 10 log10(max(1e-10, M)), then max(dB, max over the clip's n frames and 128 mels - top_db)  (top_db < 0:
 *      no clip).   6. DCT-II, norm="ortho", the first n_mfcc coefficients.
 *   7. order >= 1: delta = savgol(width, polyorder 1, deriv 1, mode="interp"), taps k / sum k^2; order 2 adds
 *      delta-delta = savgol(width, polyorder 2, deriv 2) OF THE MFCC, taps 2 (w k^2 - sum k^2) / (w sum k^4 - (sum k^2)^2);
 *      k = -h..h, h = width / 2; the first h frames take frame h's value, the last h frame n-1-h's (deriv == polyorder
 *      makes the interp edges constant).   8. rows [mfcc; delta; delta2]: F = n_mfcc (order + 1) features.
 *   9. pad with zeros or cut to max_len frames (after 5 and 7 have seen all n frames).
 *  10. with mean / std ([F] fp32, both or neither): (f - mean) / std; padded frames become -mean / std.
 * audio: clip b starts at ELEMENT b * clip_stride (fp32 or int16; no alignment beyond the element's is assumed);
 * clip_stride < L gives overlapping clips of one recording without a copy.  lengths: NULL (every clip is L long) or [B]
 * int32 on the device with 1280 <= lengths[b] <= L; the kernel clamps into that range, so no value makes it read or
 * write outside its buffers.  feats: [B, max_len, F] fp32, contiguous and fully written -- a frame pool for
 * fastgrnn_hip_forward_windows (clip b = rows b max_len ..).  tables: fastgrnn_hip_mfcc_tables_bytes() bytes that
 * fastgrnn_hip_mfcc_init_tables filled once (window-folded DFT basis, mel weights, DCT, taps: computed on the device in
 * fp64 with exact integer angle reduction, rounded to fp32); the library allocates nothing.  Arithmetic: the three
 * products on the exact-fp32 matrix instruction (a k-ordered fmaf chain), accurate log10f, no atomics: repeatable bit
 * for bit, and a clip's rows do not depend on its neighbours.  One launch on `stream`, no host decision on device data:
 * the call may be captured in a graph.
 * Supported: 1280 <= L <= 16000, 1 <= n_mfcc <= 64, order 0 / 1 / 2, width odd in 3..15 with L >= 160 (width - 1),
 * flags = 0 or FASTGRNN_MFCC_PEAK_NORMALIZE; else FASTGRNN_ERR_UNSUPPORTED.  FASTGRNN_ERR_BAD_SHAPE: B, L, clip_stride,
 * max_len or n_mfcc < 1, top_db NaN, size overflow; FASTGRNN_ERR_BAD_DTYPE: audio_dtype; FASTGRNN_ERR_NULL_POINTER: d,
 * audio, tables, feats, exactly one of mean / std; FASTGRNN_ERR_WORKSPACE as everywhere (the query answers 0 today).
 * All before any launch. */
#define FASTGRNN_MFCC_PEAK_NORMALIZE 1u
#define FASTGRNN_MFCC_AUDIO_F32 0
#define FASTGRNN_MFCC_AUDIO_I16 1
typedef struct fastgrnn_mfcc_desc {
  int32_t B, L;                       /* clips, samples per clip */
  int64_t clip_stride;                /* elements between the starts of consecutive clips, >= 1 */
  int32_t audio_dtype;                /* FASTGRNN_MFCC_AUDIO_F32 / _I16 */
  int32_t n_mfcc, order, width, max_len;
  float top_db;
  uint32_t flags;
} fastgrnn_mfcc_desc;

size_t fastgrnn_hip_mfcc_tables_bytes(void);
int fastgrnn_hip_mfcc_init_tables(void *tables, void *stream);
size_t fastgrnn_hip_mfcc_workspace_bytes(const fastgrnn_mfcc_desc *d);
int fastgrnn_hip_mfcc(const fastgrnn_mfcc_desc *d, const void *audio, const int32_t *lengths, const void *tables,
                      const float *mean, const float *std, void *feats, void *workspace, size_t workspace_bytes,
                      void *stream);

/* mfcc_augment -- the featuriser reading an AUDIO BANK through per-clip augmentation records: the reference's
 * data_pipeline/audioAugmentation.py (background noise at a gain, wrapped to the clip's length) plus the time shift of
 * preprocessing.py:13's to-do, applied while the clip is loaded; the augmented clip is never written to memory.
 * d is a fastgrnn_mfcc_desc whose B is the number of OUTPUT clips (= records) and whose clip_stride is the bank's.
 * audio: the bank, clip c at element c * clip_stride, c < bank->n_clips.  lengths: NULL or [n_clips], indexed by src.
 * noise: bank->n_noise rows of the audio's dtype, row k at element k * noise_stride; noise_lengths: [n_noise] int32 on
 * the device; the buffer holds (n_noise - 1) * noise_stride + noise_len_max elements.  aug: [B] records on the device.
 * For output clip b with record r:  c = r.src clamped into 0 .. n_clips-1;  len = lengths[c] clamped into 1280 .. L
 * (L without lengths);  and, when r.noise >= 0 and n_noise > 0:  k = min(r.noise, n_noise-1),  nlen = noise_lengths[k]
 * clamped into 1 .. noise_len_max,  off = r.noise_off mod nlen (the non-negative remainder).  For 0 <= i < len
 *   y'[i] = fl( fl(r.gain * y[i - r.shift]) + fl(r.noise_gain * nz[(off + i) mod nlen]) )
 * with y = clip c as step 1 of mfcc reads it (fp32, or int16 times 2^-15: exact), y[j] = 0 outside 0 .. len-1, and the
 * three fp32 operations rounded to nearest one by one (no fused multiply-add): numpy and torch reproduce the samples
 * bit for bit.  r.shift is any int32 (the difference does not overflow; |shift| >= len leaves no sample of y).  With
 * r.noise < 0 (or n_noise = 0) the noise term is ABSENT, y'[i] = fl(r.gain * y[i - r.shift]): the noise bank is not
 * read, so nothing in it -- NaN, inf -- can leak.  The wrap is numpy.pad(noise, mode='wrap')[:len]
 * (audioAugmentation.py:47-49) generalised by a start offset; gain = 0 gives the reference's noise-only clips.  The clip
 * keeps len samples, hence its frame count.  Steps 1 (the peak normalisation, if flagged, of y') to 10 of mfcc follow
 * unchanged; feats: [B, max_len, F].  The clamps above are the DEFINED behaviour for records outside their ranges: no
 * record value moves a read or a write outside the buffers.  One launch, no workspace, capturable.
 * Errors, all before any launch: everything mfcc refuses for d;  FASTGRNN_ERR_NULL_POINTER: bank, aug, audio, tables,
 * feats, one of mean / std, noise or noise_lengths while n_noise > 0;  FASTGRNN_ERR_BAD_SHAPE: n_clips < 1, n_noise < 0,
 * noise_stride < 1 while n_noise > 0 (clip_stride < 1 as in mfcc);  FASTGRNN_ERR_UNSUPPORTED: noise_len_max outside
 * 1 .. 2^24 while n_noise > 0. */
typedef struct fastgrnn_mfcc_aug {      /* one per OUTPUT clip, device array [B] */
  int32_t src;        /* bank clip to read, 0 .. n_clips-1 */
  int32_t shift;      /* samples; y'[i] = y[i - shift], zero outside 0 .. len-1 */
  int32_t noise;      /* noise bank row, or < 0: none */
  int32_t noise_off;  /* first noise sample, 0 .. nlen-1 */
  float   gain, noise_gain;
} fastgrnn_mfcc_aug;

#define FASTGRNN_MFCC_NOISE_LEN_MAX (1 << 24)
typedef struct fastgrnn_mfcc_bank {
  int32_t n_clips;                    /* clips in the audio bank, >= 1 */
  int32_t n_noise;                    /* rows of the noise bank, >= 0 */
  int64_t noise_stride;               /* elements between the starts of consecutive noise rows, >= 1 */
  int32_t noise_len_max;              /* 1 .. 2^24: the bound the kernel holds every noise length to */
  int32_t reserved;
} fastgrnn_mfcc_bank;

int fastgrnn_hip_mfcc_augment(const fastgrnn_mfcc_desc *d, const fastgrnn_mfcc_bank *bank, const void *audio,
                              const int32_t *lengths, const void *noise, const int32_t *noise_lengths,
                              const fastgrnn_mfcc_aug *aug, const void *tables, const float *mean, const float *std,
                              void *feats, void *workspace, size_t workspace_bytes, void *stream);

/* mfcc_stream -- mfcc for the detector's overlapping clips of ONE recording, with every frame of the recording taken
 * through the DFT and the mel projection once instead of once per clip that contains it.  Clip b is samples
 * b hop .. b hop + 15999 of the recording (audio: N elements, fp32 or int16, no alignment beyond the element's), and
 * its features are DEFINED as fastgrnn_hip_mfcc's with L = 16000, no lengths and clip_stride = hop; there are
 * (N - 16000) / hop + 1 clips.  hop is a multiple of 160, so clip b starts at frame kb = b hop / 160 of the recording:
 * its frame r is the recording's frame g = kb + r, samples 160 g - 200 .. 160 g + 199.  Frames 2..98 lie wholly inside
 * the clip -- their power spectrum and mel projection (steps 2-4) do not depend on the clip -- and frames 0, 1, 99, 100
 * see the clip's zero padding.  Two calls share a workspace of fastgrnn_hip_mfcc_stream_workspace_bytes(d) bytes
 * (a function of N alone; its layout is the library's business):
 *   mfcc_stream_frames, once per recording: the mel power (step 4, 128 fp32, before the dB) of every frame
 *     g = 0 .. N / 160 of the recording, zeros standing in for samples outside it, and the block maxima
 *     max|y[160 j .. 160 j + 159]|.  It reads and checks N, hop and audio_dtype; clip0, B, the feature settings and
 *     flags are ignored, so one call serves every mfcc_stream_clips on that recording.
 *   mfcc_stream_clips: clips clip0 .. clip0 + B - 1 into feats [B, max_len, F] fp32, contiguous and fully written, a
 *     frame pool exactly as mfcc leaves it: interior frames from the workspace, the four edge frames from the clip's own
 *     zero-padded samples, then steps 5-10.  A long recording is scored in bounded memory: frames once, clips in chunks.
 * Without FASTGRNN_MFCC_PEAK_NORMALIZE feats equals fastgrnn_hip_mfcc's BIT FOR BIT: every row of the three products is
 * the same k-ordered chain on the same operands, whichever workgroup computes it.  With the flag: m = max|y| over the
 * clip = the maximum of its 100 block maxima (exact, hence mfcc's m bit for bit); the edge frames are computed on
 * y / m as in mfcc; an interior frame's mel power is the recording's M scaled to fl(fl(M s) s), s = fl(1 / m), before
 * the 1e-10 floor of step 5; m == 0 leaves the clip unscaled.  The result differs from mfcc's by these fp32 roundings
 * only.  A clip's rows depend on the clip's own samples only.  Both calls: one launch on `stream`, no allocation, no
 * host decision on device data, no atomics -- capturable and repeatable bit for bit.
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER: d, audio, tables, workspace (clips: feats, exactly one of
 * mean / std);  FASTGRNN_ERR_BAD_SHAPE: N, hop, B, max_len or n_mfcc < 1, clip0 < 0, clip0 + B beyond the clip count,
 * top_db NaN, size overflow;  FASTGRNN_ERR_BAD_DTYPE: audio_dtype;  FASTGRNN_ERR_UNSUPPORTED: hop not a multiple of
 * 160, N < 16000 or N >= 2^31, n_mfcc / order / width / flags outside what mfcc takes;  FASTGRNN_ERR_WORKSPACE: fewer
 * bytes than the query answers, or a pointer not 256-byte aligned. */
typedef struct fastgrnn_mfcc_stream_desc {
  int64_t N;            /* elements of the recording, 16000 <= N < 2^31 */
  int32_t hop;          /* samples between clip starts: a multiple of 160, >= 160 */
  int32_t audio_dtype;  /* FASTGRNN_MFCC_AUDIO_F32 / _I16 */
  int32_t clip0, B;     /* this call featurises clips clip0 .. clip0+B-1 of (N-16000)/hop + 1 */
  int32_t n_mfcc, order, width, max_len;
  float top_db;
  uint32_t flags;       /* 0 or FASTGRNN_MFCC_PEAK_NORMALIZE */
} fastgrnn_mfcc_stream_desc;

size_t fastgrnn_hip_mfcc_stream_workspace_bytes(const fastgrnn_mfcc_stream_desc *d);
int fastgrnn_hip_mfcc_stream_frames(const fastgrnn_mfcc_stream_desc *d, const void *audio, const void *tables,
                                    void *workspace, size_t workspace_bytes, void *stream);
int fastgrnn_hip_mfcc_stream_clips(const fastgrnn_mfcc_stream_desc *d, const void *audio, const void *tables,
                                   void *workspace, size_t workspace_bytes, const float *mean, const float *std,
                                   void *feats, void *stream);

/* augment_draw -- the records of mfcc_augment from a counter-based generator, in one small launch: nothing is drawn on
 * the host, and a graph captured once draws new augmentations on every replay as step advances.  seed is a HOST value;
 * step[1] (int64) is a DEVICE scalar that is only read, like train_update's; index: [B] int32 on the device, copied to
 * src.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed_lo,
 * seed_hi); block j of clip b has the counter (b, step_lo, step_hi, j); x0..x3 = block 0, x4..x7 = block 1.  With
 * u(x) = (x >> 8) * 2^-24 and r(x, n) = ((uint64)x * n) >> 32:
 *   augment    = u(x0) < p_augment
 *   shift      = r(x1, 2 max_shift + 1) - max_shift
 *   gain       = fl(gain_lo + fl(fl(gain_hi - gain_lo) * u(x2)))
 *   with_noise = augment && n_noise > 0 && u(x3) < p_noise
 *   noise      = r(x4, n_noise)
 *   noise_off  = r(x5, nlen[noise]),   nlen = noise_lengths clamped into 1 .. noise_len_max
 *   noise_gain = fl(noise_gain_lo + fl(fl(noise_gain_hi - noise_gain_lo) * u(x6)))
 * A clip that is not augmented gets (src, 0, -1, 0, 1.0f, 0.0f); one augmented without noise gets noise = -1,
 * noise_off = 0 and noise_gain = 0.  Record b depends on (seed, step, b) alone: not on B, not on the launch geometry.
 * The reference's settings are p_noise = 0.5 and noise_gain_lo = noise_gain_hi = 0.1.
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (r, step, index, aug; noise_lengths while n_noise > 0),
 * FASTGRNN_ERR_BAD_SHAPE (B < 1; n_noise < 0; a probability outside [0,1] or NaN; lo > hi or a non-finite bound),
 * FASTGRNN_ERR_UNSUPPORTED (max_shift outside 0 .. 2^20; noise_len_max outside 1 .. 2^24 while n_noise > 0). */
#define FASTGRNN_AUGMENT_MAX_SHIFT (1 << 20)
typedef struct fastgrnn_augment_ranges {
  float p_augment, p_noise;
  int32_t max_shift, reserved;
  float gain_lo, gain_hi, noise_gain_lo, noise_gain_hi;
} fastgrnn_augment_ranges;

int fastgrnn_hip_augment_draw(int32_t B, uint64_t seed, const int64_t *step, const int32_t *index,
                              const fastgrnn_augment_ranges *r, int32_t n_noise, int32_t noise_len_max,
                              const int32_t *noise_lengths, fastgrnn_mfcc_aug *aug, void *stream);

/* train_schedule -- what a trainer iteration takes from outside the model, computed on the device from the step count:
 * the batch (a shuffled epoch order without replacement, the reference loader's shuffle=True), the learning rate (the
 * five schedules of the reference's configure_lr, trainClassifier.py:97-123, utils.py:116-143) and the IHT phase
 * (trainClassifier.py:251-259).  With it a training run is so many replays of one captured graph with no host write in
 * between.  One small launch on `stream`, no allocation, no workspace, no host decision on device data: capturable.
 * step[1] (int64) is a DEVICE scalar that is only read; s = max(step[0], 0) is the 0-BASED number of the iteration about
 * to run -- the fused optimizer's step_t as it stands BEFORE train_update's caller increments it, which is what
 * augment_draw reads.  d is a HOST struct.  Outputs, all on the device:
 *   index[B] int32     the batch's clip numbers, each in 0 .. N-1
 *   lr[1] float        the learning rate (train_update's lr)
 *   iht_mode[1] int32  0 / 1 / 2, train_update's codes; may be NULL while sparsify == 0 (otherwise 0 is written)
 *   where[4] int64     epoch, i_batch, slot = min(s, log_len - 1), 0
 * Position.  ticks = N / (B world) (integer division: drop_last), epoch = s / ticks, i_batch = s mod ticks,
 *   index[b] = perm_epoch((i_batch world + rank) B + b):  within an epoch the ranks' batches are disjoint and no clip
 * comes twice; N mod (B world) clips sit the epoch out, others in every epoch.
 * Permutation, stateless: k = the smallest even integer >= 2 with 2^k >= N, half = k / 2, mask = 2^half - 1.  One pass
 * maps x < 2^k to (L, R) = (x >> half, x & mask), runs four Feistel rounds r = 0 .. 3 of
 *   (L, R) <- (R, L ^ (P(R, r) & mask)),   P(R, r) = word 0 of Philox4x32-10 (augment_draw's generator) with the key
 *   (seed_lo, seed_hi) and the counter (R, epoch_lo, epoch_hi, 0x80000000 | r)
 * and gives x = (L << half) | R; the pass is repeated while x >= N (cycle walking; it ends because the pass is a
 * bijection of 0 .. 2^k-1, whose cycle through a start below N returns below N).  The top bit of the last counter word
 * keeps these counters apart from augment_draw's under one seed.  index[b] depends on (seed, N, B, world, rank, s, b)
 * alone, not on the launch geometry.
 * IHT phase, with sparsify != 0 (integer comparisons that agree with the reference's float ones for every pair):
 *   3 epoch < num_epochs: 0;   else 3 epoch < 2 num_epochs: 1 if i_batch mod trim_level == 0 else 2;   else 2.
 * Learning rate at it = s + lr_lead, in double, rounded once to float.  The reference calls scheduler.step() BEFORE
 * optimizer.step() (trainClassifier.py:244-249), so its iteration s runs at it = s + 1: lr_lead = 1; torch's documented
 * order is lr_lead = 0.  By lr_kind:
 *   FASTGRNN_LR_CONSTANT               lr_base
 *   FASTGRNN_LR_TRIANGLE               c = floor(1 + it / (2 stepsize)),  x = |it / stepsize - 2 c + 1|,
 *                                      lr_min + (lr_base - lr_min) gamma^(it / 3) x
 *   FASTGRNN_LR_COSINE                 lr_min + (lr_base - lr_min) (1 + cos(pi it / t_max)) / 2   (the closed form;
 *                                      torch's recursive form differs by rounding and divides by zero at some t_max)
 *   FASTGRNN_LR_EXPONENTIAL            lr_base gamma^it
 *   FASTGRNN_LR_STEP                   lr_base gamma^floor(it / step_size)
 *   FASTGRNN_LR_EXPONENTIAL_RESETTING  e = it - reset if it > reset else it,  lr_base gamma^e
 * Fields that a kind does not name are not read.
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (d, step, index, lr, where; iht_mode while sparsify != 0),
 * FASTGRNN_ERR_BAD_SHAPE (B < 1; world < 1; rank outside 0 .. world-1; B world > 2^31 - 1 or N < B world; num_epochs,
 * trim_level or log_len < 1; lr_lead other than 0, 1; lr_base or lr_min negative or not finite; gamma <= 0 or not
 * finite on the kinds that read it; stepsize likewise on TRIANGLE, t_max on COSINE; step_size < 1 on STEP; reset < 0
 * on EXPONENTIAL_RESETTING), FASTGRNN_ERR_UNSUPPORTED (an unknown lr_kind).  No value of step[0] moves a write outside
 * index[0 .. B). */
#define FASTGRNN_LR_CONSTANT 0
#define FASTGRNN_LR_TRIANGLE 1
#define FASTGRNN_LR_COSINE 2
#define FASTGRNN_LR_EXPONENTIAL 3
#define FASTGRNN_LR_STEP 4
#define FASTGRNN_LR_EXPONENTIAL_RESETTING 5
typedef struct fastgrnn_schedule_desc {
  int32_t N, B, world, rank;          /* clips in the bank, clips per batch and rank, ranks, this rank */
  uint64_t seed;
  int32_t num_epochs, trim_level;     /* the IHT phases' thirds; a threshold every trim_level batches */
  int32_t sparsify;                   /* 0: the phase is always 0 */
  int32_t lr_kind, lr_lead, reserved;
  int64_t log_len;                    /* >= 1: where[2] stays below it */
  double lr_base, lr_min, gamma, stepsize, t_max;
  int64_t step_size, reset;
} fastgrnn_schedule_desc;

int fastgrnn_hip_train_schedule(const fastgrnn_schedule_desc *d, const int64_t *step, int32_t *index, float *lr,
                                int32_t *iht_mode, int64_t *where, void *stream);

/* train_schedule_rolling, rolling_exchange -- the reference's rolling mode (options.rolling, trainClassifier.py:174-221,
 * model.py:135-156), the only one in which a batch does not start from the zero state: each layer's final states are
 * scattered into a "hidden bag" of M = B bag_count rows at shuffled positions, the next batch starts from bag rows
 * 0 .. B-1, and the early epochs are cut short and start from cleared bags.  Position, shuffle and bag exchange are
 * functions of the step count and the seed, so a rolling run too is so many replays of one captured graph.
 * Both calls: one small launch on `stream`, no allocation, no workspace, no host decision on device data: capturable.
 * d, r and the three pointer arrays are HOST data; step[1] is train_schedule's device scalar, s = max(step[0], 0).
 * Constants, all integers:  ticks_full = N / (B world)  (drop_last),
 *   max_roll = min(ticks_full, max_rolling_length + 2, num_epochs + 2),   n_short = max(0, max_roll - 2).
 * Position.  Epoch e < n_short is a SHORT epoch of e + 2 iterations (the reference's rolling_length = e + 3, trained
 * for i_batch = 0 .. e + 1 and left at the `break`); it starts at iteration e (e + 3) / 2.  The epochs after them have
 * ticks_full iterations each, so a run has  n_short (n_short + 3) / 2 + (num_epochs - n_short) ticks_full  iterations
 * (the reference's total_iterations wherever ticks_full >= 2; at ticks_full == 1 its count disagrees with its own
 * loop, and both calls refuse that).  Iterations past the run's end continue in the full-epoch pattern.
 *   fresh(s): the first iteration of every short epoch and of epoch n_short (s = 0 where there is no short epoch):
 *             the batch starts from the zero state and nothing is scattered;
 *   zero(s):  the first iteration of every short epoch: the bags are cleared (the reference's init_hidden_bag).
 * train_schedule_rolling is train_schedule at that position -- index[b] = perm_epoch((i_batch world + rank) B + b), so
 * a short epoch uses the first e + 2 batches of its order; the IHT rule on (epoch, i_batch); the learning rate at
 * it = s + lr_lead from the descriptor's constants (the caller derives them from the reference's fractional
 * ticks = total_iterations / num_epochs) -- with  where[4] = epoch, i_batch, slot, fresh | zero << 1.  Of r it reads
 * max_rolling_length and bag_count alone.
 * rolling_exchange, per layer l < layers (model.py:145-156 in one launch for all layers):
 *   state[l]:[B,H_l] fp32  the previous iteration's final states (read)
 *   bag[l]:[M,H_l] fp32    the hidden bag
 *   h0[l]:[B,H_l] fp32     the states this iteration starts from (written; must not overlap state[l] or bag[l])
 *   zero(s):   bag[l] becomes +0.0 everywhere;
 *   fresh(s):  h0[l] becomes +0.0 everywhere and the bag is not touched otherwise (on the first iteration of epoch
 *              n_short it keeps what the last short epoch left, as in the reference);
 *   otherwise  bag[l][pi_s(j)] = state[l][j] for j < B, then h0[l][r] = bag[l][r] for r < B, reading the bag AFTER the
 *              scatter.  Computed without any ordering inside the launch: h0[l][r] = state[l][pi_s^-1(r)] where
 *              pi_s^-1(r) < B, else the old bag[l][r], which nothing writes in that case.  Rows are copied bit for bit.
 * pi_s, the same for all layers (the reference draws one np.random.shuffle per iteration), is train_schedule's keyed
 * permutation over 0 .. M-1: k = the smallest even integer >= 2 with 2^k >= M, four Feistel rounds per pass with
 *   P(R, r) = word 0 of Philox4x32-10 with the key (seed_lo, seed_hi) and the counter (R, s_lo, s_hi, 0xC0000000 | r),
 * cycle-walked while the result is >= M.  The two top bits of the last counter word keep these counters apart from
 * augment_draw's (last word 0, 1) and the epoch order's (0x80000000 | r).  The inverse pass runs the rounds r = 3 .. 0
 * as (L, R) <- (R ^ (P(L, r) & mask), L) and cycle-walks the same way.
 * The exchange depends on (d, r, step[0], state, bag) alone: it recomputes the position and does not read `where`, so
 * there is no ordering contract with the schedule call.  Rows move 16 bytes per lane where H_l mod 4 == 0 and the
 * layer's three pointers are 16-byte aligned, one dword per lane otherwise.
 * Errors, all before any launch: FASTGRNN_ERR_NULL_POINTER (d, r, step and every output of train_schedule; the three
 * arrays and their first `layers` entries), train_schedule's refusals of d, FASTGRNN_ERR_BAD_SHAPE (ticks_full < 2;
 * max_rolling_length < 0; bag_count < 1; B bag_count > 2^31 - 1; for rolling_exchange also layers outside 1 .. 3 or
 * H[l] < 1 for an l < layers).  No value of step[0] moves a write outside index[0 .. B), bag[l] or h0[l]. */
typedef struct fastgrnn_rolling_desc {
  int32_t max_rolling_length;         /* >= 0; options.max_rolling_length */
  int32_t bag_count;                  /* >= 1; rows of a bag = B * bag_count; the reference's 100 */
  int32_t layers, reserved;           /* 1 .. 3 */
  int32_t H[4];                       /* H[l] >= 1 for l < layers */
} fastgrnn_rolling_desc;

int fastgrnn_hip_train_schedule_rolling(const fastgrnn_schedule_desc *d, const fastgrnn_rolling_desc *r,
                                        const int64_t *step, int32_t *index, float *lr, int32_t *iht_mode,
                                        int64_t *where, void *stream);
int fastgrnn_hip_rolling_exchange(const fastgrnn_schedule_desc *d, const fastgrnn_rolling_desc *r, const int64_t *step,
                                  const float *const state[3], float *const bag[3], float *const h0[3], void *stream);

/* frame_gemm -- the one genuinely dense, non-recurrent contraction of a layer, as a call of its own:
 *   P[rows, H] = X[rows, F] . W^T,   W:[H,F]  (rows = T*B; the reference computes it per step, `mm` at .cu:356).
 * forward_unroll runs exactly this launch in front of the scan for layers whose input is wider than 32 (the scan of a
 * 32-feature layer has the product fused); it is exported so that its MFMA utilisation can be measured and reported by
 * itself (bench.py: `wx_gemm`).  fp32 (dtype FASTGRNN_F32) or bf16 x with fp32 p (FASTGRNN_BF16_IO); (H, F) one of
 * the wide-layer shapes of the table above, else FASTGRNN_ERR_UNSUPPORTED.  No workspace. */
int fastgrnn_hip_frame_gemm(size_t rows, int32_t H, int32_t F, const void *x, const void *w, void *p, int32_t dtype,
                            void *stream);

/* ---- training-mode BatchNorm cell (FASTGRNN_FLAG_BN_TRAIN) --------------------------------------------------------
 * Per layer and frame t, over the B utterances (reference rnn.py:373-414, BatchNorm1d in training mode):
 *   wC = x_t . w^T,  uC = h_{t-1} . u^T              (w:[H,F], u:[H,H]: this ABI's [out,in] layout)
 *   s  = bn_w(wC) + bn_u(uC)                         batch mean, biased batch variance, eps, gamma, beta
 *   z  = gate(bn_gate(s + bias_gate)),  c = tanh(bn_update(s + bias_update))
 *   h_t = z . h_{t-1} + (sigmoid(zeta) (1 - z) + sigmoid(nu)) . c
 * Each BatchNorm layer is passed explicitly.  gamma, beta, running_mean, running_var: [H] fp32.  momentum < 0 means
 * torch's momentum=None (cumulative average: factor 1 / (num_batches_tracked + t + 1) at frame t, num_batches_tracked
 * read from the device and NOT incremented -- the caller adds T after the call); otherwise num_batches_tracked may be
 * NULL.  The forward updates every running statistic T times in frame order, r <- (1-m) r + m stat_t, with the
 * unbiased variance var * B/(B-1) (bn_gate / bn_update: the mean of s + bias_gate / bias_update). */
typedef struct fastgrnn_bn_layer {
  const void *gamma, *beta;
  void *running_mean, *running_var;
  const int64_t *num_batches_tracked;
  double eps, momentum;
} fastgrnn_bn_layer;

typedef struct fastgrnn_bn_params {
  fastgrnn_bn_layer w, u, gate, update;          /* bn_w, bn_u, bn_gate, bn_update */
} fastgrnn_bn_params;

/* gradients of the eight BatchNorm affine parameters, [H] each, overwritten */
typedef struct fastgrnn_bn_grads {
  void *d_gamma_w, *d_beta_w, *d_gamma_u, *d_beta_u, *d_gamma_gate, *d_beta_gate, *d_gamma_update, *d_beta_update;
} fastgrnn_bn_grads;

/* 1 if the descriptor (flags FASTGRNN_FLAG_BN_TRAIN, optionally FASTGRNN_FLAG_BATCH_MAJOR, nothing else) runs on the
 * training kernels, else 0: fp32, dense, gate sigmoid / relu / tanh, update tanh, B >= 2, any T, and
 *   H = 128 with F = 32 / 64 / 128 / 256,   H = 256 with F = 32 / 64 / 128
 * (the FASTGRNN_FLAG_PREACT_AFFINE path-2 table).  Time-major [T,B,.] or batch-major [B,T,.] sequences. */
int fastgrnn_hip_bn_train_supported(const fastgrnn_desc *d);
/* workspace bytes of the two calls (0 for an unsupported descriptor) */
size_t fastgrnn_hip_bn_train_forward_workspace_bytes(const fastgrnn_desc *d);
size_t fastgrnn_hip_bn_train_backward_workspace_bytes(const fastgrnn_desc *d);

/* forward: x, h0 -> hs (sequences in the layout of d->flags, h0 [B,H]); saved: [T,B,H] fp32 (time-major whatever the
 * layout: uC of every frame), stats: [T, 9H] fp64 (per frame and unit: mean and biased variance of wC and of uC,
 * their biased covariance; mean and biased variance of d = bn_w(wC) - beta_w + bn_u(uC) - beta_u, its co-moments with
 * the normalised wC and uC); both are read by the backward.  Updates the running statistics in bn.  p->w, p->u, bias_gate,
 * bias_update, zeta, nu as in fastgrnn_params.  Errors: FASTGRNN_ERR_NULL_POINTER, FASTGRNN_ERR_BAD_SHAPE (B < 2:
 * torch's "more than 1 value per channel"), FASTGRNN_ERR_UNSUPPORTED (flag missing, other flags, dtype, factorised
 * operands, shapes off the table), FASTGRNN_ERR_WORKSPACE. */
int fastgrnn_hip_bn_train_forward(const fastgrnn_desc *d, const fastgrnn_params *p, const fastgrnn_bn_params *bn,
                                  const void *x, const void *h0, void *hs, void *saved, void *stats,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* backward: grad_hs (the layout of hs) -> g->d_x (may be NULL), d_h0, d_w, d_u ([out,in]), d_bias_gate,
 * d_bias_update, d_zeta, d_nu and the eight BatchNorm affine gradients in bg.  beta_w, beta_u, bias_gate and
 * bias_update only shift the input of a batch-normalised layer: their gradients are written as exact zeros.
 * saved / stats: the forward's.  Reads the BatchNorm gammas, betas and eps of bn (not its running statistics). */
int fastgrnn_hip_bn_train_backward(const fastgrnn_desc *d, const fastgrnn_params *p, const fastgrnn_bn_params *bn,
                                   const void *grad_hs, const void *x, const void *hs, const void *saved,
                                   const void *stats, const void *h0, const fastgrnn_grads *g,
                                   const fastgrnn_bn_grads *bg, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* Test hook, not part of the reference boundary: one launch that leaves `pattern` in every CU's LDS and vector
 * registers (on-chip state is not cleared between kernels).  tests/test_hip_state_independence.py runs it before the
 * operators with a NaN pattern: results must not change, i.e. no kernel reads LDS or registers it did not write. */
int fastgrnn_hip_debug_poison_cu_state(uint32_t pattern, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTGRNN_HIP_H */
