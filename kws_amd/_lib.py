"""ctypes binding of libfastgrnn_hip.so (C ABI: include/fastgrnn_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C kws_amd/csrc``).
There is NO fallback: if the shared object is missing or does not export the ABI
this module raises, and every operator in ``kws_amd`` fails with it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FASTGRNN_HIP_LIB: A/B a differently built library (tools/) without touching the in-tree one
LIB_PATH = os.environ.get("FASTGRNN_HIP_LIB") or os.path.join(_HERE, "csrc", "libfastgrnn_hip.so")

ABI_VERSION = 1

F32, F64, BF16_IO = 0, 1, 2     # fastgrnn_dtype; BF16_IO: bf16 sequences, fp32 everything else
FLAG_FORCE_GENERIC = 1
FLAG_FORCE_F32_MFMA = 2
FLAG_SAVE_PREACT = 4
FLAG_FWD_4WAVE = 8            # A/B: older 4-wave forward shape
FLAG_FWD_BF16X3 = 64          # A/B: forward state product on three bf16 planes
FLAG_X_BFT = 128              # x / d_x are the trainer's [B,F,T]
FLAG_GRAD_LAST = 256          # backward_unroll: grad_h is [B,H], the gradient of the last state alone (model.py:227)
FLAG_HS_LAST = 512            # forward_unroll (inference, no saved tensors): hs is [B,H] = h_T
FLAG_BATCH_MAJOR = 16         # sequences are [B,T,.] (batch_first) instead of [T,B,.]
FLAG_PREACT_AFFINE = 1024     # fastgrnn_hip_forward_unroll_affine: per-unit pre-activation scales (eval-mode BatchNorm)
FLAG_BN_TRAIN = 2048          # fastgrnn_hip_bn_train_*: the training-mode BatchNorm cell
FLAG_ZERO_EXTEND = 4096       # odd H <= 256 / F on kernel path 2 by zero-padding to a path-2 shape (a permission)
FLAG_NO_INPUT_GRAD = 8192     # backward_unroll: d_x may be NULL on dense H=128/F=32 too (a permission)
# FASTGRNN_FLAG_BWD_8WAVE (A/B: the 8-wave shape of the H=128/F=32 backward without input gradient).  Not a FLAG_*
# name: those are the set tests/support.py re-exports, one by one.
AB_BWD_8WAVE = 32

# include/fastgrnn_hip.h: fastgrnn_nonlinearity.  0..2 are the reference's table
# (rnn.py:478,751); 3..5 the CPU cell's quantised family (rnn.py:53-60).
NONLINEARITY = {"sigmoid": 0, "relu": 1, "tanh": 2, "quantTanh": 3, "quantSigm": 4, "quantSigm4": 5}

EXPORTS = (
    "fastgrnn_hip_abi_version", "fastgrnn_hip_status_string", "fastgrnn_hip_kernel_path",
    "fastgrnn_hip_forward_workspace_bytes", "fastgrnn_hip_backward_workspace_bytes",
    "fastgrnn_hip_forward_unroll", "fastgrnn_hip_backward_unroll",
    "fastgrnn_hip_forward", "fastgrnn_hip_backward",
    "fastgrnn_hip_head_workspace_bytes", "fastgrnn_hip_head_xent", "fastgrnn_hip_debug_poison_cu_state",
    "fastgrnn_hip_frame_gemm", "fastgrnn_hip_forward_unroll_affine",
    "fastgrnn_hip_bn_train_supported", "fastgrnn_hip_bn_train_forward_workspace_bytes",
    "fastgrnn_hip_bn_train_backward_workspace_bytes", "fastgrnn_hip_bn_train_forward", "fastgrnn_hip_bn_train_backward",
    "fastgrnn_hip_zero_extend_plan", "fastgrnn_hip_plan",
    "fastgrnn_hip_windows_supported", "fastgrnn_hip_forward_windows_workspace_bytes", "fastgrnn_hip_forward_windows",
    "fastgrnn_hip_train_windows_supported", "fastgrnn_hip_train_windows_forward_workspace_bytes",
    "fastgrnn_hip_train_windows_backward_workspace_bytes", "fastgrnn_hip_forward_windows_train",
    "fastgrnn_hip_backward_windows",
    "fastgrnn_hip_head_predict_workspace_bytes", "fastgrnn_hip_head_predict", "fastgrnn_hip_vote_windows",
    "fastgrnn_hip_train_update", "fastgrnn_hip_optim_update",
    "fastgrnn_hip_mfcc_tables_bytes", "fastgrnn_hip_mfcc_init_tables", "fastgrnn_hip_mfcc_workspace_bytes",
    "fastgrnn_hip_mfcc", "fastgrnn_hip_mfcc_augment", "fastgrnn_hip_augment_draw", "fastgrnn_hip_train_schedule",
    "fastgrnn_hip_mfcc_stream_workspace_bytes", "fastgrnn_hip_mfcc_stream_frames", "fastgrnn_hip_mfcc_stream_clips",
    "fastgrnn_hip_train_schedule_rolling", "fastgrnn_hip_rolling_exchange",
    "fastgrnn_hip_grad_guard_workspace_bytes", "fastgrnn_hip_grad_guard", "fastgrnn_hip_train_update_guarded",
    "fastgrnn_hip_optim_update_guarded",
)


class Desc(C.Structure):
    _fields_ = [("T", C.c_int32), ("B", C.c_int32), ("F", C.c_int32), ("H", C.c_int32),
                ("w_rank", C.c_int32), ("u_rank", C.c_int32),
                ("gate_nl", C.c_int32), ("update_nl", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("w", "u", "w1", "w2", "u1", "u2", "bias_gate", "bias_update", "zeta", "nu")]


class Grads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("d_x", "d_bias_gate", "d_bias_update", "d_zeta", "d_nu", "d_h0",
                 "d_w", "d_u", "d_w1", "d_w2", "d_u1", "d_u2")]


class BnLayer(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p),
                ("eps", C.c_double), ("momentum", C.c_double)]


class BnParams(C.Structure):
    _fields_ = [("w", BnLayer), ("u", BnLayer), ("gate", BnLayer), ("update", BnLayer)]


class BnGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("d_gamma_w", "d_beta_w", "d_gamma_u", "d_beta_u", "d_gamma_gate", "d_beta_gate",
                 "d_gamma_update", "d_beta_update")]


class ZextPlan(C.Structure):
    """fastgrnn_zext_plan: what FLAG_ZERO_EXTEND does for a descriptor."""
    _fields_ = [("forward", C.c_int32), ("backward", C.c_int32), ("Hp", C.c_int32), ("Fp", C.c_int32),
                ("dx_optional", C.c_int32), ("reserved", C.c_int32), ("saved_bytes", C.c_size_t)]


class Plan(C.Structure):
    """fastgrnn_plan: what the calls of a descriptor run on and what that route needs from the caller."""
    _fields_ = [("path", C.c_int32 * 2), ("forward_ws_optional", C.c_int32), ("dx_optional", C.c_int32),
                ("rank_space_cols", C.c_int32), ("reserved", C.c_int32), ("workspace_bytes", C.c_size_t * 2),
                ("zext", ZextPlan)]


UPDATE_MAX_SEGS = 32            # FASTGRNN_UPDATE_MAX_SEGS: segments per launch of fastgrnn_hip_train_update
UPDATE_MAX_N = 1 << 22          # FASTGRNN_UPDATE_MAX_N: elements per segment
ADAM, SGD = 0, 1                # fastgrnn_update_hyper.algo
IHT_NONE, IHT_THRESHOLD, IHT_SUPPORT = 0, 1, 2     # the device scalar iht_mode


class UpdateSeg(C.Structure):
    """fastgrnn_update_seg: one parameter tensor of fastgrnn_hip_train_update."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state0", C.c_void_p), ("state1", C.c_void_p),
                ("support", C.c_void_p), ("n", C.c_int64), ("keep_rank", C.c_int64), ("iht", C.c_int32),
                ("reserved", C.c_int32)]


class UpdateHyper(C.Structure):
    """fastgrnn_update_hyper."""
    _fields_ = [("algo", C.c_int32), ("nesterov", C.c_int32), ("beta1_or_momentum", C.c_double),
                ("beta2_or_dampening", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double)]


RMSPROP, ADAGRAD, ADADELTA, ADAMAX, ASGD, RPROP = 2, 3, 4, 5, 6, 7     # fastgrnn_optim_hyper.algo
RMSPROP_CENTERED = 1            # fastgrnn_optim_hyper.flags


class OptimSeg(C.Structure):
    """fastgrnn_optim_seg: one parameter tensor of fastgrnn_hip_optim_update."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state", C.c_void_p * 3), ("support", C.c_void_p),
                ("n", C.c_int64), ("keep_rank", C.c_int64), ("iht", C.c_int32), ("reserved", C.c_int32)]


class OptimHyper(C.Structure):
    """fastgrnn_optim_hyper."""
    _fields_ = [("algo", C.c_int32), ("flags", C.c_int32), ("h", C.c_double * 6), ("weight_decay", C.c_double)]


GUARD_SKIP_NONFINITE = 1        # FASTGRNN_GUARD_SKIP_NONFINITE: fastgrnn_hip_grad_guard's flags


class GuardSeg(C.Structure):
    """fastgrnn_guard_seg: one gradient tensor of fastgrnn_hip_grad_guard."""
    _fields_ = [("grad", C.c_void_p), ("n", C.c_int64)]


class GuardState(C.Structure):
    """fastgrnn_guard_state: the 32 bytes on the device that the guard writes and the guarded updates read."""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("skip", C.c_int32), ("reserved", C.c_int32),
                ("applied", C.c_int64), ("skipped", C.c_int64)]


MFCC_PEAK_NORMALIZE = 1         # FASTGRNN_MFCC_PEAK_NORMALIZE
MFCC_AUDIO_F32, MFCC_AUDIO_I16 = 0, 1
MFCC_MIN_SAMPLES, MFCC_MAX_SAMPLES = 1280, 16000     # the clip lengths fastgrnn_hip_mfcc takes


class MfccDesc(C.Structure):
    """fastgrnn_mfcc_desc."""
    _fields_ = [("B", C.c_int32), ("L", C.c_int32), ("clip_stride", C.c_int64), ("audio_dtype", C.c_int32),
                ("n_mfcc", C.c_int32), ("order", C.c_int32), ("width", C.c_int32), ("max_len", C.c_int32),
                ("top_db", C.c_float), ("flags", C.c_uint32)]


MFCC_STREAM_CLIP, MFCC_STREAM_HOP_UNIT = 16000, 160     # fastgrnn_hip_mfcc_stream_*: the clip length, what a hop is a multiple of


class MfccStreamDesc(C.Structure):
    """fastgrnn_mfcc_stream_desc."""
    _fields_ = [("N", C.c_int64), ("hop", C.c_int32), ("audio_dtype", C.c_int32), ("clip0", C.c_int32), ("B", C.c_int32),
                ("n_mfcc", C.c_int32), ("order", C.c_int32), ("width", C.c_int32), ("max_len", C.c_int32),
                ("top_db", C.c_float), ("flags", C.c_uint32)]


MFCC_NOISE_LEN_MAX = 1 << 24     # FASTGRNN_MFCC_NOISE_LEN_MAX
AUGMENT_MAX_SHIFT = 1 << 20      # FASTGRNN_AUGMENT_MAX_SHIFT


class MfccAug(C.Structure):
    """fastgrnn_mfcc_aug: one augmentation record (a row of the ``[B, 6]`` int32 tensors of ``kws_amd.augment``)."""
    _fields_ = [("src", C.c_int32), ("shift", C.c_int32), ("noise", C.c_int32), ("noise_off", C.c_int32),
                ("gain", C.c_float), ("noise_gain", C.c_float)]


class MfccBank(C.Structure):
    """fastgrnn_mfcc_bank."""
    _fields_ = [("n_clips", C.c_int32), ("n_noise", C.c_int32), ("noise_stride", C.c_int64),
                ("noise_len_max", C.c_int32), ("reserved", C.c_int32)]


class AugmentRanges(C.Structure):
    """fastgrnn_augment_ranges."""
    _fields_ = [("p_augment", C.c_float), ("p_noise", C.c_float), ("max_shift", C.c_int32), ("reserved", C.c_int32),
                ("gain_lo", C.c_float), ("gain_hi", C.c_float), ("noise_gain_lo", C.c_float),
                ("noise_gain_hi", C.c_float)]


# fastgrnn_schedule_desc.lr_kind, by the reference's scheduler names (trainClassifier.py:107-122)
LR_KINDS = {None: 0, "TriangleLR": 1, "CosineAnnealingLR": 2, "ExponentialLR": 3, "StepLR": 4,
            "ExponentialResettingLR": 5}


class ScheduleDesc(C.Structure):
    """fastgrnn_schedule_desc."""
    _fields_ = [("N", C.c_int32), ("B", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32), ("seed", C.c_uint64),
                ("num_epochs", C.c_int32), ("trim_level", C.c_int32), ("sparsify", C.c_int32), ("lr_kind", C.c_int32),
                ("lr_lead", C.c_int32), ("reserved", C.c_int32), ("log_len", C.c_int64),
                ("lr_base", C.c_double), ("lr_min", C.c_double), ("gamma", C.c_double), ("stepsize", C.c_double),
                ("t_max", C.c_double), ("step_size", C.c_int64), ("reset", C.c_int64)]


ROLLING_MAX_LAYERS = 3          # layers of one fastgrnn_hip_rolling_exchange launch


class RollingDesc(C.Structure):
    """fastgrnn_rolling_desc."""
    _fields_ = [("max_rolling_length", C.c_int32), ("bag_count", C.c_int32), ("layers", C.c_int32),
                ("reserved", C.c_int32), ("H", C.c_int32 * 4)]


class FastGRNNLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load (once) and return the ctypes handle; raise loudly if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FastGRNNLibraryError(
            "libfastgrnn_hip.so not found at %s -- build it first: "
            "python -c 'import __graft_entry__ as g; g.build()'  (or make -C kws_amd/csrc). "
            "kws_amd has no CPU or eager fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise FastGRNNLibraryError("%s does not export %s" % (LIB_PATH, name))
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    DP, PP, GP = C.POINTER(Desc), C.POINTER(Params), C.POINTER(Grads)
    lib.fastgrnn_hip_abi_version.restype = i32
    lib.fastgrnn_hip_status_string.restype = C.c_char_p
    lib.fastgrnn_hip_status_string.argtypes = [i32]
    lib.fastgrnn_hip_kernel_path.restype = i32
    lib.fastgrnn_hip_kernel_path.argtypes = [DP, i32]
    for f in (lib.fastgrnn_hip_forward_workspace_bytes, lib.fastgrnn_hip_backward_workspace_bytes):
        f.restype = sz
        f.argtypes = [DP]
    lib.fastgrnn_hip_forward_unroll.restype = i32
    lib.fastgrnn_hip_forward_unroll.argtypes = [DP, PP, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_forward_unroll_affine.restype = i32
    lib.fastgrnn_hip_forward_unroll_affine.argtypes = [DP, PP, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_backward_unroll.restype = i32
    lib.fastgrnn_hip_backward_unroll.argtypes = [DP, PP, vp, vp, vp, vp, vp, vp, GP, vp, sz, vp]
    lib.fastgrnn_hip_forward.restype = i32
    lib.fastgrnn_hip_forward.argtypes = [DP, PP, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_backward.restype = i32
    lib.fastgrnn_hip_backward.argtypes = [DP, PP, vp, vp, vp, vp, vp, GP, vp, sz, vp]
    lib.fastgrnn_hip_debug_poison_cu_state.restype = i32
    lib.fastgrnn_hip_debug_poison_cu_state.argtypes = [C.c_uint32, vp]
    lib.fastgrnn_hip_head_workspace_bytes.restype = sz
    lib.fastgrnn_hip_head_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fastgrnn_hip_head_xent.restype = i32
    lib.fastgrnn_hip_head_xent.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_head_predict_workspace_bytes.restype = sz
    lib.fastgrnn_hip_head_predict_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.fastgrnn_hip_head_predict.restype = i32
    lib.fastgrnn_hip_head_predict.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_vote_windows.restype = i32
    lib.fastgrnn_hip_vote_windows.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
    lib.fastgrnn_hip_train_update.restype = i32
    lib.fastgrnn_hip_train_update.argtypes = [C.POINTER(UpdateHyper), C.POINTER(UpdateSeg), C.c_int32, vp, vp, vp, vp]
    lib.fastgrnn_hip_optim_update.restype = i32
    lib.fastgrnn_hip_optim_update.argtypes = [C.POINTER(OptimHyper), C.POINTER(OptimSeg), C.c_int32, vp, vp, vp, vp, vp]
    lib.fastgrnn_hip_grad_guard_workspace_bytes.restype = sz
    lib.fastgrnn_hip_grad_guard_workspace_bytes.argtypes = [C.c_int32]
    lib.fastgrnn_hip_grad_guard.restype = i32
    lib.fastgrnn_hip_grad_guard.argtypes = [C.POINTER(GuardSeg), C.c_int32, C.c_double, C.c_int32, vp, vp, sz, vp]
    lib.fastgrnn_hip_train_update_guarded.restype = i32
    lib.fastgrnn_hip_train_update_guarded.argtypes = [C.POINTER(UpdateHyper), C.POINTER(UpdateSeg), C.c_int32, vp, vp, vp, vp]
    lib.fastgrnn_hip_optim_update_guarded.restype = i32
    lib.fastgrnn_hip_optim_update_guarded.argtypes = [C.POINTER(OptimHyper), C.POINTER(OptimSeg), C.c_int32, vp, vp, vp, vp, vp]
    MD = C.POINTER(MfccDesc)
    lib.fastgrnn_hip_mfcc_tables_bytes.restype = sz
    lib.fastgrnn_hip_mfcc_tables_bytes.argtypes = []
    lib.fastgrnn_hip_mfcc_init_tables.restype = i32
    lib.fastgrnn_hip_mfcc_init_tables.argtypes = [vp, vp]
    lib.fastgrnn_hip_mfcc_workspace_bytes.restype = sz
    lib.fastgrnn_hip_mfcc_workspace_bytes.argtypes = [MD]
    lib.fastgrnn_hip_mfcc.restype = i32
    lib.fastgrnn_hip_mfcc.argtypes = [MD, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_mfcc_augment.restype = i32
    lib.fastgrnn_hip_mfcc_augment.argtypes = [MD, C.POINTER(MfccBank), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    SD = C.POINTER(MfccStreamDesc)
    lib.fastgrnn_hip_mfcc_stream_workspace_bytes.restype = sz
    lib.fastgrnn_hip_mfcc_stream_workspace_bytes.argtypes = [SD]
    lib.fastgrnn_hip_mfcc_stream_frames.restype = i32
    lib.fastgrnn_hip_mfcc_stream_frames.argtypes = [SD, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_mfcc_stream_clips.restype = i32
    lib.fastgrnn_hip_mfcc_stream_clips.argtypes = [SD, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.fastgrnn_hip_augment_draw.restype = i32
    lib.fastgrnn_hip_augment_draw.argtypes = [C.c_int32, C.c_uint64, vp, vp, C.POINTER(AugmentRanges), C.c_int32,
                                              C.c_int32, vp, vp, vp]
    lib.fastgrnn_hip_train_schedule.restype = i32
    lib.fastgrnn_hip_train_schedule.argtypes = [C.POINTER(ScheduleDesc), vp, vp, vp, vp, vp, vp]
    RD, P3 = C.POINTER(RollingDesc), C.POINTER(vp * 3)
    lib.fastgrnn_hip_train_schedule_rolling.restype = i32
    lib.fastgrnn_hip_train_schedule_rolling.argtypes = [C.POINTER(ScheduleDesc), RD, vp, vp, vp, vp, vp, vp]
    lib.fastgrnn_hip_rolling_exchange.restype = i32
    lib.fastgrnn_hip_rolling_exchange.argtypes = [C.POINTER(ScheduleDesc), RD, vp, P3, P3, P3, vp]
    lib.fastgrnn_hip_frame_gemm.restype = i32
    lib.fastgrnn_hip_frame_gemm.argtypes = [sz, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp]
    BP, BG = C.POINTER(BnParams), C.POINTER(BnGrads)
    lib.fastgrnn_hip_bn_train_supported.restype = i32
    lib.fastgrnn_hip_bn_train_supported.argtypes = [DP]
    for f in (lib.fastgrnn_hip_bn_train_forward_workspace_bytes, lib.fastgrnn_hip_bn_train_backward_workspace_bytes):
        f.restype = sz
        f.argtypes = [DP]
    lib.fastgrnn_hip_bn_train_forward.restype = i32
    lib.fastgrnn_hip_bn_train_forward.argtypes = [DP, PP, BP, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_bn_train_backward.restype = i32
    lib.fastgrnn_hip_bn_train_backward.argtypes = [DP, PP, BP, vp, vp, vp, vp, vp, vp, GP, BG, vp, sz, vp]
    lib.fastgrnn_hip_zero_extend_plan.restype = i32
    lib.fastgrnn_hip_zero_extend_plan.argtypes = [DP, C.POINTER(ZextPlan)]
    lib.fastgrnn_hip_plan.restype = i32
    lib.fastgrnn_hip_plan.argtypes = [DP, C.POINTER(Plan)]
    lib.fastgrnn_hip_windows_supported.restype = i32
    lib.fastgrnn_hip_windows_supported.argtypes = [DP]
    lib.fastgrnn_hip_forward_windows_workspace_bytes.restype = sz
    lib.fastgrnn_hip_forward_windows_workspace_bytes.argtypes = [DP, sz]
    lib.fastgrnn_hip_forward_windows.restype = i32
    lib.fastgrnn_hip_forward_windows.argtypes = [DP, PP, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_train_windows_supported.restype = i32
    lib.fastgrnn_hip_train_windows_supported.argtypes = [DP]
    for f in (lib.fastgrnn_hip_train_windows_forward_workspace_bytes,
              lib.fastgrnn_hip_train_windows_backward_workspace_bytes):
        f.restype = sz
        f.argtypes = [DP, sz]
    lib.fastgrnn_hip_forward_windows_train.restype = i32
    lib.fastgrnn_hip_forward_windows_train.argtypes = [DP, PP, vp, sz, vp, vp, vp, vp, vp, sz, vp]
    lib.fastgrnn_hip_backward_windows.restype = i32
    lib.fastgrnn_hip_backward_windows.argtypes = [DP, PP, vp, vp, sz, vp, vp, vp, vp, GP, vp, sz, vp]
    if lib.fastgrnn_hip_abi_version() != ABI_VERSION:
        raise FastGRNNLibraryError("ABI version mismatch: library %d, binding %d"
                                   % (lib.fastgrnn_hip_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def status_string(code):
    return load().fastgrnn_hip_status_string(int(code)).decode()


def check(code, what):
    if code != 0:
        raise RuntimeError("%s failed: %s (fastgrnn_status %d)" % (what, status_string(code), code))
