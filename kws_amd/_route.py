"""How one call of an unrolled module reaches the operator shim, decided once per call signature: the layout ``x`` is
presented in, the forward's descriptor flags, what is saved for the backward, the form of the last-state gradient and
how the result is handed back.  ``FastGRNNCUDA``, ``FastGRNNUnrollFunction`` and the BatchNorm modules read the record;
none of them asks the library about kernel paths themselves.  Beside it: the small helpers those modules share."""
from __future__ import annotations

import collections
import functools

import torch

from . import _lib, fastgrnn_cuda

PLAIN, AFFINE = "plain", "affine"            # the cell of FastGRNNCUDA / the folded eval-mode BatchNorm cell
# Signature.mode: the grad mode of a module call, or APPLY: FastGRNNUnrollFunction called directly, whose
# ``batch_major`` argument (``batch_first`` here) is the caller's statement and is taken in place as given; None for
# the affine kind, which saves nothing in any mode
AUTOGRAD, NO_GRAD, INFERENCE, APPLY = "autograd", "no_grad", "inference_mode", "apply"
# Route.present: x goes to the shim as it is, after .contiguous(), as its [B,F,T] base permute(1,2,0) (FLAG_X_BFT), or
# -- batch_first not taken in place -- as the [T,B,F] copy transpose(0,1).contiguous()
AS_IS, CONTIGUOUS, BFT_BASE, TRANSPOSE_COPY = "as_is", "contiguous", "bft_base", "transpose_copy"
# Route.saved: the pre-activation (FLAG_SAVE_PREACT), the reference's (z_s, h_prime_s) pair, or None: an hs-only forward
PREACT, GATES = "preact", "gates"
# Route.post: hs as the kernel wrote it, transposed back to [B,T,H], its last step sliced off, or the [B,H] last state
# the kernel wrote alone (FLAG_HS_LAST)
TRANSPOSE_BACK, LAST_STEP, LAST_STATE = "transpose_back", "last_step", "last_state"

Signature = collections.namedtuple("Signature", "kind shape strides dtype is_cuda H w_rank u_rank gate update "
                                                "batch_first last_state mode")
# grad_last: the backward takes the [B,H] gradient under FLAG_GRAD_LAST (else it builds the dense one); dims: (T, B, F)
Route = collections.namedtuple("Route", "present flags saved grad_last post dims")


def seq_dims(shape, batch_major):
    """(T, B, F) of a ``[T,B,F]`` input, or of a ``[B,T,F]`` one."""
    a, b, F = shape
    return (b, a, F) if batch_major else (a, b, F)


def ranks(w1, u1):
    """(wRank, uRank) of a cell from its W1 / U1, whose leading sizes they are (empty: dense, 0)."""
    return w1.shape[0] if w1.numel() else 0, u1.shape[0] if u1.numel() else 0


def grad_mode():
    return AUTOGRAD if torch.is_grad_enabled() else INFERENCE if torch.is_inference_mode_enabled() else NO_GRAD


def _contiguous(shape, strides):
    expect = 1
    for n, s in zip(reversed(shape), reversed(strides)):
        if n != 1 and s != expect:
            return 0 in shape            # (an empty tensor is contiguous whatever its strides)
        expect *= n
    return True


def is_bft_view(shape, strides):
    """What the trainer hands over: permute(2,0,1) of the loader's [B,F,T] batch (trainClassifier.py:204,299), a
    [T,B,F] view whose base the kernels can take under FLAG_X_BFT."""
    return (len(shape) == 3 and not _contiguous(shape, strides)
            and _contiguous((shape[1], shape[2], shape[0]), (strides[1], strides[2], strides[0])))


_zero_states = {}        # (B, H, dtype, device) -> the default h0


def zero_state(B, H, dtype, device):
    """The default initial state.  It is read-only to every kernel and never handed out: one tensor per shape instead
    of a fill launch per call -- except under inference mode, whose tensors could not be saved for a backward later."""
    if torch.is_inference_mode_enabled():
        return torch.zeros([B, H], dtype=dtype, device=device)
    key = (B, H, dtype, device)
    h0 = _zero_states.get(key)
    if h0 is None:
        if len(_zero_states) >= 16:
            _zero_states.clear()
        h0 = _zero_states[key] = torch.zeros([B, H], dtype=dtype, device=device)
    return h0


def last_step(hs, flags):
    return hs[:, -1] if flags & _lib.FLAG_BATCH_MAJOR else hs[-1]


@functools.lru_cache(maxsize=1024)
def route(s):
    """The ``Route`` of the call signature ``s`` (a ``Signature``).  A pure function of it: the library's answers
    (``fastgrnn_cuda.kernel_path``) depend on the descriptor alone, which is why the device index is no part of the
    key -- two devices get one entry -- and why a bounded cache (the bound of ``fastgrnn_cuda._plan``) is all the
    state there is: an evicted signature is decided again."""
    SP, ZE, BM = _lib.FLAG_SAVE_PREACT, _lib.FLAG_ZERO_EXTEND, _lib.FLAG_BATCH_MAJOR
    XB, HL = _lib.FLAG_X_BFT, _lib.FLAG_HS_LAST
    shape, strides, last = s.shape, s.strides, s.last_state

    def path2(direction, flags):
        """kernel path 2 (the split-precision scans): a GPU tensor of a dtype they take and the library's answer"""
        return (s.is_cuda and s.dtype in (torch.float32, torch.bfloat16)
                and fastgrnn_cuda.kernel_path(T, B, F, s.H, s.w_rank, s.u_rank, s.gate, s.update, s.dtype, direction,
                                              flags) == 2)

    if s.kind == AFFINE:
        # the eval-mode BatchNorm forward (forward_unroll_affine adds FLAG_PREACT_AFFINE itself): nothing is saved
        bm = s.batch_first
        (B, T), F = (shape[:2] if bm else (shape[1], shape[0])), shape[-1]
        AF = _lib.FLAG_PREACT_AFFINE
        flags = HL if last else 0
        if bm:                   # in place where the kernels index [B,T,.], else transposed as the reference's BaseRNN does
            bm = path2(0, flags | BM | AF)
            flags |= BM if bm else 0
        if not s.batch_first and is_bft_view(shape, strides) and path2(0, flags | XB | AF):
            return Route(BFT_BASE, flags | XB, None, False, LAST_STATE if last else AS_IS, (T, B, F))
        present = TRANSPOSE_COPY if s.batch_first and not bm else AS_IS if _contiguous(shape, strides) else CONTIGUOUS
        if last and not path2(0, flags | AF):
            return Route(present, flags & ~HL, None, False, LAST_STEP, (T, B, F))   # (path 0 writes every state)
        post = LAST_STATE if last else TRANSPOSE_BACK if present == TRANSPOSE_COPY else AS_IS
        return Route(present, flags, None, False, post, (T, B, F))

    bm, copied = s.batch_first, False
    T, B, F = seq_dims(shape, bm)
    if bm and s.mode != APPLY and not path2(1, SP | BM | ZE):
        # batch_first: the reference transposes to [T,B,F] and back (rnn.py:812-813,823-825); only where the kernels
        # index [B,T,.] in place (FLAG_BATCH_MAJOR) is no copy made
        bm, copied = False, True
    dense = copied or _contiguous(shape, strides)
    bft = not bm and not dense and s.is_cuda and is_bft_view(shape, strides)
    present = TRANSPOSE_COPY if copied else AS_IS if dense else CONTIGUOUS
    back = TRANSPOSE_BACK if copied else AS_IS
    bmf = BM if bm else 0
    if s.mode in (NO_GRAD, INFERENCE):
        # nothing will be differentiated: hs alone (one [T,B,H] write instead of two), or h_T alone (FLAG_HS_LAST: hs
        # is not written at all), where the kernels have such a variant.  FLAG_X_BFT never goes beside
        # FLAG_ZERO_EXTEND: a [B,F,T] view on a zero-extended shape goes the autograd function's way and is copied
        if last:
            if bft and path2(0, HL | XB):
                return Route(BFT_BASE, HL | XB, None, False, LAST_STATE, (T, B, F))
            if path2(0, HL | ZE | bmf):
                return Route(present, HL | ZE | bmf, None, False, LAST_STATE, (T, B, F))
        elif (dense or bft) and path2(0, XB if bft else ZE | bmf):
            return Route(BFT_BASE if bft else present, XB if bft else ZE | bmf, None, False, back, (T, B, F))
    # the autograd function: on path 2 it keeps the pre-activation (FLAG_ZERO_EXTEND: hidden sizes up to 256 that no
    # path-2 shape covers run zero-padded to one), elsewhere the reference's pair under flags 0
    x_bft = bft and path2(1, SP | XB)
    preact = path2(1, SP | ZE)
    flags = (SP | ZE if preact else 0) | bmf | (XB if x_bft else 0)
    return Route(BFT_BASE if x_bft else present, flags, PREACT if preact else GATES,
                 bool(last and path2(1, flags | _lib.FLAG_GRAD_LAST)), LAST_STEP if last else back, (T, B, F))
