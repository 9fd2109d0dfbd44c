"""Drop-in for the reference's native operator module ``fastgrnn_cuda``
(/root/reference cuda/fastgrnn_cuda.cpp:235-240): the same four functions with the
same positional argument orders and return lists, backed by the C ABI of
``libfastgrnn_hip.so`` (include/fastgrnn_hip.h).

    forward(input, w, u, bias_gate, bias_update, zeta, nu, old_h, z_non_linearity,
            w1, w2, u1, u2)                                  -> [new_h, z, h_prime]
    backward(grad_h, input, old_h, zeta, nu, w, u, z, h_prime, w1, w2, u1, u2,
             z_non_linearity)                                -> 12 tensors
    forward_unroll(input, w, u, bias_gate, bias_update, zeta, nu, initial_h,
                   z_non_linearity, w1, w2, u1, u2)          -> [hs, z_s, h_prime_s]
    backward_unroll(grad_h, input, hidden_states, zeta, nu, w, u, z, h_prime,
                    initial_h, w1, w2, u1, u2, z_non_linearity) -> 12 tensors

(fastgrnn_cuda.cpp:73-232).  The 12-tuple order is
``d_input, d_bias_z, d_bias_h_prime, d_zeta, d_nu, d_old_h, d_w, d_u, d_w1, d_w2,
d_u1, d_u2`` (.cu:317,556); operands that do not apply are ``torch.empty(0)`` on both
sides of the call (rnn.py:783-798, .cu:221-224).

This shim only checks arguments the way ``CHECK_INPUT`` does
(fastgrnn_cuda.cpp:69-71 -> RuntimeError), allocates outputs + workspace with torch,
and launches on torch's CURRENT stream of the input's device.  All arithmetic is in
the HIP kernels; there is no eager fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import torch

from . import _lib

_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.bfloat16: _lib.BF16_IO}


def _param_dtype(io_dtype):
    """bf16 sequences (x, hs, grad_hs, d_x) go with fp32 parameters, h0 and gradients."""
    return torch.float32 if io_dtype == torch.bfloat16 else io_dtype

# Optional per-launch timing (bench.py): when set to a list, every C-ABI call appends
# (tag, start_event, end_event) recorded on the stream the kernels are launched on.
_timing = None


class _Timed:
    def __init__(self, tag, device):
        self.tag, self.device = tag, device

    def __enter__(self):
        self.on = _timing is not None and self.tag is not None     # (tag None: a call that records no sample)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.device))

    def __exit__(self, *exc):
        if self.on:
            self.e1.record(torch.cuda.current_stream(self.device))
            _timing.append((self.tag, self.e0, self.e1))
        return False


def _check_input(t, name):
    # CHECK_CUDA / CHECK_CONTIGUOUS, fastgrnn_cuda.cpp:69-71
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _present(t):
    # reference: low-rank is detected by w1.size(0) != 0 (.cu:138-139)
    return t is not None and t.numel() != 0


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if _present(t) else C.c_void_p(None)


def _expect(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


def _describe(T, B, F, H, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu, dtype, gate_nl,
              update_nl, flags):
    """Validate parameters against (F,H) and build the C descriptor + params struct."""
    if dtype not in _DTYPES:
        raise RuntimeError("fastgrnn: unsupported dtype %s (float32/float64, or bfloat16 sequences)" % dtype)
    io_dtype, dtype = dtype, _param_dtype(dtype)
    w_lr, u_lr = _present(w1), _present(u1)
    if w_lr:
        _check_input(w1, "w1"); _check_input(w2, "w2")
        rw = w1.shape[0]
        _expect(w1, (rw, F), "w1"); _expect(w2, (H, rw), "w2")
    else:
        _check_input(w, "w")
        rw = 0
        _expect(w, (H, F), "w")
    if u_lr:
        _check_input(u1, "u1"); _check_input(u2, "u2")
        ru = u1.shape[0]
        _expect(u1, (ru, H), "u1"); _expect(u2, (H, ru), "u2")
    else:
        _check_input(u, "u")
        ru = 0
        _expect(u, (H, H), "u")
    for t, n in ((zeta, "zeta"), (nu, "nu")):
        _check_input(t, n)
        if t.numel() != 1:
            raise RuntimeError("%s must hold one element" % n)
    tensors = [t for t in (w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu) if _present(t)]
    for t in tensors:
        if t.dtype != dtype:
            raise RuntimeError("fastgrnn: all operands must share dtype %s (got %s)" % (dtype, t.dtype))
    plan = _plan(T, B, F, H, rw, ru, int(gate_nl), int(update_nl), _DTYPES[io_dtype], int(flags))
    return plan, _params(w_lr, u_lr, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu), w_lr, u_lr


def _params(w_lr, u_lr, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu):
    """The C params struct: dense matrices or their factors, whichever the cell has."""
    return _lib.Params(_ptr(None if w_lr else w), _ptr(None if u_lr else u),
                       _ptr(w1 if w_lr else None), _ptr(w2 if w_lr else None),
                       _ptr(u1 if u_lr else None), _ptr(u2 if u_lr else None),
                       _ptr(bias_gate), _ptr(bias_update), _ptr(zeta), _ptr(nu))


def _seq_dims(input, flags):
    """(T, B, F) of an unrolled call's input under the layout flags."""
    if flags & _lib.FLAG_X_BFT:              # the trainer's [B,F,T] (trainClassifier.py:204)
        B, F, T = input.shape
    elif flags & _lib.FLAG_BATCH_MAJOR:
        B, T, F = input.shape
    else:
        T, B, F = input.shape
    return T, B, F


def _seq_shape(T, B, H, batch_major, last):
    """The shape of an unrolled call's hidden states: every state in the input's layout, or the last one alone."""
    return (B, H) if last else (B, T, H) if batch_major else (T, B, H)


def _desc(T, B, F, H, rw, ru, gate_nl, update_nl, dtype_code, flags):
    """The C descriptor (the one place it is built); its arguments are the key of every per-descriptor cache."""
    return _lib.Desc(T, B, F, H, rw, ru, int(gate_nl), int(update_nl), dtype_code, int(flags))


def _key(d):
    return d.T, d.B, d.F, d.H, d.w_rank, d.u_rank, d.gate_nl, d.update_nl, d.dtype, d.flags


# Scratch workspace, kept per (device, stream) and grown on demand: its contents never outlive a call and every use
# is stream-ordered, so consecutive calls on one stream can share it (a fresh torch.empty per call was a few
# microseconds of host time per step; the 8-GPU step adds the collective's latency on top of whatever the host spends)
_ws_cache = {}

_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or \
    (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _call(fn, what, tag, dev, nbytes, *args):
    """The launch path of every C-ABI call: ``fn(*args, workspace, nbytes, stream)`` on torch's current stream of
    ``dev`` (``nbytes=None``: ``fn(*args, stream)``, a call without a workspace), timed under ``tag`` (``_timing``) and
    its status checked as ``what``.  Callers allocate their outputs under ``torch.cuda.device(dev)`` around it."""
    idx = dev.index
    # (the raw-stream query is one C call; building a torch.cuda.Stream object for it cost ~5 us per operator call)
    stream = _get_raw_stream(torch.cuda.current_device() if idx is None else idx)
    if nbytes is not None:
        ws = _ws_cache.get((idx, stream)) if nbytes else None
        if nbytes and (ws is None or ws.numel() < nbytes):
            ws = _ws_cache[idx, stream] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        # (ws stays referenced until fn has enqueued; reuse by the next call is stream-ordered behind these launches)
        args += (ws.data_ptr() if nbytes else None, nbytes)
    with _Timed(tag, dev):
        st = fn(*args, stream)
    _lib.check(st, what)


# What the library decides from a descriptor alone (include/fastgrnn_hip.h, fastgrnn_plan): the kernel family and the
# workspace size per direction, what the route lets the caller leave out, and the FLAG_ZERO_EXTEND plan
_Plan = collections.namedtuple("_Plan", "desc path ws forward_ws_optional dx_optional rank_space_cols zext")


@functools.lru_cache(maxsize=1024)
def _plan(T, B, F, H, rw, ru, gate_nl, update_nl, dtype_code, flags):
    """Everything about a descriptor that does not depend on the tensors: the C struct itself and the library's plan
    for it (a pure function of the descriptor in the C ABI, one call).  One dictionary lookup per operator call
    instead of a ctypes round trip.  ``zext`` is the ``_lib.ZextPlan``: all zero where FLAG_ZERO_EXTEND does not take
    the padded route."""
    desc = _desc(T, B, F, H, rw, ru, gate_nl, update_nl, dtype_code, flags)
    out = _lib.Plan()
    st = _lib.load().fastgrnn_hip_plan(C.byref(desc), C.byref(out))
    if flags & _lib.FLAG_ZERO_EXTEND:
        _lib.check(st, "fastgrnn zero_extend_plan")
    # (any other descriptor error is the operator call's to report; the path query answers -1 for it)
    return _Plan(desc, (-1, -1) if st else tuple(out.path), tuple(int(n) for n in out.workspace_bytes),
                 bool(out.forward_ws_optional), bool(out.dx_optional), int(out.rank_space_cols), out.zext)


_cliff_warned = set()


def _warn_fallback(plan, direction):
    """Perf cliffs are not silent: the first call of a shape that lands on the generic scan (kernel path 0) at a size
    where that matters says so once (include/fastgrnn_hip.h lists what runs on the matrix pipe)."""
    d = plan.desc
    if plan.path[direction] != 0 or d.T * d.B < 4096 or (d.flags & _lib.FLAG_FORCE_GENERIC):
        return
    key = _key(d) + (direction,)
    if key in _cliff_warned:
        return
    _cliff_warned.add(key)
    import warnings
    warnings.warn("fastgrnn: %s of shape T=%d B=%d F=%d H=%d ranks=(%d,%d) dtype=%d flags=0x%x runs on the generic "
                  "scan (kernel path 0), typically 20-30x slower than the matrix-pipe kernels; see "
                  "include/fastgrnn_hip.h (fastgrnn_hip_kernel_path) for the shapes those cover"
                  % ("backward" if direction else "forward", d.T, d.B, d.F, d.H, d.w_rank, d.u_rank, d.dtype, d.flags),
                  RuntimeWarning, stacklevel=4)


def kernel_path(T, B, F, H, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=torch.float32,
                direction=0, flags=0):
    """0 = generic scan, 1 = fp32-MFMA scan, 2 = split-precision scan (pure function of the descriptor; cached)."""
    return _plan(T, B, F, H, w_rank, u_rank, int(gate_nl), int(update_nl), _DTYPES[dtype], int(flags)).path[int(direction)]


def zero_extend_plan(T, B, F, H, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=torch.float32, flags=0):
    """What FLAG_ZERO_EXTEND does for a descriptor (include/fastgrnn_hip.h, fastgrnn_hip_zero_extend_plan): a dict with
    ``forward`` / ``backward`` (the padded route is taken), ``Hp``, ``Fp``, ``dx_optional`` and ``saved_bytes`` (the
    opaque z_s buffer under FLAG_SAVE_PREACT).  All zero where the route does not apply."""
    zx = _plan(T, B, F, H, w_rank, u_rank, int(gate_nl), int(update_nl), _DTYPES[dtype],
               int(flags) | _lib.FLAG_ZERO_EXTEND).zext
    names = ("forward", "backward", "Hp", "Fp", "dx_optional", "saved_bytes")
    return {n: int(getattr(zx, n)) for n in names}


# Signatures (shapes, dtypes, flags of one call) that have passed the full argument checks once.  A training loop makes
# the same call thousands of times: after the first one only what can change from call to call without changing the
# signature is re-checked (device, contiguity), and the checks that are pure functions of the signature are skipped --
# half of the host time of a step (tools/host_overhead.py: the host's enqueue time is within reach of the GPU's).
_seen = {}
_SEEN_MAX = 1024                 # (the bound of _plan: a loader with variable T or a ragged last batch keeps adding)
_use_seen = True                 # (tools/host_overhead.py switches it off for its A/B)


def _remember(sig, ent):
    if len(_seen) >= _SEEN_MAX:  # (cleared when full, as the default states of _route are)
        _seen.clear()
    _seen[sig] = ent


def _all_dense_on(dev, *ts):
    """What the validated-signature path re-checks: every non-empty operand is contiguous on the input's device."""
    for t in ts:
        if t.numel() and not (t.device == dev and t.is_contiguous()):
            return False
    return True


def _check_devices(dev, named, meta_ok=False):
    """Every present operand is on the input's device: its pointer is launched there."""
    for t, n in named:
        if _present(t) and t.device != dev and not (meta_ok and t.device.type == "meta"):
            raise RuntimeError("%s is on %s, but input is on %s" % (n, t.device, dev))


def _launch_forward(lib, plan, ent, unrolled, preact, want_gates, input, h0, params):
    """Allocate the outputs and launch (the counterpart of _launch_backward)."""
    oshape, hshape, rank_space_shape, nbytes, zsaved = ent
    dev = input.device
    pdt = h0.dtype
    with torch.cuda.device(dev):
        hs = torch.empty(hshape, dtype=input.dtype, device=dev)
        if zsaved:
            zs = torch.empty(zsaved, dtype=torch.uint8, device=dev)
        else:
            zs = torch.empty(oshape, dtype=pdt, device=dev) if (want_gates or preact) else None
        cs = torch.empty(oshape, dtype=pdt, device=dev) if (want_gates and not preact) else None
        if rank_space_shape:
            cs = torch.empty(rank_space_shape, dtype=pdt, device=dev)
        _call(lib.fastgrnn_hip_forward_unroll if unrolled else lib.fastgrnn_hip_forward,
              "fastgrnn forward_unroll" if unrolled else "fastgrnn forward", "forward", dev, nbytes,
              C.byref(plan.desc), C.byref(params), _ptr(input), _ptr(h0), _ptr(hs), _ptr(zs), _ptr(cs))
    if preact:                  # zs holds the pre-activation W.x + U.h
        return [hs, zs] if cs is None else [hs, zs, cs]
    return [hs, zs, cs] if want_gates else [hs]


def _forward_impl(input, w, u, bias_gate, bias_update, zeta, nu, h0, gate_nl, w1, w2, u1, u2,
                  unrolled, update_nl, want_gates, flags):
    lib = _lib.load()
    preact = bool(flags & _lib.FLAG_SAVE_PREACT)
    sig = ("f", unrolled, input.shape, input.dtype, h0.shape, h0.dtype, w.shape, u.shape, w1.shape, w2.shape,
           u1.shape, u2.shape, bias_gate.shape, bias_update.shape, zeta.shape, nu.shape,
           (w if w.numel() else w1).dtype, (u if u.numel() else u1).dtype, bias_gate.dtype, bias_update.dtype,
           zeta.dtype, nu.dtype, gate_nl, update_nl, flags, want_gates, input.device.index)
    ent = _seen.get(sig) if _use_seen else None
    if ent is not None and _all_dense_on(input.device, input, h0, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta,
                                         nu):
        plan, w_lr, u_lr, tail = ent
        return _launch_forward(lib, plan, tail, unrolled, preact, want_gates, input, h0,
                               _params(w_lr, u_lr, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu))
    _check_input(input, "input")
    _check_input(bias_gate, "bias_gate"); _check_input(bias_update, "bias_update")
    _check_input(h0, "initial_h" if unrolled else "old_h")
    if unrolled:
        if input.dim() != 3:
            raise RuntimeError("input must be [timesteps, batch, features]")
        T, B, F = _seq_dims(input, flags)
    else:
        if input.dim() != 2:
            raise RuntimeError("input must be [batch, features]")
        T = 1
        B, F = input.shape
    H = h0.shape[-1]
    _expect(h0, (B, H), "initial_h" if unrolled else "old_h")
    if bias_gate.numel() != H or bias_update.numel() != H:
        raise RuntimeError("bias_gate/bias_update must hold H=%d elements" % H)
    pdt = _param_dtype(input.dtype)
    if h0.dtype != pdt:
        raise RuntimeError("input and hidden state dtypes differ" if pdt == input.dtype
                           else "bfloat16 sequences take a float32 hidden state")
    plan, params, w_lr, u_lr = _describe(T, B, F, H, w, u, w1, w2, u1, u2, bias_gate, bias_update, zeta, nu,
                                         input.dtype, gate_nl, update_nl, flags)
    _check_devices(input.device, ((h0, "initial_h" if unrolled else "old_h"), (w, "w"), (u, "u"), (w1, "w1"),
                                  (w2, "w2"), (u1, "u1"), (u2, "u2"), (bias_gate, "bias_gate"),
                                  (bias_update, "bias_update"), (zeta, "zeta"), (nu, "nu")))
    _warn_fallback(plan, 0)
    oshape = _seq_shape(T, B, H, flags & _lib.FLAG_BATCH_MAJOR, not unrolled)
    hs_last = bool(unrolled and (flags & _lib.FLAG_HS_LAST))
    if hs_last and (want_gates or preact):
        raise RuntimeError("FLAG_HS_LAST is an inference mode: nothing can be saved for a backward "
                           "(want_gates=False and no FLAG_SAVE_PREACT)")
    # FLAG_ZERO_EXTEND on the padded route: under FLAG_SAVE_PREACT the saved tensor is one opaque buffer
    # (fastgrnn_hip.h: the padded pre-activation, the padded hidden states and, for the low-rank scans, the
    # rank-space vector) that the backward takes back as z
    zroute = bool(plan.zext.forward) and (preact or not want_gates)
    zsaved = int(plan.zext.saved_bytes) if (zroute and preact) else 0
    # factorised operands on the low-rank scans: the forward also saves the rank-space vector [U1.h | W1.x] per step,
    # always time-major and zero-extended to 16 + 16 columns (an opaque tensor for the backward)
    rank_space_shape = (T * B, plan.rank_space_cols) if plan.rank_space_cols else None
    # (layers that park the frame product in the auxiliary outputs need no workspace when those are requested:
    # include/fastgrnn_hip.h, forward workspace)
    nbytes = 0 if (plan.forward_ws_optional and (want_gates or preact)) else plan.ws[0]
    tail = (oshape, (B, H) if hs_last else oshape, rank_space_shape, nbytes, zsaved)
    _remember(sig, (plan, w_lr, u_lr, tail))
    return _launch_forward(lib, plan, tail, unrolled, preact, want_gates, input, h0, params)


def _launch_backward(lib, plan, ent, unrolled, preact, grad_h, input, hs_or_old_h, z, h_prime, rank_space, h0,
                     w, u, w1, w2, u1, u2, b0, b1, zeta, nu, need_dx):
    """Allocate the 12 outputs (the parameter gradients through ``_flat_grads``) and launch."""
    w_lr, u_lr, shapes, sizes, dx_optional, B, H = ent
    desc = plan.desc
    dev = input.device
    dt = input.dtype
    pdt = h0.dtype
    params = _params(w_lr, u_lr, w, u, w1, w2, u1, u2, b0, b1, zeta, nu)
    with torch.cuda.device(dev):
        # the input's gradient is optional on these shapes (fastgrnn_hip.h, fastgrnn_grads.d_x): skipped when autograd
        # does not ask for it (a model's first layer)
        d_input = _NONE if (dx_optional and not need_dx) else torch.empty(input.shape, dtype=dt, device=dev)
        d_old_h = torch.empty((B, H), dtype=pdt, device=dev)
        views, slots = _flat_grads(w_lr, u_lr, shapes, sizes, pdt, dev)
        out = [d_input, *views[-4:], d_old_h, *slots]        # (the 12-tuple is in the order of the C grads struct)
        grads = _lib.Grads(*map(_ptr, out))
        if unrolled:
            _call(lib.fastgrnn_hip_backward_unroll, "fastgrnn backward_unroll", "backward", dev, plan.ws[1],
                  C.byref(desc), C.byref(params), _ptr(grad_h), _ptr(input), _ptr(hs_or_old_h), _ptr(z),
                  _ptr(rank_space if preact else h_prime), _ptr(h0), C.byref(grads))
        else:
            _call(lib.fastgrnn_hip_backward, "fastgrnn backward", "backward", dev, plan.ws[1], C.byref(desc),
                  C.byref(params), _ptr(grad_h), _ptr(input), _ptr(h0), _ptr(z), _ptr(h_prime), C.byref(grads))
    return out


_NONE = torch.empty(0)           # the reference's placeholder for operands / gradients that do not apply


def _flat_grads(w_lr, u_lr, shapes, sizes, dtype, device):
    """The parameter gradients as views of ONE flat buffer, laid out in the order the modules register their
    parameters (W | W1,W2 ; U | U1,U2 ; bias_gate ; bias_update ; zeta ; nu).  autograd adopts them as the .grad
    tensors, so a data-parallel step can all-reduce that buffer in place (kws_amd.dp.GradBucket) instead of packing
    and unpacking six tensors.  Returns (the views in that order, the ``d_w, d_u, d_w1, d_w2, d_u1, d_u2`` slots of
    the 12-tuple with ``_NONE`` where the cell has no such operand)."""
    views = [v.view(sh) for v, sh in zip(torch.empty(sum(sizes), dtype=dtype, device=device).split(sizes), shapes)]
    nw = 2 if w_lr else 1
    d_w, d_w1, d_w2 = (_NONE, views[0], views[1]) if w_lr else (views[0], _NONE, _NONE)
    d_u, d_u1, d_u2 = (_NONE, views[nw], views[nw + 1]) if u_lr else (views[nw], _NONE, _NONE)
    return views, (d_w, d_u, d_w1, d_w2, d_u1, d_u2)


def _backward_impl(grad_h, input, hs_or_old_h, zeta, nu, w, u, z, h_prime, h0, w1, w2, u1, u2, gate_nl,
                   unrolled, update_nl, flags, bias_gate=None, bias_update=None, need_dx=True):
    lib = _lib.load()
    preact = bool(flags & _lib.FLAG_SAVE_PREACT)
    if unrolled and not need_dx:
        # FLAG_NO_INPUT_GRAD lets dense H=128/F=32 skip d_x as well (a scan without the d_x product; elsewhere the flag
        # changes nothing).  Part of the descriptor, hence of the cached plan and of the signature below: calls with and
        # without the input's gradient never share an entry.
        flags |= _lib.FLAG_NO_INPUT_GRAD
    sig = ("b", unrolled, grad_h.shape, grad_h.dtype, input.shape, input.dtype, hs_or_old_h.shape, hs_or_old_h.dtype,
           z.shape, z.dtype, h_prime.shape, h_prime.dtype, h0.shape, h0.dtype, w.shape, u.shape, w1.shape, w2.shape,
           u1.shape, u2.shape, (w if w.numel() else w1).dtype, (u if u.numel() else u1).dtype, zeta.shape, nu.shape,
           zeta.dtype, nu.dtype, None if bias_gate is None else (bias_gate.shape, bias_gate.dtype),
           None if bias_update is None else (bias_update.shape, bias_update.dtype),
           gate_nl, update_nl, flags, input.device.index)
    ent = _seen.get(sig) if _use_seen else None
    dev = input.device
    if ent is not None and _all_dense_on(dev, grad_h, input, hs_or_old_h, z, h_prime, h0, w, u, w1, w2, u1, u2, zeta,
                                         nu) and (not preact or _all_dense_on(dev, bias_gate, bias_update)):
        plan, rs, tail = ent
        return _launch_backward(lib, plan, tail, unrolled, preact, grad_h, input, hs_or_old_h, z,
                                z if preact else h_prime, h_prime if rs else None, h0, w, u, w1, w2, u1, u2,
                                bias_gate if preact else zeta, bias_update if preact else zeta, zeta, nu, need_dx)
    # FLAG_ZERO_EXTEND's padded route: z is the forward's opaque saved buffer (uint8), h_prime is not used
    zsaved = preact and bool(flags & _lib.FLAG_ZERO_EXTEND) and z.dtype == torch.uint8
    rank_space = None
    if preact:
        if bias_gate is None or bias_update is None:
            raise RuntimeError("FLAG_SAVE_PREACT backward needs bias_gate and bias_update")
        rank_space, h_prime = h_prime, z         # (h_prime = z keeps the shape checks below uniform)
    for t, n in ((grad_h, "grad_h"), (input, "input"), (hs_or_old_h, "hidden_states" if unrolled else "old_h"),
                 (z, "z"), (h_prime, "h_prime"), (h0, "initial_h")):
        if not (preact and t.device.type == "meta"):
            _check_input(t, n)
    if unrolled:
        T, B, F = _seq_dims(input, flags)
        H = grad_h.shape[-1]
        lead = (B, T) if flags & _lib.FLAG_BATCH_MAJOR else (T, B)
        # FLAG_GRAD_LAST: the gradient of the last state only (the classifier head's view, model.py:227)
        _expect(grad_h, (B, H) if flags & _lib.FLAG_GRAD_LAST else lead + (H,), "grad_h")
        _expect(hs_or_old_h, lead + (H,), "hidden_states")
        if not zsaved:
            _expect(z, lead + (H,), "z"); _expect(h_prime, lead + (H,), "h_prime")
        _expect(h0, (B, H), "initial_h")
    else:
        T = 1
        B, F = input.shape
        H = grad_h.shape[-1]
        _expect(grad_h, (B, H), "grad_h"); _expect(h0, (B, H), "old_h")
        _expect(z, (B, H), "z"); _expect(h_prime, (B, H), "h_prime")
    dt = input.dtype
    pdt = _param_dtype(dt)
    for t, want in ((grad_h, dt), (hs_or_old_h, dt if unrolled else pdt), (z, torch.uint8 if zsaved else pdt),
                    (h_prime, torch.uint8 if zsaved else pdt), (h0, pdt)):
        if t.dtype != want:
            raise RuntimeError("fastgrnn backward: operand dtypes differ")
    # biases are not needed by the backward when z, h_prime are given: pass zeta as a dummy
    plan, params, w_lr, u_lr = _describe(T, B, F, H, w, u, w1, w2, u1, u2,
                                         bias_gate if preact else zeta, bias_update if preact else zeta,
                                         zeta, nu, dt, gate_nl, update_nl, flags)
    _check_devices(dev, ((grad_h, "grad_h"), (hs_or_old_h, "hidden_states" if unrolled else "old_h"), (z, "z"),
                         (h_prime, "h_prime"), (rank_space, "rank_space"), (h0, "initial_h"), (w, "w"), (u, "u"),
                         (w1, "w1"), (w2, "w2"), (u1, "u1"), (u2, "u2"), (zeta, "zeta"), (nu, "nu"))
                   + (((bias_gate, "bias_gate"), (bias_update, "bias_update")) if preact else ()), meta_ok=preact)
    zx = plan.zext
    if zsaved and not (zx.backward and z.numel() == zx.saved_bytes):
        raise RuntimeError("fastgrnn backward: z is not the saved buffer of a FLAG_ZERO_EXTEND forward of this shape")
    if preact and not zsaved and zx.backward:
        raise RuntimeError("fastgrnn backward: FLAG_ZERO_EXTEND takes the saved buffer of its forward as z (uint8)")
    # (the low-rank scans save a rank-space vector that comes back as h_prime; every other FLAG_SAVE_PREACT cell saves
    # the pre-activation alone and h_prime is not used)
    if plan.rank_space_cols:
        _check_input(rank_space, "rank_space")
        _expect(rank_space, (T * B, plan.rank_space_cols), "rank_space")
    else:
        rank_space = None
    _warn_fallback(plan, 1)
    shapes = ([tuple(w1.shape), tuple(w2.shape)] if w_lr else [(H, F)]) + \
             ([tuple(u1.shape), tuple(u2.shape)] if u_lr else [(H, H)]) + [(1, H), (1, H), (1, 1), (1, 1)]
    sizes = [a * b for a, b in shapes]
    ent = (w_lr, u_lr, shapes, sizes, plan.dx_optional, B, H)
    _remember(sig, (plan, rank_space is not None, ent))
    return _launch_backward(lib, plan, ent, unrolled, preact, grad_h, input, hs_or_old_h, z, h_prime,
                            rank_space, h0, w, u, w1, w2, u1, u2,
                            bias_gate if preact else zeta, bias_update if preact else zeta, zeta, nu, need_dx)


def frame_gemm(x, w):
    """P[rows, H] = X[rows, F] . W^T (W:[H,F]): the batched frame product a wide-input layer's forward runs in front of
    its scan (include/fastgrnn_hip.h, fastgrnn_hip_frame_gemm), as a call of its own -- for measuring it."""
    _check_input(x, "x"); _check_input(w, "w")
    rows, F = x.shape
    H = w.shape[0]
    _expect(w, (H, F), "w")
    p = torch.empty((rows, H), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _call(_lib.load().fastgrnn_hip_frame_gemm, "fastgrnn frame_gemm", "frame_gemm", x.device, None,
              rows, H, F, _ptr(x), _ptr(w), _ptr(p), _DTYPES[x.dtype])
    return p


# ---- the four reference entry points (fastgrnn_cuda.cpp:235-240) -------------------------

def forward(input, w, u, bias_gate, bias_update, zeta, nu, old_h, z_non_linearity, w1, w2, u1, u2,
            *, update_non_linearity=2, flags=0):
    """fastgrnn_cuda.cpp:73-107 -> [new_h, z, h_prime]."""
    return _forward_impl(input, w, u, bias_gate, bias_update, zeta, nu, old_h, z_non_linearity,
                         w1, w2, u1, u2, False, update_non_linearity, True, flags)


def backward(grad_h, input, old_h, zeta, nu, w, u, z, h_prime, w1, w2, u1, u2, z_non_linearity,
             *, update_non_linearity=2, flags=0):
    """fastgrnn_cuda.cpp:109-145 -> 12 tensors (.cu:317)."""
    return _backward_impl(grad_h, input, old_h, zeta, nu, w, u, z, h_prime, old_h, w1, w2, u1, u2,
                          z_non_linearity, False, update_non_linearity, flags)


def forward_unroll(input, w, u, bias_gate, bias_update, zeta, nu, initial_h, z_non_linearity,
                   w1, w2, u1, u2, *, update_non_linearity=2, want_gates=True, flags=0):
    """fastgrnn_cuda.cpp:147-180 -> [hidden_states, z_s, h_prime_s] (each [T,B,H]).
    ``want_gates=False`` (extension) returns ``[hidden_states]`` only and skips the two
    extra [T,B,H] stores -- forward-only / inference use."""
    return _forward_impl(input, w, u, bias_gate, bias_update, zeta, nu, initial_h, z_non_linearity,
                         w1, w2, u1, u2, True, update_non_linearity, want_gates, flags)


def forward_unroll_affine(input, w, u, bias_gate, bias_update, zeta, nu, gate_scale, update_scale, initial_h,
                          z_non_linearity, update_non_linearity=2, flags=0):
    """Inference forward of the cell with per-unit pre-activation scales (include/fastgrnn_hip.h,
    ``fastgrnn_hip_forward_unroll_affine``): ``z = gate(gate_scale*pre + bias_gate)``, ``h' = update(update_scale*pre
    + bias_update)``, ``pre = w.x + u.h`` -- an eval-mode BatchNorm cell after folding.  Dense operands in the
    ``[out,in]`` layout, fp32 or fp64.  Returns hs (``[T,B,H]``, ``[B,T,H]`` under FLAG_BATCH_MAJOR, ``[B,H]`` under
    FLAG_HS_LAST).  With FLAG_X_BFT ``input`` is the data loader's ``[B,F,T]`` batch (layers whose frame product is a
    GEMM of its own: F = 64 / 128 / 256 on kernel path 2).  Nothing is saved for a backward."""
    lib = _lib.load()
    flags = int(flags) | _lib.FLAG_PREACT_AFFINE
    for t, n in ((input, "input"), (initial_h, "initial_h"), (bias_gate, "bias_gate"), (bias_update, "bias_update"),
                 (gate_scale, "gate_scale"), (update_scale, "update_scale")):
        _check_input(t, n)
    if input.dim() != 3:
        raise RuntimeError("input must be [timesteps, batch, features]")
    T, B, F = _seq_dims(input, flags)
    H = initial_h.shape[-1]
    _expect(initial_h, (B, H), "initial_h")
    for t, n in ((bias_gate, "bias_gate"), (bias_update, "bias_update"), (gate_scale, "gate_scale"),
                 (update_scale, "update_scale")):
        if t.numel() != H:
            raise RuntimeError("%s must hold H=%d elements" % (n, H))
    if input.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("fastgrnn: the affine forward takes float32 or float64 sequences (got %s)" % input.dtype)
    for t in (initial_h, gate_scale, update_scale):
        if t.dtype != input.dtype:
            raise RuntimeError("fastgrnn: all operands must share dtype %s (got %s)" % (input.dtype, t.dtype))
    plan, params, _, _ = _describe(T, B, F, H, w, u, None, None, None, None, bias_gate, bias_update, zeta, nu,
                                   input.dtype, z_non_linearity, update_non_linearity, flags)
    _warn_fallback(plan, 0)
    dev = input.device
    with torch.cuda.device(dev):
        hs = torch.empty(_seq_shape(T, B, H, flags & _lib.FLAG_BATCH_MAJOR, flags & _lib.FLAG_HS_LAST),
                         dtype=input.dtype, device=dev)
        _call(lib.fastgrnn_hip_forward_unroll_affine, "fastgrnn forward_unroll_affine", "forward_affine", dev,
              plan.ws[0], C.byref(plan.desc), C.byref(params), _ptr(gate_scale), _ptr(update_scale), _ptr(input),
              _ptr(initial_h), _ptr(hs))
    return hs


# What the library answers for a descriptor in one family of calls that goes beyond ``_plan``: whether the family holds
# it, and the workspace of its forward and its backward (0 where there is none, or where the family does not hold it)
_PoolPlan = collections.namedtuple("_PoolPlan", "desc supported ws_forward ws_backward")

# family -> the C ABI's queries (supported, forward workspace, backward workspace)
_FAMILIES = {
    "windows": ("fastgrnn_hip_windows_supported", "fastgrnn_hip_forward_windows_workspace_bytes", None),
    "train_windows": ("fastgrnn_hip_train_windows_supported", "fastgrnn_hip_train_windows_forward_workspace_bytes",
                      "fastgrnn_hip_train_windows_backward_workspace_bytes"),
    "bn_train": ("fastgrnn_hip_bn_train_supported", "fastgrnn_hip_bn_train_forward_workspace_bytes",
                 "fastgrnn_hip_bn_train_backward_workspace_bytes"),
}


@functools.lru_cache(maxsize=1024)
def _pool_plan(key, family, rows=None):
    """The ``_PoolPlan`` of the descriptor ``_desc(*key)`` in a family of ``_FAMILIES``, for a pool of ``rows`` frames
    (None: the family's workspace queries take the descriptor alone).  Pure functions of the descriptor in the C ABI,
    asked once per signature like ``_plan``."""
    desc = _desc(*key)
    lib = _lib.load()
    supported, *sizes = (q and getattr(lib, q) for q in _FAMILIES[family])
    if not supported(C.byref(desc)):
        return _PoolPlan(desc, False, 0, 0)
    rest = () if rows is None else (rows,)
    return _PoolPlan(desc, True, *(int(q(C.byref(desc), *rest)) if q else 0 for q in sizes))


def windows_supported(T, B, F, H, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=torch.float32, flags=0):
    """``forward_windows`` runs this descriptor on the windowed scans (include/fastgrnn_hip.h,
    ``fastgrnn_hip_windows_supported``); where it does not, the modules gather the windows and call the existing
    forward.  ``flags``: FLAG_BATCH_MAJOR / FLAG_HS_LAST / FLAG_PREACT_AFFINE."""
    if dtype not in _DTYPES:
        return False
    return _pool_plan((T, B, F, H, w_rank, u_rank, int(gate_nl), int(update_nl), _DTYPES[dtype], int(flags)),
                      "windows", T).supported


def forward_windows(pool, starts, T, w, u, bias_gate, bias_update, zeta, nu, initial_h, z_non_linearity,
                    gate_scale=None, update_scale=None, batch_major=False, last_state=False, *,
                    update_non_linearity=2, check=True):
    """Inference forward over windows of a shared frame pool (include/fastgrnn_hip.h, ``fastgrnn_hip_forward_windows``):
    utterance ``b`` is the ``T`` consecutive rows of ``pool:[R,F]`` from row ``starts[b]`` on, read in place -- no
    gathered ``[T,B,F]`` copy.  ``starts``: ``[B]`` int32 or int64 on the pool's device, ``0 <= starts[b] <= R - T``;
    overlapping, repeated and unordered starts are fine.  ``check=True`` validates that range with one ``aminmax``
    (one host synchronisation) and raises ``ValueError``; ``check=False`` skips it and makes the range the caller's
    obligation.  ``gate_scale`` / ``update_scale``: both given for the eval-mode BatchNorm arithmetic of
    ``forward_unroll_affine``, both None for the plain cell.  Returns hs: ``[T,B,H]``, ``[B,T,H]`` with
    ``batch_major`` or ``[B,H]`` (h_T) with ``last_state``.  Nothing is saved for a backward.  Cells the windowed scans
    do not hold (``windows_supported``) raise: there is no eager fallback here."""
    lib = _lib.load()
    affine = gate_scale is not None or update_scale is not None
    if affine and (gate_scale is None or update_scale is None):
        raise RuntimeError("forward_windows: gate_scale and update_scale go together")
    scales = ((gate_scale, "gate_scale"), (update_scale, "update_scale")) if affine else ()
    R, F, B, T, H, starts = _windows_operands(pool, starts, T, initial_h, bias_gate, bias_update, check, scales)
    flags = (_lib.FLAG_BATCH_MAJOR if batch_major else 0) | (_lib.FLAG_HS_LAST if last_state else 0) | \
        (_lib.FLAG_PREACT_AFFINE if affine else 0)
    plan, params, w_lr, u_lr = _describe(T, B, F, H, w, u, None, None, None, None, bias_gate, bias_update, zeta, nu,
                                         pool.dtype, z_non_linearity, update_non_linearity, flags)
    d = plan.desc
    dev = pool.device
    with torch.cuda.device(dev):
        hs = torch.empty(_seq_shape(T, B, H, batch_major, last_state), dtype=pool.dtype, device=dev)
        _call(lib.fastgrnn_hip_forward_windows, "fastgrnn forward_windows", "forward_windows", dev,
              _pool_plan(_key(d), "windows", R).ws_forward, C.byref(d), C.byref(params), _ptr(gate_scale),
              _ptr(update_scale), _ptr(pool), R, _ptr(starts), _ptr(initial_h), _ptr(hs))
    return hs


def train_windows_supported(T, B, F, H, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=torch.float32, flags=0):
    """``forward_windows_train`` / ``backward_windows`` run this descriptor (include/fastgrnn_hip.h,
    ``fastgrnn_hip_train_windows_supported``); where they do not, ``FastGRNNCUDA.unroll_windows`` gathers the windows
    and calls the existing forward.  ``flags``: FLAG_BATCH_MAJOR / FLAG_GRAD_LAST."""
    if dtype not in _DTYPES:
        return False
    return _pool_plan((T, B, F, H, w_rank, u_rank, int(gate_nl), int(update_nl), _DTYPES[dtype], int(flags)),
                      "train_windows", T).supported


def check_starts_range(starts, R, T):
    """The one host range check of every windowed call (``forward_windows``, ``forward_windows_train``,
    ``rnn.gather_windows``): ``T`` fits the pool and ``0 <= starts[b] <= R - T``, with one ``aminmax`` (one
    device-to-host copy); ``ValueError`` otherwise.  An empty ``starts`` checks ``T`` alone (``check=False``)."""
    if T < 1 or T > R:
        raise ValueError("forward_windows: window length T=%d does not fit a pool of %d frames" % (T, R))
    if starts.numel():
        lo, hi = torch.stack(torch.aminmax(starts)).tolist()
        if lo < 0 or hi > R - T:
            raise ValueError("forward_windows: starts must lie in [0, %d] (pool of %d frames, T=%d); got [%d, %d]"
                             % (R - T, R, T, lo, hi))


def _windows_operands(pool, starts, T, initial_h, bias_gate, bias_update, check, extra=()):
    """The argument checks every windowed call shares; (R, F, B, T, H, starts as int32).  ``extra``: further named
    per-unit vectors (the two scales of the affine forward), checked like the biases and held to the parameter dtype."""
    named = [(pool, "pool"), (starts, "starts"), (initial_h, "initial_h"), (bias_gate, "bias_gate"),
             (bias_update, "bias_update"), *extra]
    for t, n in named:
        _check_input(t, n)
    if pool.dim() != 2:
        raise RuntimeError("pool must be [frames, features]")
    if starts.dim() != 1 or starts.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("starts must be a 1-D int32 or int64 tensor")
    if starts.device != pool.device:
        raise RuntimeError("starts must be on the pool's device")
    R, F = pool.shape
    B, T = starts.numel(), int(T)
    H = initial_h.shape[-1]
    _expect(initial_h, (B, H), "initial_h")
    check_starts_range(starts if check else starts[:0], R, T)
    for t, n in named[3:]:
        if t.numel() != H:
            raise RuntimeError("%s must hold H=%d elements" % (n, H))
    for t in (initial_h, *(t for t, _ in extra)):
        if t.dtype != _param_dtype(pool.dtype):
            raise RuntimeError("fastgrnn: all operands must share dtype %s (got %s)" % (_param_dtype(pool.dtype), t.dtype))
    if starts.dtype != torch.int32:
        starts = starts.to(torch.int32)
    return R, F, B, T, H, starts


def forward_windows_train(pool, starts, T, w, u, bias_gate, bias_update, zeta, nu, initial_h, z_non_linearity,
                          batch_major=False, check=True, *, update_non_linearity=2):
    """Training forward over windows of a shared frame pool (include/fastgrnn_hip.h,
    ``fastgrnn_hip_forward_windows_train``): utterance ``b`` is the ``T`` consecutive rows of ``pool:[R,F]`` from row
    ``starts[b]`` on (H=256 reads the pool in place, H=128 gathers into the call's workspace).  Returns
    ``(hs, saved)``: the hidden states ``[T,B,H]`` (``[B,T,H]`` with ``batch_major``) and the fp32 pre-activation in the same layout, the one tensor ``backward_windows`` needs -- both
    bit for bit what ``forward_unroll(..., flags=FLAG_SAVE_PREACT)`` returns for the gathered windows.  ``starts`` and
    ``check`` as in ``forward_windows``.  Cells the calls do not hold (``train_windows_supported``) raise: there is no
    eager fallback here."""
    lib = _lib.load()
    R, F, B, T, H, starts = _windows_operands(pool, starts, T, initial_h, bias_gate, bias_update, check)
    flags = _lib.FLAG_BATCH_MAJOR if batch_major else 0
    plan, params, _, _ = _describe(T, B, F, H, w, u, None, None, None, None, bias_gate, bias_update, zeta, nu,
                                   pool.dtype, z_non_linearity, update_non_linearity, flags)
    d = plan.desc
    dev = pool.device
    shape = _seq_shape(T, B, H, batch_major, False)
    with torch.cuda.device(dev):
        hs = torch.empty(shape, dtype=pool.dtype, device=dev)
        saved = torch.empty(shape, dtype=torch.float32, device=dev)
        _call(lib.fastgrnn_hip_forward_windows_train, "fastgrnn forward_windows_train", "forward_windows_train", dev,
              _pool_plan(_key(d), "train_windows", R).ws_forward, C.byref(d), C.byref(params), _ptr(pool), R,
              _ptr(starts), _ptr(initial_h), _ptr(hs), _ptr(saved))
    return hs, saved


def backward_windows(grad_h, pool, starts, T, hidden_states, saved, zeta, nu, w, u, bias_gate, bias_update, initial_h,
                     z_non_linearity, batch_major=False, grad_last=False, *, update_non_linearity=2):
    """Backward of ``forward_windows_train`` (include/fastgrnn_hip.h, ``fastgrnn_hip_backward_windows``).  ``grad_h``:
    the layout of ``hidden_states``, or ``[B,H]`` with ``grad_last`` (the gradient of the last state alone).  Returns
    the 12-tuple of ``backward_unroll`` with an empty ``d_input``: the gradient with respect to the pool is a
    scatter-add over overlapping windows and is not built.  The parameter gradients are views of one flat buffer, as
    in ``backward_unroll``.  ``starts`` must be the (range-checked) starts of the forward."""
    lib = _lib.load()
    for t, n in ((grad_h, "grad_h"), (hidden_states, "hidden_states"), (saved, "saved")):
        _check_input(t, n)
    R, F, B, T, H, starts = _windows_operands(pool, starts, T, initial_h, bias_gate, bias_update, False)
    lead = (B, T) if batch_major else (T, B)
    _expect(grad_h, (B, H) if grad_last else lead + (H,), "grad_h")
    _expect(hidden_states, lead + (H,), "hidden_states")
    _expect(saved, lead + (H,), "saved")
    if grad_h.dtype != pool.dtype or hidden_states.dtype != pool.dtype or saved.dtype != _param_dtype(pool.dtype):
        raise RuntimeError("fastgrnn backward: operand dtypes differ")
    flags = (_lib.FLAG_BATCH_MAJOR if batch_major else 0) | (_lib.FLAG_GRAD_LAST if grad_last else 0)
    plan, params, _, _ = _describe(T, B, F, H, w, u, None, None, None, None, bias_gate, bias_update, zeta, nu,
                                   pool.dtype, z_non_linearity, update_non_linearity, flags)
    d = plan.desc
    dev = pool.device
    pdt = initial_h.dtype
    shapes = [(H, F), (H, H), (1, H), (1, H), (1, 1), (1, 1)]
    with torch.cuda.device(dev):
        d_old_h = torch.empty((B, H), dtype=pdt, device=dev)
        views, slots = _flat_grads(False, False, shapes, [a * b for a, b in shapes], pdt, dev)
        out = [_NONE, *views[-4:], d_old_h, *slots]
        grads = _lib.Grads(*map(_ptr, out))
        _call(lib.fastgrnn_hip_backward_windows, "fastgrnn backward_windows", "backward_windows", dev,
              _pool_plan(_key(d), "train_windows", R).ws_backward, C.byref(d), C.byref(params), _ptr(grad_h),
              _ptr(pool), R, _ptr(starts), _ptr(hidden_states), _ptr(saved), _ptr(initial_h), C.byref(grads))
    return out


def backward_unroll(grad_h, input, hidden_states, zeta, nu, w, u, z, h_prime, initial_h, w1, w2, u1, u2,
                    z_non_linearity, *, update_non_linearity=2, flags=0, bias_gate=None, bias_update=None,
                    need_dx=True):
    """fastgrnn_cuda.cpp:182-232 -> 12 tensors (.cu:556).  With ``flags & FLAG_SAVE_PREACT``
    (extension, kernel path 2) ``z`` is the pre-activation tensor returned by
    ``forward_unroll(..., flags=FLAG_SAVE_PREACT)``, ``h_prime`` is ignored and the two bias
    tensors must be given."""
    return _backward_impl(grad_h, input, hidden_states, zeta, nu, w, u, z, h_prime, initial_h,
                          w1, w2, u1, u2, z_non_linearity, True, update_non_linearity, flags,
                          bias_gate=bias_gate, bias_update=bias_update, need_dx=need_dx)
