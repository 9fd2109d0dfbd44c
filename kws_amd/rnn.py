"""Host-side mirror of the reference's GPU FastGRNN classes (/root/reference rnn.py):

* ``FastGRNNCUDACell``        rnn.py:454-549   single-step cell
* ``FastGRNNCUDA``            rnn.py:738-889   unrolled module (the class the build sits behind)
* ``FastGRNNFunction``        rnn.py:891-905   autograd glue, single step
* ``FastGRNNUnrollFunction``  rnn.py:907-972   autograd glue, unrolled

Same constructor keywords, same parameter names and ``[out,in]`` shapes (so reference
state dicts ``rnn_list.{l}.W|U|W1|W2|U1|U2|bias_gate|bias_update|zeta|nu`` load), same
gate-code table, zero ``h0`` default, ``batch_first`` handling and error behaviour, with
these deliberate differences:

* the GPU gate is ``torch.cuda.is_available()`` (ROCm reports HIP devices there), not
  ``utils.findCUDA()`` which looks for nvcc (utils.py:12-36);
* ``device=`` may be passed explicitly (e.g. a specific ``cuda:N`` for one-process-per-GPU
  data parallel, or ``"cpu"`` to inspect parameter layout without a GPU -- calling
  ``forward`` on CPU tensors still raises like CHECK_CUDA, fastgrnn_cuda.cpp:69);
* non-Parameter placeholders for absent operands are registered buffers so ``.to()``
  keeps them beside the parameters;
* the tanh-gate backward uses d_tanh (reference defect .cu:519-521 not reproduced).
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, _route, fastgrnn_cuda, utils

NON_LINEARITY = {"sigmoid": 0, "relu": 1, "tanh": 2}   # rnn.py:478,751


def _resolve_device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        # same message and exception type as rnn.py:476-477,749-750
        raise Exception('FastGRNNCUDA is supported only on GPU devices.')
    return torch.device("cuda", torch.cuda.current_device())


class FastGRNNFunction(Function):
    """rnn.py:891-905."""

    @staticmethod
    def forward(ctx, input, bias_gate, bias_update, zeta, nu, old_h, w, u, w1, w2, u1, u2, gate_non_linearity):
        outputs = fastgrnn_cuda.forward(input.contiguous(), w, u, bias_gate, bias_update, zeta, nu,
                                        old_h.contiguous(), gate_non_linearity, w1, w2, u1, u2)
        new_h = outputs[0]
        variables = [input, old_h, zeta, nu, w, u] + outputs[1:] + [w1, w2, u1, u2]
        ctx.save_for_backward(*variables)
        ctx.non_linearity = gate_non_linearity
        return new_h

    @staticmethod
    def backward(ctx, grad_h):
        input, old_h, zeta, nu, w, u, z, h_prime, w1, w2, u1, u2 = ctx.saved_tensors
        outputs = fastgrnn_cuda.backward(grad_h.contiguous(), input.contiguous(), old_h.contiguous(), zeta, nu,
                                         w, u, z, h_prime, w1, w2, u1, u2, ctx.non_linearity)
        return _as_autograd_grads(outputs, ctx.needs_input_grad)


def gather_windows(pool, starts, T, check=True, batch_first=True):
    """``[B,T,F]``: window ``b`` = rows ``starts[b] .. starts[b]+T-1`` of ``pool:[R,F]``, materialised (what
    ``forward_windows`` avoids where the windowed scans hold the cell).  ``batch_first=False``: its ``[T,B,F]`` copy,
    what a module that is not ``batch_first`` takes."""
    T = int(T)
    fastgrnn_cuda.check_starts_range(starts if check else starts[:0], pool.shape[0], T)
    windows = pool[starts.long()[:, None] + torch.arange(T, device=pool.device)]
    return windows if batch_first else windows.transpose(0, 1).contiguous()


class FastGRNNUnrollFunction(Function):
    """rnn.py:907-972.  Same inputs, same gradients; what is SAVED between the two passes is
    an internal matter: on the split-precision kernel path the forward keeps one auxiliary
    tensor (the pre-activation W.x+U.h) instead of the reference's two (z_s, h_prime_s) and the
    backward recomputes the gates from it -- one [T,B,H] HBM write and read less per step."""

    @staticmethod
    def forward(ctx, input, bias_gate, bias_update, zeta, nu, old_h, w, u, w1, w2, u1, u2, gate_non_linearity,
                batch_major=False, last_state=False, route=None):
        """``batch_major`` (not in the reference signature): ``input`` / the result are [B,T,.] and the
        kernels index them in place (FLAG_BATCH_MAJOR) instead of working on transposed copies.
        ``last_state``: return h_T [B,H] alone -- what the classifier head reads
        (model.py:227) -- so that the backward receives a [B,H] gradient instead of the dense, all-but-one-
        step-zero [T,B,H] tensor autograd builds for ``hs[-1]`` (FLAG_GRAD_LAST: not written, not read).
        ``route``: the ``_route.Route`` of this call where the module has looked it up already."""
        old_h = old_h.contiguous()
        if route is None:
            route = _route.route(_route.Signature(
                _route.PLAIN, input.shape, input.stride(), input.dtype, input.is_cuda, old_h.shape[1],
                *_route.ranks(w1, u1), gate_non_linearity, 2, bool(batch_major), bool(last_state), _route.APPLY))
        # (the trainer's [T,B,F] view of a [B,F,T] batch: the reference copies it here; under FLAG_X_BFT its base goes)
        input = input.permute(1, 2, 0) if route.present == _route.BFT_BASE else input.contiguous()
        outputs = fastgrnn_cuda.forward_unroll(input, w, u, bias_gate, bias_update, zeta, nu, old_h,
                                               gate_non_linearity, w1, w2, u1, u2, flags=route.flags)
        hidden_states = outputs[0]
        # saved beside hs: (pre-activation, the factorised cells' rank-space vector [U1.h | W1.x]) + biases, or (z_s, h_prime_s)
        biases = [bias_gate, bias_update] if route.saved == _route.PREACT else []
        ctx.save_for_backward(input, hidden_states, zeta, nu, w, u, outputs[1], outputs[-1], old_h, w1, w2, u1, u2,
                              *biases)
        ctx.gate_non_linearity, ctx.route = gate_non_linearity, route
        if route.post == _route.LAST_STEP:
            return _route.last_step(hidden_states, route.flags).clone()
        return hidden_states

    @staticmethod
    def backward(ctx, grad_h):
        route, flags = ctx.route, ctx.route.flags
        input, hidden_states, zeta, nu, w, u, z_s, aux2, old_h, w1, w2, u1, u2, *biases = ctx.saved_tensors
        if route.post == _route.LAST_STEP:
            if route.grad_last:
                flags |= _lib.FLAG_GRAD_LAST            # the kernel takes the [B,H] gradient as it is
            else:                                        # other kernel paths: the dense form autograd would build
                dense = torch.zeros_like(hidden_states)
                _route.last_step(dense, flags).copy_(grad_h)
                grad_h = dense
        bias_gate, bias_update = biases or (None, None)
        outputs = fastgrnn_cuda.backward_unroll(grad_h.contiguous(), input, hidden_states, zeta, nu, w, u, z_s, aux2,
                                                old_h, w1, w2, u1, u2, ctx.gate_non_linearity, flags=flags,
                                                bias_gate=bias_gate, bias_update=bias_update,
                                                need_dx=ctx.needs_input_grad[0])
        if flags & _lib.FLAG_X_BFT:                     # d_input was produced as [B,F,T]: hand back the [T,B,F] view
            outputs = [outputs[0].permute(2, 0, 1) if outputs[0].numel() else outputs[0]] + list(outputs[1:])
        return _as_autograd_grads(outputs, ctx.needs_input_grad) + (None, None, None)


class FastGRNNWindowsFunction(Function):
    """Autograd glue over ``fastgrnn_cuda.forward_windows_train`` / ``backward_windows``: the unrolled cell on windows
    of a frame pool, differentiable with respect to the parameters and the initial state.  The pool is data: it gets no
    gradient (that would be a scatter-add over overlapping windows, which is not built), and nothing but the pool
    itself and the ``[B]`` starts is kept of the input between the two passes."""

    @staticmethod
    def forward(ctx, pool, starts, T, bias_gate, bias_update, zeta, nu, old_h, w, u, gate_non_linearity, batch_major,
                last_state, check):
        old_h = old_h.contiguous()
        if starts.dtype != torch.int32:
            if check:                                    # (checked here, on the caller's values: the cast could wrap)
                fastgrnn_cuda.check_starts_range(starts, pool.shape[0], int(T))
                check = False
            starts = starts.to(torch.int32)
        hs, saved = fastgrnn_cuda.forward_windows_train(pool, starts, T, w, u, bias_gate, bias_update, zeta, nu, old_h,
                                                        gate_non_linearity, batch_major=batch_major, check=check)
        ctx.save_for_backward(pool, starts, hs, saved, zeta, nu, w, u, bias_gate, bias_update, old_h)
        ctx.T, ctx.gate_non_linearity = int(T), gate_non_linearity
        ctx.batch_major, ctx.last_state = bool(batch_major), bool(last_state)
        if last_state:
            return (hs[:, -1] if batch_major else hs[-1]).clone()
        return hs

    @staticmethod
    def backward(ctx, grad_h):
        pool, starts, hs, saved, zeta, nu, w, u, bias_gate, bias_update, old_h = ctx.saved_tensors
        g = fastgrnn_cuda.backward_windows(grad_h.contiguous(), pool, starts, ctx.T, hs, saved, zeta, nu, w, u,
                                           bias_gate, bias_update, old_h, ctx.gate_non_linearity,
                                           batch_major=ctx.batch_major, grad_last=ctx.last_state)
        # (pool, starts, T, bias_gate, bias_update, zeta, nu, old_h, w, u, nl, batch_major, last_state, check)
        grads = [None, None, None, g[1], g[2], g[3], g[4], g[5], g[6], g[7]]
        grads = [v if need else None for v, need in zip(grads, ctx.needs_input_grad[:10])]
        return tuple(grads) + (None, None, None, None)


def _as_autograd_grads(outputs, needs):
    """Map the operator's 12-tuple (.cu:556) onto the Function's 13 inputs
    (input, bias_gate, bias_update, zeta, nu, old_h, w, u, w1, w2, u1, u2, nl):
    same order + trailing None (rnn.py:905,972); empty(0) placeholders become None."""
    grads = []
    for g, need in zip(outputs, needs[:12]):
        grads.append(g if (need and g.numel() != 0) else None)
    return tuple(grads + [None])


def _make_params(mod, input_size, hidden_size, wRank, uRank, zetaInit, nuInit, device):
    """Parameter set of rnn.py:491-517 / 782-805: [out,in] layout, 0.1*randn, biases one."""
    if wRank is None:
        mod.W = nn.Parameter(0.1 * torch.randn([hidden_size, input_size], device=device))
        mod.register_buffer("W1", torch.empty(0), persistent=False)
        mod.register_buffer("W2", torch.empty(0), persistent=False)
    else:
        mod.register_buffer("W", torch.empty(0), persistent=False)
        mod.W1 = nn.Parameter(0.1 * torch.randn([wRank, input_size], device=device))
        mod.W2 = nn.Parameter(0.1 * torch.randn([hidden_size, wRank], device=device))
    if uRank is None:
        mod.U = nn.Parameter(0.1 * torch.randn([hidden_size, hidden_size], device=device))
        mod.register_buffer("U1", torch.empty(0), persistent=False)
        mod.register_buffer("U2", torch.empty(0), persistent=False)
    else:
        mod.register_buffer("U", torch.empty(0), persistent=False)
        mod.U1 = nn.Parameter(0.1 * torch.randn([uRank, hidden_size], device=device))
        mod.U2 = nn.Parameter(0.1 * torch.randn([hidden_size, uRank], device=device))
    mod.bias_gate = nn.Parameter(torch.ones([1, hidden_size], device=device))
    mod.bias_update = nn.Parameter(torch.ones([1, hidden_size], device=device))
    mod.zeta = nn.Parameter(zetaInit * torch.ones([1, 1], device=device))
    mod.nu = nn.Parameter(nuInit * torch.ones([1, 1], device=device))


def _get_vars(mod):
    # rnn.py:536-549, 828-841
    Vars = []
    if mod._num_W_matrices == 1:
        Vars.append(mod.W)
    else:
        Vars.extend([mod.W1, mod.W2])
    if mod._num_U_matrices == 1:
        Vars.append(mod.U)
    else:
        Vars.extend([mod.U1, mod.U2])
    Vars.extend([mod.bias_gate, mod.bias_update, mod.zeta, mod.nu])
    return Vars


# ---- sparsification bookkeeping (rnn.py:843-889), all on the parameters' device ----------
def _get_model_size(mod):
    """rnn.py:843-865: 4 bytes x (non-zeros of the W/U matrices when their sparsity flag is set, else their
    sizes) + biases + zeta, nu.  The reference counts on CPU copies; ``isSparse`` is the truthiness of the
    sparsity value exactly as there (rnn.py:855-860)."""
    mats = mod.getVars()
    endW = mod._num_W_matrices
    endU = endW + mod._num_U_matrices
    total = 2
    for i in range(0, endW):
        total += utils.countNNZ(mats[i], mod._wSparsity)
    for i in range(endW, endU):
        total += utils.countNNZ(mats[i], mod._uSparsity)
    for i in range(endU, len(mats)):
        total += utils.countNNZ(mats[i], False)
    return total * 4


def _copy_previous_UW(mod):
    mats = mod.getVars()
    n = mod._num_W_matrices + mod._num_U_matrices
    mod.oldmats = [mats[i].detach().clone() for i in range(n)]


def _sparsify(mod):
    """Hard-threshold W/U (or their factors) IN PLACE and remember the support.  This is what the CPU cell does
    (``mats[i].data = utils.hardThreshold(...)``, rnn.py:433-443); the reference's CUDA class rebinds list
    entries instead (rnn.py:875-883), which leaves its parameters untouched -- a defect not reproduced."""
    mats = mod.getVars()
    endW = mod._num_W_matrices
    endU = endW + mod._num_U_matrices
    for i in range(0, endW):
        utils.hardThreshold(mats[i], mod._wSparsity)
    for i in range(endW, endU):
        utils.hardThreshold(mats[i], mod._uSparsity)
    _copy_previous_UW(mod)


def _sparsify_with_support(mod):
    mats = mod.getVars()
    endU = mod._num_W_matrices + mod._num_U_matrices
    for i in range(0, endU):
        utils.supportBasedThreshold(mats[i], mod.oldmats[i])


class FastGRNNCUDACell(nn.Module):
    """Single-step GPU cell (rnn.py:454-549).

    z_t = non_linearity(W x_t + U h_{t-1} + B_g);  h_t^ = tanh(W x_t + U h_{t-1} + B_h)
    h_t = z_t*h_{t-1} + (sigmoid(zeta)(1-z_t) + sigmoid(nu))*h_t^
    """

    def __init__(self, input_size, hidden_size, gate_nonlinearity="sigmoid",
                 update_nonlinearity="tanh", wRank=None, uRank=None, zetaInit=1.0, nuInit=-4.0,
                 wSparsity=1.0, uSparsity=1.0, name="FastGRNNCUDACell", device=None):
        super().__init__()
        self.device = _resolve_device(device)
        if update_nonlinearity != "tanh":
            raise ValueError("FastGRNNCUDA fixes update_nonlinearity to tanh (rnn.py:741-742)")
        self._input_size = input_size
        self._hidden_size = hidden_size
        self._gate_nonlinearity = gate_nonlinearity
        self._update_nonlinearity = update_nonlinearity
        self._zetaInit = zetaInit
        self._nuInit = nuInit
        self._name = name
        self._wRank, self._uRank = wRank, uRank
        self._wSparsity, self._uSparsity = wSparsity, uSparsity
        self._num_W_matrices = 1 if wRank is None else 2
        self._num_U_matrices = 1 if uRank is None else 2
        self._num_biases = 2
        self._num_weight_matrices = [self._num_W_matrices, self._num_U_matrices, self._num_biases]
        _make_params(self, input_size, hidden_size, wRank, uRank, zetaInit, nuInit, self.device)
        self._gate_non_linearity = NON_LINEARITY[gate_nonlinearity]   # KeyError on others, as rnn.py:512
        self.oldmats = []

    @property
    def name(self):
        return self._name

    @property
    def cellType(self):
        return "FastGRNNCUDACell"

    @property
    def state_size(self):
        return self._hidden_size

    @property
    def input_size(self):
        return self._input_size

    @property
    def output_size(self):
        return self._hidden_size

    def forward(self, input, state):
        return FastGRNNFunction.apply(input, self.bias_gate, self.bias_update, self.zeta, self.nu, state,
                                      self.W, self.U, self.W1, self.W2, self.U1, self.U2,
                                      self._gate_non_linearity)

    def getVars(self):
        return _get_vars(self)

    def get_model_size(self):
        return _get_model_size(self)

    def copy_previous_UW(self):
        _copy_previous_UW(self)

    def sparsify(self):
        _sparsify(self)

    def sparsifyWithSupport(self):
        _sparsify_with_support(self)


class FastGRNNCUDA(nn.Module):
    """Unrolled GPU FastGRNN (rnn.py:738-889).  ``update_nonlinearity`` is fixed to tanh,
    only ``gate_nonlinearity`` is configurable (rnn.py:741-742)."""

    def __init__(self, input_size, hidden_size, gate_nonlinearity="sigmoid",
                 update_nonlinearity="tanh", wRank=None, uRank=None,
                 wSparsity=1.0, uSparsity=1.0, zetaInit=1.0, nuInit=-4.0,
                 batch_first=False, name="FastGRNNCUDA", device=None):
        super().__init__()
        self.device = _resolve_device(device)
        if update_nonlinearity != "tanh":
            raise ValueError("FastGRNNCUDA fixes update_nonlinearity to tanh (rnn.py:741-742)")
        self._input_size = input_size
        self._hidden_size = hidden_size
        self._zetaInit = zetaInit
        self._nuInit = nuInit
        self._name = name
        self._wRank, self._uRank = wRank, uRank
        self._wSparsity, self._uSparsity = wSparsity, uSparsity
        self._num_W_matrices = 1 if wRank is None else 2
        self._num_U_matrices = 1 if uRank is None else 2
        self._num_biases = 2
        self._num_weight_matrices = [self._num_W_matrices, self._num_U_matrices, self._num_biases]
        self.oldmats = []
        self.batch_first = batch_first
        _make_params(self, input_size, hidden_size, wRank, uRank, zetaInit, nuInit, self.device)
        self._gate_non_linearity = NON_LINEARITY[gate_nonlinearity]

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.device = self.bias_gate.device
        return out

    def forward(self, input, hiddenState=None, cell_state=None, last_state=False):
        """input: [timesteps, batch, features] (or [batch, timesteps, features] when
        ``batch_first``); hiddenState: [batch, state_size], zeros if not provided
        (rnn.py:807-826).  Returns every hidden state, same leading layout as the input -- or, with
        ``last_state=True`` (not in the reference signature; the last layer under the classifier head,
        model.py:227), the final state [batch, state_size] alone: equal to ``forward(...)[-1]`` with the same
        gradients, without the dense mostly-zero grad_hs on the way back; under ``torch.no_grad()`` the
        hidden-state sequence is not written at all (FLAG_HS_LAST)."""
        if not input.is_cuda:
            input = input.to(self.device)
        route = _route.route(_route.Signature(
            _route.PLAIN, input.shape, input.stride(), input.dtype, input.is_cuda, self._hidden_size,
            *_route.ranks(self.W1, self.U1), self._gate_non_linearity, 2, self.batch_first is True, bool(last_state),
            _route.grad_mode()))
        if route.present == _route.TRANSPOSE_COPY:
            input = input.transpose(0, 1).contiguous()
        if hiddenState is None:
            # bf16 sequences (BASELINE config "bf16 with fp32 master grads") keep an fp32 state and parameters
            hiddenState = _route.zero_state(route.dims[1], self._hidden_size, fastgrnn_cuda._param_dtype(input.dtype),
                                            input.device)
        if not hiddenState.is_cuda:
            hiddenState = hiddenState.to(self.device)
        if route.saved is None:                          # nothing will be differentiated: hs, or h_T, alone
            input = input.permute(1, 2, 0) if route.present == _route.BFT_BASE else input.contiguous()
            result = fastgrnn_cuda.forward_unroll(input, self.W, self.U, self.bias_gate, self.bias_update, self.zeta,
                                                  self.nu, hiddenState.contiguous(), self._gate_non_linearity, self.W1,
                                                  self.W2, self.U1, self.U2, want_gates=False, flags=route.flags)[0]
        else:
            result = FastGRNNUnrollFunction.apply(input, self.bias_gate, self.bias_update, self.zeta, self.nu,
                                                  hiddenState, self.W, self.U, self.W1, self.W2, self.U1, self.U2,
                                                  self._gate_non_linearity, bool(route.flags & _lib.FLAG_BATCH_MAJOR),
                                                  bool(last_state), route)
        return result.transpose(0, 1) if route.post == _route.TRANSPOSE_BACK else result

    @torch.no_grad()
    def forward_windows(self, pool, starts, T, hiddenState=None, last_state=False, check=True):
        """Inference over windows of a shared frame pool (not in the reference; its detector gathers every window,
        inferencetry.py:165-227): utterance ``b`` is the ``T`` consecutive rows of ``pool:[R,F]`` from row
        ``starts[b]`` on.  Returns what ``forward`` returns for the gathered batch under ``torch.no_grad()`` -- hs
        ``[T,B,H]`` (``[B,T,H]`` with ``batch_first``), or h_T ``[B,H]`` with ``last_state`` -- without a graph.
        Where the windowed scans hold the cell (``fastgrnn_cuda.windows_supported``) the pool is read in place;
        elsewhere (factorised weights, other sizes, bf16) the windows are gathered and ``forward`` runs them."""
        pool = pool.to(self.device) if not pool.is_cuda else pool
        starts = starts.to(pool.device)
        B, H, T = starts.numel(), self._hidden_size, int(T)
        h0 = _route.zero_state(B, H, fastgrnn_cuda._param_dtype(pool.dtype), pool.device) if hiddenState is None \
            else hiddenState.to(pool.device).contiguous()
        bm = self.batch_first is True
        flags = (_lib.FLAG_BATCH_MAJOR if bm else 0) | (_lib.FLAG_HS_LAST if last_state else 0)
        if pool.dim() == 2 and fastgrnn_cuda.windows_supported(T, B, pool.shape[1], H, *_route.ranks(self.W1, self.U1),
                                                               self._gate_non_linearity, 2, pool.dtype, flags):
            return fastgrnn_cuda.forward_windows(pool.contiguous(), starts, T, self.W, self.U, self.bias_gate,
                                                 self.bias_update, self.zeta, self.nu, h0, self._gate_non_linearity,
                                                 batch_major=bm, last_state=last_state, check=check)
        return self.forward(gather_windows(pool, starts, T, check, bm), hiddenState=h0, last_state=last_state)

    def unroll_windows(self, pool, starts, T, hiddenState=None, last_state=False, check=True):
        """Training on windows of a shared frame pool (not in the reference): utterance ``b`` is the ``T`` consecutive
        rows of ``pool:[R,F]`` from row ``starts[b]`` on, so a batch is ``B`` start rows -- no assembled ``[B,T,F]``
        batch, and random time-shift crops are other start rows.  Returns what ``forward`` returns for the gathered
        batch -- hs ``[T,B,H]`` (``[B,T,H]`` with ``batch_first``) or h_T ``[B,H]`` with ``last_state`` -- differentiable
        with respect to the parameters and ``hiddenState``.  The pool is data and gets no gradient (a scatter-add over
        overlapping windows, not built): a pool that requires grad raises ``ValueError``.  ``check`` as in
        ``forward_windows``.  Where the training calls hold the cell (``fastgrnn_cuda.train_windows_supported``) the
        library reads the pool itself and no ``[B,T,F]`` batch is kept; elsewhere (factorised weights, other sizes,
        bf16, fp64) the windows are gathered and ``forward`` runs them: exactly ``forward(gather_windows(...))``."""
        if pool.requires_grad:
            raise ValueError("unroll_windows: the pool must not require grad -- its gradient is a scatter-add over "
                             "overlapping windows, which is not built (the pool is a model's input data)")
        pool = pool.to(self.device) if not pool.is_cuda else pool
        starts = starts.to(pool.device)
        B, H, T = starts.numel(), self._hidden_size, int(T)
        bm = self.batch_first is True
        flags = (_lib.FLAG_BATCH_MAJOR if bm else 0) | (_lib.FLAG_GRAD_LAST if last_state else 0)
        if pool.is_cuda and pool.dim() == 2 and fastgrnn_cuda.train_windows_supported(
                T, B, pool.shape[1], H, *_route.ranks(self.W1, self.U1), self._gate_non_linearity, 2, pool.dtype, flags):
            h0 = _route.zero_state(B, H, pool.dtype, pool.device) if hiddenState is None else hiddenState.to(pool.device)
            return FastGRNNWindowsFunction.apply(pool.contiguous(), starts, T, self.bias_gate, self.bias_update,
                                                 self.zeta, self.nu, h0, self.W, self.U, self._gate_non_linearity,
                                                 bm, bool(last_state), bool(check))
        return self.forward(gather_windows(pool, starts, T, check, bm), hiddenState=hiddenState, last_state=last_state)

    def getVars(self):
        return _get_vars(self)

    def get_model_size(self):
        """rnn.py:843-865."""
        return _get_model_size(self)

    def copy_previous_UW(self):
        """rnn.py:867-873."""
        _copy_previous_UW(self)

    def sparsify(self):
        """rnn.py:875-883 (with the in-place effect the CPU cell has, rnn.py:433-443)."""
        _sparsify(self)

    def sparsifyWithSupport(self):
        """rnn.py:885-889."""
        _sparsify_with_support(self)
