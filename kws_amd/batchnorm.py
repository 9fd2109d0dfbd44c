"""Eval-mode FastGRNN with BatchNorm (/root/reference rnn.py:316-452 ``FastGRNNBatchNormCell``, rnn.py:709-735
``FastGRNNBatchNorm``): the cell of the reference's trained keyword spotter, run on the fused scans.

In eval mode every ``BatchNorm1d`` is a per-unit affine map ``a*v + b`` with ``a = gamma / sqrt(running_var + eps)``
and ``b = beta - running_mean * a``, so the reference cell (rnn.py:377-414)

    pre_gate   = bn_gate  (bn_w(x.W) + bn_u(h.U) + bias_gate)
    pre_update = bn_update(bn_w(x.W) + bn_u(h.U) + bias_update)

folds to one shared product and two per-unit scales (``fold_batchnorm``):

    w'[j,:] = a_w[j] * W[:,j]      u'[j,:] = a_u[j] * U[:,j]      p = w'.x_t + u'.h_{t-1}
    z  = gate  (a_gate   * p + a_gate   * (b_w + b_u + bias_gate)   + b_gate)
    h' = update(a_update * p + a_update * (b_w + b_u + bias_update) + b_update)

which is ``fastgrnn_cuda.forward_unroll_affine``: one launch per layer (plus the frame GEMM of the wide layers).

Same constructor keywords, parameter names and layouts as the reference (``W:[F,H]``, ``U:[H,H]``: the CPU cell's
layout, not ``FastGRNNCUDA``'s ``[out,in]``), the four ``BatchNorm1d`` modules ``bn_w``, ``bn_u``, ``bn_gate``,
``bn_update``, and the cell registered as both ``cell`` and ``unrollRNN.RNNCell`` -- the reference checkpoint's key
set, duplicates included, loads with ``strict=True``.  Differences:

* ``training=True`` raises ``NotImplementedError``: batch statistics at every frame need a reduction over the whole
  batch inside every step of the scan (a grid-wide synchronisation per frame), which the fused scans do not have;
* eval mode runs through an autograd function whose backward raises: fine-tuning fails loudly instead of training
  nothing;
* factorised weights (``wRank`` / ``uRank``) raise ``ValueError`` (the reference cell cannot run them either: its
  forward reads ``self.W``, rnn.py:378);
* ``forward`` accepts ``last_state=True`` (not in the reference signature), like ``FastGRNNCUDA``: the final state
  ``[B,H]`` alone, without writing the hidden-state sequence.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, _route, fastgrnn_cuda
from .rnn import NON_LINEARITY, _resolve_device, _sparsify, _sparsify_with_support, gather_windows

_TRAINING_MSG = ("FastGRNNBatchNorm runs in eval mode only (training=False / model.eval()): training-mode BatchNorm "
                 "normalises every frame with the statistics of the whole batch at that frame, which needs a "
                 "grid-wide reduction inside every step of the fused scan")


def _bn_affine(bn):
    """(a, b) with bn(v) == a * v + b in eval mode (torch.nn.functional.batch_norm, running statistics)."""
    rv = bn.running_var if bn.running_var is not None else torch.ones_like(bn.weight)
    rm = bn.running_mean if bn.running_mean is not None else torch.zeros_like(bn.weight)
    a = torch.rsqrt(rv + bn.eps)
    if bn.weight is not None:
        a = a * bn.weight
    b = -rm * a
    if bn.bias is not None:
        b = b + bn.bias
    return a, b


@torch.no_grad()
def fold_batchnorm(cell):
    """The eval-mode cell as the affine forward's operands, in the cell's dtype and device:
    ``(w [H,F], u [H,H], bias_gate [H], bias_update [H], gate_scale [H], update_scale [H])`` (``[out,in]`` layout;
    zeta, nu are the cell's own)."""
    a_w, b_w = _bn_affine(cell.bn_w)
    a_u, b_u = _bn_affine(cell.bn_u)
    a_g, b_g = _bn_affine(cell.bn_gate)
    a_c, b_c = _bn_affine(cell.bn_update)
    w = (cell.W * a_w).t().contiguous()                    # w'[j,:] = a_w[j] W[:,j]
    u = (cell.U * a_u).t().contiguous()
    shared = b_w + b_u
    bias_gate = (a_g * (shared + cell.bias_gate.reshape(-1)) + b_g).contiguous()
    bias_update = (a_c * (shared + cell.bias_update.reshape(-1)) + b_c).contiguous()
    return w, u, bias_gate, bias_update, a_g.contiguous(), a_c.contiguous()


class _Unroll(nn.Module):
    """Holds the cell under the reference's second name (``unrollRNN.RNNCell``, rnn.py:561-572)."""

    def __init__(self, cell):
        super().__init__()
        self.RNNCell = cell


class _BatchNormInference(Function):
    """Forward: the folded cell on the fused scan.  Backward: refused (eval-mode inference only)."""

    @staticmethod
    def forward(ctx, cell, input, h0, flags, *params):
        w, u, bg, bu, sg, sc = cell._folded()
        return fastgrnn_cuda.forward_unroll_affine(input, w, u, bg, bu, cell.zeta, cell.nu, sg, sc, h0,
                                                   cell._gate_code, cell._update_code, flags)

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("FastGRNNBatchNorm has no backward: the fused BatchNorm forward is eval-mode "
                                  "inference only. " + _TRAINING_MSG)


class FastGRNNBatchNormCell(nn.Module):
    """rnn.py:316-452.  The single-step ``forward`` is the reference's formula in torch ops (eval mode, any device);
    the fused scan is ``FastGRNNBatchNorm``."""

    def __init__(self, input_size, hidden_size, gate_nonlinearity="sigmoid", update_nonlinearity="tanh",
                 wRank=None, uRank=None, wSparsity=1.0, uSparsity=1.0, zetaInit=1.0, nuInit=-4.0,
                 name="FastGRNNBatchNorm", device=None):
        super().__init__()
        if wRank is not None or uRank is not None:
            raise ValueError("FastGRNNBatchNorm takes dense W and U only (wRank=%r, uRank=%r): the reference "
                             "BatchNorm cell reads self.W / self.U (rnn.py:378)" % (wRank, uRank))
        if gate_nonlinearity not in NON_LINEARITY or update_nonlinearity != "tanh":
            raise ValueError("FastGRNNBatchNorm: gate sigmoid / relu / tanh and update tanh "
                             "(got %r, %r)" % (gate_nonlinearity, update_nonlinearity))
        dev = _resolve_device(device)
        self._input_size, self._hidden_size = input_size, hidden_size
        self._gate_nonlinearity, self._update_nonlinearity = gate_nonlinearity, update_nonlinearity
        self._gate_code, self._update_code = NON_LINEARITY[gate_nonlinearity], NON_LINEARITY[update_nonlinearity]
        self._wRank, self._uRank = wRank, uRank
        self._wSparsity, self._uSparsity = wSparsity, uSparsity
        self._zetaInit, self._nuInit = zetaInit, nuInit
        self._num_W_matrices, self._num_U_matrices, self._num_biases = 1, 1, 2
        self._name = name
        self.W = nn.Parameter(0.1 * torch.randn([input_size, hidden_size], device=dev))        # rnn.py:345
        self.U = nn.Parameter(0.1 * torch.randn([hidden_size, hidden_size], device=dev))       # rnn.py:352
        self.bias_gate = nn.Parameter(torch.ones([1, hidden_size], device=dev))
        self.bias_update = nn.Parameter(torch.ones([1, hidden_size], device=dev))
        self.zeta = nn.Parameter(zetaInit * torch.ones([1, 1], device=dev))
        self.nu = nn.Parameter(nuInit * torch.ones([1, 1], device=dev))
        self.bn_w = nn.BatchNorm1d(hidden_size, device=dev)                                     # rnn.py:366-369
        self.bn_u = nn.BatchNorm1d(hidden_size, device=dev)
        self.bn_gate = nn.BatchNorm1d(hidden_size, device=dev)
        self.bn_update = nn.BatchNorm1d(hidden_size, device=dev)
        self.oldmats = []
        self._fold_key, self._fold = None, None

    @property
    def name(self):
        return self._name

    @property
    def cellType(self):
        return "FastGRNNBatchNorm"

    @property
    def state_size(self):
        return self._hidden_size

    @property
    def input_size(self):
        return self._input_size

    @property
    def output_size(self):
        return self._hidden_size

    def _fold_tensors(self):
        return [self.W, self.U, self.bias_gate, self.bias_update] + [
            t for bn in (self.bn_w, self.bn_u, self.bn_gate, self.bn_update)
            for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]

    def _folded(self):
        """fold_batchnorm(self), recomputed only when a parameter or running statistic has changed (``_version``
        counts in-place writes, ``data_ptr`` catches rebinding and ``.to()``)."""
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in self._fold_tensors())
        if key != self._fold_key:
            self._fold = fold_batchnorm(self)
            self._fold_key = key
        return self._fold

    def forward(self, input, state, training=True):
        """One step, rnn.py:373-414 in torch ops (reference semantics, including training-mode BatchNorm)."""
        wComp = torch.matmul(input, self.W)
        uComp = torch.matmul(state, self.U)
        wComp = self.bn_w(wComp) if training else self.bn_w.eval()(wComp)
        uComp = self.bn_u(uComp) if training else self.bn_u.eval()(uComp)
        pre_gate = self.bn_gate(wComp + uComp + self.bias_gate) if training else \
            self.bn_gate.eval()(wComp + uComp + self.bias_gate)
        pre_update = self.bn_update(wComp + uComp + self.bias_update) if training else \
            self.bn_update.eval()(wComp + uComp + self.bias_update)
        z = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}[self._gate_nonlinearity](pre_gate)
        c = torch.tanh(pre_update)
        return z * state + (torch.sigmoid(self.zeta) * (1.0 - z) + torch.sigmoid(self.nu)) * c

    def getVars(self):
        return [self.W, self.U, self.bias_gate, self.bias_update, self.zeta, self.nu]

    def get_model_size(self):
        """Bytes of the dense parameters at 4 bytes each (the BatchNorm layers fold into them)."""
        return 4 * (self.W.numel() + self.U.numel() + self.bias_gate.numel() + self.bias_update.numel() + 2)

    def sparsify(self):                                   # rnn.py:430-440, in place
        _sparsify(self)

    def sparsifyWithSupport(self):                        # rnn.py:442-449
        _sparsify_with_support(self)


class FastGRNNBatchNorm(nn.Module):
    """rnn.py:709-735: the unrolled BatchNorm FastGRNN, eval mode on the fused scans."""

    def __init__(self, input_size, hidden_size, gate_nonlinearity="sigmoid", update_nonlinearity="tanh",
                 wRank=None, uRank=None, wSparsity=1.0, uSparsity=1.0, zetaInit=1.0, nuInit=-4.0,
                 batch_first=False, device=None):
        super().__init__()
        self.cell = FastGRNNBatchNormCell(input_size, hidden_size, gate_nonlinearity=gate_nonlinearity,
                                          update_nonlinearity=update_nonlinearity, wRank=wRank, uRank=uRank,
                                          wSparsity=wSparsity, uSparsity=uSparsity, zetaInit=zetaInit,
                                          nuInit=nuInit, device=device)
        self.unrollRNN = _Unroll(self.cell)
        self.batch_first = batch_first
        self.training = True

    @property
    def device(self):
        return self.cell.W.device

    def getVars(self):
        return self.cell.getVars()

    def get_model_size(self):
        return self.cell.get_model_size()

    def sparsify(self):
        self.cell.sparsify()

    def sparsifyWithSupport(self):
        self.cell.sparsifyWithSupport()

    def forward(self, input, hiddenState=None, training=True, last_state=False):
        """input [T,B,F] (``[B,T,F]`` with ``batch_first``) -> every hidden state in the input's layout, or with
        ``last_state=True`` the final state ``[B,H]``.  ``training`` must be False (see the module docstring)."""
        if training:
            raise NotImplementedError(_TRAINING_MSG)
        cell = self.cell
        dev = cell.W.device
        if dev.type != "cuda":
            raise RuntimeError("FastGRNNBatchNorm.forward runs on the GPU only (parameters are on %s)" % dev)
        input = input.to(dev)
        if input.dtype != cell.W.dtype:
            raise RuntimeError("input dtype %s differs from the parameters' %s" % (input.dtype, cell.W.dtype))
        route = _route.route(_route.Signature(
            _route.AFFINE, input.shape, input.stride(), input.dtype, input.is_cuda, cell._hidden_size, 0, 0,
            cell._gate_code, cell._update_code, self.batch_first is True, bool(last_state), None))
        Bn, H = route.dims[1], cell._hidden_size
        if hiddenState is None:
            h0 = _route.zero_state(Bn, H, input.dtype, dev)
        else:
            h0 = hiddenState.to(dev).reshape(Bn, H).contiguous()
        # batch_first in place where the kernels index [B,T,.] (kernel path 2), else transposed as BaseRNN does; the
        # trainer's view of the loader's [B,F,T] batch (trainClassifier.py:299) as its base under FLAG_X_BFT, else a copy
        if route.present == _route.TRANSPOSE_COPY:
            input = input.transpose(0, 1)
        x = input.permute(1, 2, 0) if route.present == _route.BFT_BASE else input.contiguous()
        hs = _BatchNormInference.apply(cell, x, h0, route.flags, *cell._fold_tensors())
        if route.post == _route.LAST_STEP:
            return _route.last_step(hs, route.flags)
        return hs.transpose(0, 1) if route.post == _route.TRANSPOSE_BACK else hs

    @torch.no_grad()
    def forward_windows(self, pool, starts, T, hiddenState=None, last_state=False, check=True, training=False):
        """Eval-mode inference over windows of a shared frame pool (``FastGRNNCUDA.forward_windows``): utterance ``b``
        is the ``T`` consecutive rows of ``pool:[R,F]`` from row ``starts[b]`` on.  Returns what ``forward(...,
        training=False)`` returns for the gathered batch, without a graph; the pool is read in place where the windowed
        scans hold the cell (``fastgrnn_cuda.windows_supported``), gathered elsewhere."""
        if training:
            raise NotImplementedError(_TRAINING_MSG)
        cell = self.cell
        dev = cell.W.device
        if dev.type != "cuda":
            raise RuntimeError("FastGRNNBatchNorm.forward_windows runs on the GPU only (parameters are on %s)" % dev)
        pool, starts = pool.to(dev), starts.to(dev)
        if pool.dtype != cell.W.dtype:
            raise RuntimeError("pool dtype %s differs from the parameters' %s" % (pool.dtype, cell.W.dtype))
        B, H, T = starts.numel(), cell._hidden_size, int(T)
        h0 = _route.zero_state(B, H, pool.dtype, dev) if hiddenState is None else \
            hiddenState.to(dev).reshape(B, H).contiguous()
        bm = self.batch_first is True
        flags = (_lib.FLAG_BATCH_MAJOR if bm else 0) | (_lib.FLAG_HS_LAST if last_state else 0) | _lib.FLAG_PREACT_AFFINE
        if pool.dim() == 2 and fastgrnn_cuda.windows_supported(T, B, pool.shape[1], H, 0, 0, cell._gate_code,
                                                               cell._update_code, pool.dtype, flags):
            w, u, bg, bu, sg, sc = cell._folded()
            return fastgrnn_cuda.forward_windows(pool.contiguous(), starts, T, w, u, bg, bu, cell.zeta, cell.nu, h0,
                                                 cell._gate_code, sg, sc, batch_major=bm, last_state=last_state,
                                                 update_non_linearity=cell._update_code, check=check)
        return FastGRNNBatchNorm.forward(self, gather_windows(pool, starts, T, check, bm), hiddenState=h0,
                                         training=False, last_state=last_state)
