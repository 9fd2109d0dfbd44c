"""Training-mode FastGRNN with BatchNorm on the GPU: ``FastGRNNBatchNormCUDA``, the name the reference reserves for it
(/root/reference trainClassifier.py:344-346, ``#todo: add FastGRNNBatchNormCUDA``).

Same parameters, buffers and checkpoint keys as ``FastGRNNBatchNorm`` (it is a subclass), so a model trained with
one class is evaluated or served by the other.  ``forward(input, hiddenState=None, training=True, last_state=False)``:

* ``training=True`` runs the reference cell (rnn.py:373-414) with every ``BatchNorm1d`` in training mode: per frame,
  batch mean and biased batch variance over the B utterances; each of the four layers' running statistics is updated
  once per frame, T times per call in frame order, and ``num_batches_tracked`` grows by T.  On the shapes
  ``fastgrnn_hip_bn_train_supported`` admits (fp32, H = 128 with F = 32/64/128/256, H = 256 with F = 32/64/128,
  gate sigmoid / relu / tanh) this is an autograd function over ``fastgrnn_hip_bn_train_forward`` / ``_backward``
  (include/fastgrnn_hip.h, FASTGRNN_FLAG_BN_TRAIN): gradients for W, U, bias_gate, bias_update, zeta, nu, the eight
  BatchNorm affine parameters, the input and the initial state.  Every other case (other shapes, fp64, BatchNorm
  layers not in training mode or without affine parameters / running statistics) runs the reference formula per
  frame in torch ops on the GPU -- slow and correct, warned once.
* ``training=False`` is ``FastGRNNBatchNorm.forward``: the eval-mode cell folded into the fused scans.

``B == 1`` raises ``ValueError`` in training mode, as torch's BatchNorm does.
"""
from __future__ import annotations

import ctypes as C
import warnings

import torch
from torch.autograd import Function

from . import _lib, _route
from .batchnorm import FastGRNNBatchNorm
from .fastgrnn_cuda import _call, _params, _pool_plan, _ptr

_warned = set()


def _bn_layer(bn, forward):
    mom = -1.0 if bn.momentum is None else float(bn.momentum)
    return _lib.BnLayer(_ptr(bn.weight), _ptr(bn.bias), _ptr(bn.running_mean) if forward else None,
                        _ptr(bn.running_var) if forward else None,
                        _ptr(bn.num_batches_tracked) if forward else None, float(bn.eps), mom)


def _bn_struct(cell, forward=True):
    return _lib.BnParams(*(_bn_layer(bn, forward) for bn in (cell.bn_w, cell.bn_u, cell.bn_gate, cell.bn_update)))


def _plan(T, B, F, H, gate_code, batch_major):
    """The cached descriptor of a training step with what the library answers for it (fastgrnn_cuda._pool_plan)."""
    flags = _lib.FLAG_BN_TRAIN | (_lib.FLAG_BATCH_MAJOR if batch_major else 0)
    return _pool_plan((T, B, F, H, 0, 0, int(gate_code), 2, _lib.F32, flags), "bn_train")


def bn_train_supported(T, B, F, H, gate_code=0, dtype=torch.float32, batch_major=False):
    """True where the training step runs on the fused kernels (fastgrnn_hip_bn_train_supported)."""
    if dtype != torch.float32:
        return False
    return _plan(T, B, F, H, gate_code, batch_major).supported


class _BatchNormTrain(Function):
    """Forward: the training-mode scan (updates the running statistics).  Backward: every gradient."""

    @staticmethod
    def forward(ctx, cell, x, h0, batch_major, W, U, bias_gate, bias_update, zeta, nu, gw, bw, gu, bu, gg, bg, gc, bc):
        lib = _lib.load()
        T, B, F = _route.seq_dims(x.shape, batch_major)
        H = cell._hidden_size
        plan = _plan(T, B, F, H, cell._gate_code, batch_major)
        dev = x.device
        w = W.detach().t().contiguous()
        u = U.detach().t().contiguous()
        bgate, bupd = bias_gate.detach().contiguous(), bias_update.detach().contiguous()
        params = _params(False, False, w, u, None, None, None, None, bgate, bupd, zeta, nu)
        bnp = _bn_struct(cell, True)
        with torch.cuda.device(dev):
            hs = torch.empty(tuple(x.shape[:2]) + (H,), dtype=x.dtype, device=dev)
            saved = torch.empty(T, B, H, dtype=torch.float32, device=dev)
            stats = torch.empty(T, 9 * H, dtype=torch.float64, device=dev)
            _call(lib.fastgrnn_hip_bn_train_forward, "fastgrnn_hip_bn_train_forward", None, dev, plan.ws_forward,
                  C.byref(plan.desc), C.byref(params), C.byref(bnp), _ptr(x), _ptr(h0), _ptr(hs), _ptr(saved),
                  _ptr(stats))
            with torch.no_grad():
                for bn in (cell.bn_w, cell.bn_u, cell.bn_gate, cell.bn_update):
                    bn.num_batches_tracked.add_(T)
        ctx.cell, ctx.desc_args = cell, (T, B, F, H, cell._gate_code, batch_major)
        ctx.eps_mom = [(bn.eps, bn.momentum) for bn in (cell.bn_w, cell.bn_u, cell.bn_gate, cell.bn_update)]
        ctx.save_for_backward(x, h0, hs, saved, stats, w, u, bgate, bupd, zeta, nu, gw, bw, gu, bu, gg, bg, gc, bc)
        return hs

    @staticmethod
    def backward(ctx, grad_hs):
        lib = _lib.load()
        x, h0, hs, saved, stats, w, u, bgate, bupd, zeta, nu, gw, bw, gu, bu, gg, bg, gc, bc = ctx.saved_tensors
        T, B, F, H, gate_code, batch_major = ctx.desc_args
        plan = _plan(T, B, F, H, gate_code, batch_major)
        dev = x.device
        grad_hs = grad_hs.contiguous()
        params = _params(False, False, w, u, None, None, None, None, bgate, bupd, zeta, nu)
        layers = []
        for (g_, b_), (eps, mom) in zip(((gw, bw), (gu, bu), (gg, bg), (gc, bc)), ctx.eps_mom):
            layers.append(_lib.BnLayer(_ptr(g_), _ptr(b_), None, None, None, float(eps),
                                       -1.0 if mom is None else float(mom)))
        bnp = _lib.BnParams(*layers)
        with torch.cuda.device(dev):
            e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
            d_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            d_h0, d_w, d_u = e(B, H), e(H, F), e(H, H)
            d_bg, d_bu, d_zeta, d_nu = e(1, H), e(1, H), e(1, 1), e(1, 1)
            dbn = [e(H) for _ in range(8)]
            grads = _lib.Grads(_ptr(d_x), _ptr(d_bg), _ptr(d_bu), _ptr(d_zeta), _ptr(d_nu), _ptr(d_h0), _ptr(d_w),
                               _ptr(d_u), None, None, None, None)
            bgr = _lib.BnGrads(*(_ptr(t) for t in dbn))
            _call(lib.fastgrnn_hip_bn_train_backward, "fastgrnn_hip_bn_train_backward", None, dev, plan.ws_backward,
                  C.byref(plan.desc), C.byref(params), C.byref(bnp), _ptr(grad_hs), _ptr(x), _ptr(hs), _ptr(saved),
                  _ptr(stats), _ptr(h0), C.byref(grads), C.byref(bgr))
        return (None, d_x, d_h0, None, d_w.t(), d_u.t(), d_bg.reshape(bgate.shape), d_bu.reshape(bupd.shape),
                d_zeta.reshape(zeta.shape), d_nu.reshape(nu.shape), *dbn)


class FastGRNNBatchNormCUDA(FastGRNNBatchNorm):
    """The BatchNorm FastGRNN trained on the GPU (module docstring).  Constructor, parameters and state dict are
    ``FastGRNNBatchNorm``'s."""

    def _fused(self, x, batch_major, B):
        cell = self.cell
        bns = (cell.bn_w, cell.bn_u, cell.bn_gate, cell.bn_update)
        if not all(bn.training and bn.affine and bn.track_running_stats for bn in bns):
            return False
        T, _, F = _route.seq_dims(x.shape, batch_major)
        return bn_train_supported(T, B, F, cell._hidden_size, cell._gate_code, x.dtype, batch_major) and \
            cell.W.dtype == torch.float32

    def forward(self, input, hiddenState=None, training=True, last_state=False):
        """input [T,B,F] (``[B,T,F]`` with ``batch_first``) -> every hidden state in the input's layout, or with
        ``last_state=True`` the final state ``[B,H]``."""
        if not training:
            # The fused training forward writes the running statistics in the kernel (their _version does not move,
            # nor does anything under a graph replay), so the eval-mode fold of FastGRNNBatchNorm cannot tell from
            # its cache key that they changed: fold again on every eval call.
            self.cell._fold_key = None
            return super().forward(input, hiddenState=hiddenState, training=False, last_state=last_state)
        cell = self.cell
        dev = cell.W.device
        if dev.type != "cuda":
            raise RuntimeError("FastGRNNBatchNormCUDA.forward runs on the GPU only (parameters are on %s)" % dev)
        input = input.to(dev)
        if input.dtype != cell.W.dtype:
            raise RuntimeError("input dtype %s differs from the parameters' %s" % (input.dtype, cell.W.dtype))
        bf = self.batch_first is True
        B = input.shape[0] if bf else input.shape[1]
        if B < 2:
            raise ValueError("FastGRNNBatchNormCUDA: training-mode BatchNorm needs more than 1 utterance per batch "
                             "(got B=%d)" % B)
        H = cell._hidden_size
        h0 = _route.zero_state(B, H, input.dtype, dev) if hiddenState is None else \
            hiddenState.to(dev, input.dtype).reshape(B, H).contiguous()
        x = input.contiguous()
        if self._fused(x, bf, B):
            hs = _BatchNormTrain.apply(cell, x, h0, bf, cell.W, cell.U, cell.bias_gate, cell.bias_update, cell.zeta,
                                       cell.nu, cell.bn_w.weight, cell.bn_w.bias, cell.bn_u.weight, cell.bn_u.bias,
                                       cell.bn_gate.weight, cell.bn_gate.bias, cell.bn_update.weight,
                                       cell.bn_update.bias)
        else:
            hs = self._torch_ops(x, h0, bf)
        return _route.last_step(hs, _lib.FLAG_BATCH_MAJOR if bf else 0) if last_state else hs

    def forward_windows(self, pool, starts, T, hiddenState=None, last_state=False, check=True, training=False):
        """``FastGRNNBatchNorm.forward_windows`` (eval mode only), folding again on every call as ``forward`` does."""
        self.cell._fold_key = None
        return super().forward_windows(pool, starts, T, hiddenState=hiddenState, last_state=last_state, check=check,
                                       training=training)

    def _torch_ops(self, x, h0, bf):
        """The reference formula per frame in torch ops (rnn.py:373-414 under BaseRNN, rnn.py:588-668)."""
        cell = self.cell
        key = (tuple(x.shape), x.dtype, cell._gate_code, bf)
        if key not in _warned:
            _warned.add(key)
            warnings.warn("FastGRNNBatchNormCUDA: shape %s dtype %s gate %s is not on the fused training kernels "
                          "(fastgrnn_hip_bn_train_supported); running the reference formula per frame in torch ops"
                          % (tuple(x.shape), x.dtype, cell._gate_nonlinearity), RuntimeWarning, stacklevel=3)
        xs = x.transpose(0, 1) if bf else x
        h = h0
        out = []
        for t in range(xs.shape[0]):
            h = cell(xs[t], h, training=True)
            out.append(h)
        hs = torch.stack(out)
        return hs.transpose(0, 1) if bf else hs
