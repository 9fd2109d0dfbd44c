"""``optimizer.step()`` and the IHT phase of a trainer iteration (trainClassifier.py:249-259) in one library call.

``FusedAdam`` / ``FusedSGD`` are ``torch.optim.Optimizer`` subclasses with torch's constructor arguments, ``param_groups``
keys and ``state_dict`` layout whose ``step()`` hands EVERY parameter of the model to ``fastgrnn_hip_train_update``: one
kernel launch per 32 parameter tensors applies the update and, on the W/U matrices registered with ``register_iht``,
the hard threshold (``utils.hardThreshold``) or the support mask (``utils.supportBasedThreshold``).  The learning rate,
the step count and the IHT phase are read from device scalars (``lr_t``, ``step_t``, ``iht_t``), so a step captured in a
HIP graph serves a whole training run: the caller rewrites the scalars between replays, or a ``kws_amd.TrainSchedule``
computes the learning rate (the reference's five schedules) and the phase on the device from ``step_t``, inside the graph.

Limits, each refused with a message that names it: one param group; float32, dense, contiguous parameters on one
device; ``amsgrad``, ``maximize``, ``differentiable`` and decoupled weight decay (AdamW) off; at most 2^22 elements per
tensor.  Constructing an optimizer and moving its state need no GPU -- ``step()`` does.  The other eight optimizers of the
reference's ``configure_optimizer`` stay with ``torch.optim``.

The library writes parameters, moments and masks through raw pointers; ``step()`` then bumps the parameters' torch
versions, so a step between a forward and its backward, or a cache keyed on ``_version``, sees it.  The segment table
handed to the library is cached and rebuilt when a parameter, gradient, state tensor or mask has been replaced.

The masks of the IHT phases belong to the optimizer (``support(param)``), not to the layers: ``sparsify()`` /
``sparsifyWithSupport()`` and their ``oldmats`` are untouched and independent.  Use one mechanism per run.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .fastgrnn_cuda import _call

IHT_MODES = {"none": _lib.IHT_NONE, "threshold": _lib.IHT_THRESHOLD, "support": _lib.IHT_SUPPORT}


def keep_rank(n, s):
    """The 0-based rank, among ``n`` ascending magnitudes, of the threshold that keeps (about) a fraction ``s``:
    ``ceil((1-s)(n-1))`` in double, clamped to ``0..n-1`` -- numpy's ``percentile(..., (1-s)*100, 'higher')`` index,
    computed as ``utils.hardThreshold`` does."""
    pos = (1.0 - float(s)) * (n - 1)
    return min(max(int(math.ceil(pos - 1e-12)), 0), n - 1)


def iht_phase(epoch, num_epochs, i_batch, trim_level):
    """Which IHT phase follows ``optimizer.step()`` in iteration ``i_batch`` of ``epoch`` when the trainer sparsifies
    (trainClassifier.py:251-259): ``"none"`` in the first third of training, in the middle third ``"threshold"`` every
    ``trim_level`` batches and ``"support"`` between them, ``"support"`` in the last third."""
    if epoch >= num_epochs / 3:
        if epoch < (2 * num_epochs) / 3:
            return "threshold" if i_batch % trim_level == 0 else "support"
        return "support"
    return "none"


class _FusedOptimizer(torch.optim.Optimizer):
    _ALGO = None
    _STATE_KEYS = ()                                  # the tensors of a parameter's state, in state0, state1 order

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("%s takes one param group (got %d)" % (type(self).__name__, len(self.param_groups)))
        ps = self.param_groups[0]["params"]
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.is_sparse:
                raise ValueError("%s updates dense float32 parameters only (got %s)" % (type(self).__name__, p.dtype))
            if p.device != dev:
                raise ValueError("%s needs every parameter on one device (got %s and %s)"
                                 % (type(self).__name__, dev, p.device))
            if not p.is_contiguous():
                raise ValueError("%s needs contiguous parameters" % type(self).__name__)
            if not 1 <= p.numel() <= _lib.UPDATE_MAX_N:
                raise ValueError("%s takes tensors of 1 to 2^22 elements (got %d)" % (type(self).__name__, p.numel()))
        self._check_group()
        self._device = dev
        # the device scalars of the library call (on the parameters' device, wherever that is)
        self.lr_t = torch.full((1,), float(self.param_groups[0]["lr"]), dtype=torch.float32, device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.iht_t = torch.zeros(1, dtype=torch.int32, device=dev)
        self._lr_filled = float(self.param_groups[0]["lr"])
        self._iht_filled = 0
        self._iht = {}                                # parameter -> (keep_rank, support mask)
        self._table = None                            # (key, ctypes segment array, n): rebuilt when an address moves

    # ---- what the subclasses say ----------------------------------------------------------------------------------
    def _check_group(self):
        raise NotImplementedError

    def _hyper(self, group):
        raise NotImplementedError

    # ---- IHT --------------------------------------------------------------------------------------------------------
    def register_iht(self, model_or_layer):
        """Mark the W/U matrices (or their factors) of a layer, or of every layer in a model's ``rnn_list``, for the IHT
        phases: ``getVars()[:num_W + num_U]`` with the layer's ``_wSparsity`` / ``_uSparsity``, as ``sparsify()`` picks
        them.  Allocates each matrix's support mask (all ones: until a ``"threshold"`` step has run, ``"support"``
        masks nothing).  Returns the number of matrices registered."""
        layers = list(model_or_layer.rnn_list) if hasattr(model_or_layer, "rnn_list") else [model_or_layer]
        mine = set(self.param_groups[0]["params"])
        count = 0
        for layer in layers:
            if not hasattr(layer, "_num_W_matrices") and hasattr(layer, "cell"):
                layer = layer.cell                    # the BatchNorm layers keep the matrices on their cell
            mats = layer.getVars()
            end_w = layer._num_W_matrices
            end_u = end_w + layer._num_U_matrices
            for i in range(end_u):
                p = mats[i]
                if p not in mine:
                    raise ValueError("register_iht: a W/U matrix of the layer is not a parameter of this optimizer")
                s = layer._wSparsity if i < end_w else layer._uSparsity
                self._iht[p] = (keep_rank(p.numel(), s),
                                torch.ones(p.numel(), dtype=torch.uint8, device=p.device))
                count += 1
        self._table = None
        return count

    def support(self, param):
        """The support mask of a registered matrix: uint8, the parameter's shape, 1 where the last ``"threshold"`` step
        left a non-zero."""
        return self._iht[param][1].view(param.shape)

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _init_state(self, p):
        st = self.state[p]
        for k in self._STATE_KEYS:
            if st.get(k) is None:
                st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _segments(self):
        """The C segment table for the parameters that have a gradient, rebuilt whenever anything it points at has moved:
        a parameter's or gradient's address, or the identity of a state tensor or a mask (the table keeps those tensors
        referenced, so an identity is never recycled while the table lives).  Gradients are checked on every call."""
        ps = [p for p in self.param_groups[0]["params"] if p.grad is not None]
        key = []
        for p in ps:
            g, st = p.grad, self.state.get(p) or self._init_state(p)
            if g.dtype is not torch.float32 or g.is_sparse or g.device != p.device or not g.is_contiguous():
                raise RuntimeError("%s: gradients must be dense contiguous float32 tensors on the parameter's device"
                                   % type(self).__name__)
            key.append((p.data_ptr(), g.data_ptr()) + tuple(id(st.get(k)) for k in self._STATE_KEYS)
                       + (id(self._iht[p][1]) if p in self._iht else 0,))
        if self._table is not None and self._table[0] == key:
            return self._table[1], self._table[2]
        segs = (_lib.UpdateSeg * max(1, len(ps)))()
        held = []
        for sg, p in zip(segs, ps):
            st = self._init_state(p)
            sg.param, sg.grad, sg.n = p.data_ptr(), p.grad.data_ptr(), p.numel()
            sg.state0 = st[self._STATE_KEYS[0]].data_ptr()
            sg.state1 = st[self._STATE_KEYS[1]].data_ptr() if len(self._STATE_KEYS) > 1 else None
            held.extend(st[k] for k in self._STATE_KEYS)
            if p in self._iht:
                sg.keep_rank, mask = self._iht[p]
                sg.support, sg.iht = mask.data_ptr(), 1
                held.append(mask)
        # (a state tensor created just now changes the key the next call computes: one more rebuild, then hits)
        self._table = (key, segs, len(ps), held, ps)
        return segs, len(ps)

    def add_param_group(self, param_group):
        if getattr(self, "param_groups", None):
            raise ValueError("%s takes one param group: add_param_group() after construction is not supported"
                             % type(self).__name__)
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, iht="none", closure=None):
        """One update of every parameter that has a gradient, then the IHT phase ``iht`` on the registered matrices:
        ``"none"``, ``"threshold"``, ``"support"``, or ``None`` to leave ``iht_t`` as the caller wrote it.  Copies
        ``param_groups[0]['lr']`` into ``lr_t`` (not with ``capturable=True``: the caller writes ``lr_t``), adds one to
        ``step_t`` on the device and makes one library call."""
        if callable(iht):                                    # torch's positional step(closure)
            iht, closure = "none", iht
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._device.type != "cuda":
            raise RuntimeError("%s.step() runs on the GPU (parameters are on %s); kws_amd has no CPU fallback"
                               % (type(self).__name__, self._device))
        group = self.param_groups[0]
        self._check_group()
        if iht is None:
            self._iht_filled = None                          # (the caller owns iht_t now)
        else:
            if iht not in IHT_MODES:
                raise ValueError("iht must be 'none', 'threshold', 'support' or None (got %r)" % (iht,))
            if IHT_MODES[iht] != self._iht_filled:
                self._iht_filled = IHT_MODES[iht]
                self.iht_t.fill_(self._iht_filled)
        if group["capturable"]:
            self._lr_filled = None
        elif float(group["lr"]) != self._lr_filled:
            self._lr_filled = float(group["lr"])
            self.lr_t.fill_(self._lr_filled)
        segs, n = self._segments()
        if n == 0:
            return loss
        self.step_t.add_(1)
        hy = self._hyper(group)
        with torch.cuda.device(self._device):
            _call(_lib.load().fastgrnn_hip_train_update, "fastgrnn train_update", None, self._device, None,
                  C.byref(hy), segs, n, self.lr_t.data_ptr(), self.step_t.data_ptr(), self.iht_t.data_ptr())
        # the library wrote through raw pointers: tell torch, so that whatever is keyed on a tensor's version (autograd's
        # saved-tensor check, the eval-mode BatchNorm fold cache) sees the step
        torch.autograd.graph.increment_version(self._table[4])
        return loss

    # ---- checkpoints: torch's layout, plus the masks under a key torch ignores ---------------------------------------
    def _export_step(self, t):
        pass

    def _import_step(self, sd):
        raise NotImplementedError

    def state_dict(self):
        self._export_step(int(self.step_t.item()))
        sd = super().state_dict()
        order = {p: i for i, p in enumerate(self.param_groups[0]["params"])}
        sd["iht_support"] = {order[p]: mask.clone() for p, (_, mask) in self._iht.items()}
        sd["fused_step"] = int(self.step_t.item())
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("%s takes one param group" % type(self).__name__)
        self._check_group()
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if st:
                for k in self._STATE_KEYS:
                    if st.get(k) is not None:
                        st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        self.step_t.fill_(self._import_step(state_dict))
        ps = self.param_groups[0]["params"]
        for i, mask in (state_dict.get("iht_support") or {}).items():
            p = ps[int(i)]
            if p not in self._iht:
                raise ValueError("load_state_dict: a support mask for a matrix that register_iht has not marked")
            self._iht[p][1].copy_(mask.reshape(-1))
        self._lr_filled = self._iht_filled = None
        self.lr_t.fill_(float(self.param_groups[0]["lr"]))
        self._lr_filled = float(self.param_groups[0]["lr"])
        self._table = None


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` (L2 weight decay, no amsgrad) on ``fastgrnn_hip_train_update``."""
    _ALGO = _lib.ADAM
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize, foreach=foreach, capturable=capturable,
                                      differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _check_group(self):
        g = self.param_groups[0]
        g.setdefault("capturable", False)
        for k in ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay"):
            if g.get(k):
                raise ValueError("FusedAdam does not implement %s=True" % k)
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError("FusedAdam takes a float lr (the device scalar is lr_t)")
        b1, b2 = g["betas"]
        if not (float(g["lr"]) >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] > 0.0
                and g["weight_decay"] >= 0.0):
            raise ValueError("FusedAdam: lr >= 0, betas in [0,1), eps > 0, weight_decay >= 0 (got %r, %r, %r, %r)"
                             % (g["lr"], g["betas"], g["eps"], g["weight_decay"]))

    def _hyper(self, g):
        return _lib.UpdateHyper(_lib.ADAM, 0, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                float(g["weight_decay"]))

    def _export_step(self, t):
        for p in self.param_groups[0]["params"]:
            if p in self.state and self.state[p]:
                self.state[p]["step"] = torch.tensor(float(t))          # torch's: a float32 scalar on the host

    def _import_step(self, sd):
        steps = {int(float(st["step"])) for st in self.state.values() if st and "step" in st}
        if len(steps) > 1:
            raise ValueError("FusedAdam keeps one step count for all parameters (the checkpoint has %s)" % sorted(steps))
        return steps.pop() if steps else 0


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` (momentum, dampening, nesterov, L2 weight decay) on ``fastgrnn_hip_train_update``."""
    _ALGO = _lib.SGD
    _STATE_KEYS = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, capturable=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, foreach=foreach,
                                      differentiable=differentiable, fused=fused, capturable=capturable))

    def _check_group(self):
        g = self.param_groups[0]
        g.setdefault("capturable", False)
        for k in ("maximize", "differentiable"):
            if g.get(k):
                raise ValueError("FusedSGD does not implement %s=True" % k)
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError("FusedSGD takes a float lr (the device scalar is lr_t)")
        if not (float(g["lr"]) >= 0.0 and 0.0 <= g["momentum"] < 1.0 and g["weight_decay"] >= 0.0):
            raise ValueError("FusedSGD: lr >= 0, momentum in [0,1), weight_decay >= 0 (got %r, %r, %r)"
                             % (g["lr"], g["momentum"], g["weight_decay"]))
        if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")      # torch's own rule

    def _hyper(self, g):
        return _lib.UpdateHyper(_lib.SGD, 1 if g["nesterov"] else 0, float(g["momentum"]), float(g["dampening"]), 0.0,
                                float(g["weight_decay"]))

    def _import_step(self, sd):
        if "fused_step" in sd:
            return int(sd["fused_step"])
        # torch.optim.SGD keeps no count: a buffer means the first step (b = g) is behind us
        have = [st.get("momentum_buffer") is not None for st in self.state.values() if st]
        if any(have) and not all(have):
            raise ValueError("FusedSGD keeps one step count for all parameters (some have a momentum buffer, some none)")
        return 1 if any(have) else 0
