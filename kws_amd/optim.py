"""``optimizer.step()`` and the IHT phase of a trainer iteration (trainClassifier.py:249-259) in one library call.

``FusedAdam`` / ``FusedSGD`` (on ``fastgrnn_hip_train_update``) and ``FusedRMSprop`` / ``FusedAdagrad`` / ``FusedAdadelta`` /
``FusedAdamax`` / ``FusedASGD`` / ``FusedRprop`` (on ``fastgrnn_hip_optim_update``) -- the eight optimizers of the
reference's ``configure_optimizer``, which ``configure_optimizer(params, options)`` here maps to them -- are
``torch.optim.Optimizer`` subclasses with torch's constructor arguments, ``param_groups``
keys and ``state_dict`` layout whose ``step()`` hands EVERY parameter of the model to the library: one
kernel launch per 32 parameter tensors applies the update and, on the W/U matrices registered with ``register_iht``,
the hard threshold (``utils.hardThreshold``) or the support mask (``utils.supportBasedThreshold``).  The learning rate,
the step count and the IHT phase are read from device scalars (``lr_t``, ``step_t``, ``iht_t``), so a step captured in a
HIP graph serves a whole training run: the caller rewrites the scalars between replays, or a ``kws_amd.TrainSchedule``
computes the learning rate (the reference's five schedules) and the phase on the device from ``step_t``, inside the graph.

Limits, each refused with a message that names it: one param group; float32, dense, contiguous parameters on one
device; ``amsgrad``, ``maximize``, ``differentiable`` and decoupled weight decay (AdamW) off; at most 2^22 elements per
tensor.  Constructing an optimizer and moving its state need no GPU -- ``step()`` does.  ``capturable`` is accepted by
every class, also where ``torch.optim``'s has no such argument.  ``FusedRprop`` adapts a step size per element and never
reads the learning rate after its state exists: ``lr_t`` -- and a ``TrainSchedule`` that writes it -- is ignored there.

The library writes parameters, moments and masks through raw pointers; ``step()`` then bumps the parameters' torch
versions, so a step between a forward and its backward, or a cache keyed on ``_version``, sees it.  The segment table
handed to the library is cached and rebuilt when a parameter, gradient, state tensor or mask has been replaced.

``guard(max_grad_norm=None, skip_nonfinite=True)`` puts the gradient guard in front of the update, on the device and
inside the same graph: the global norm of all gradients (``fastgrnn_hip_grad_guard``: a fixed-order sum in double),
``torch.nn.utils.clip_grad_norm_``'s coefficient, and the rejection of a step whose gradient holds a NaN or an
infinity -- such a step leaves parameters and optimizer state as they are and is counted in ``skipped_t``; the rules
then count the steps actually taken (``applied_t``), while ``step_t`` goes on counting iterations.

The masks of the IHT phases belong to the optimizer (``support(param)``), not to the layers: ``sparsify()`` /
``sparsifyWithSupport()`` and their ``oldmats`` are untouched and independent.  Use one mechanism per run.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from . import _lib
from .fastgrnn_cuda import _call

IHT_MODES = {"none": _lib.IHT_NONE, "threshold": _lib.IHT_THRESHOLD, "support": _lib.IHT_SUPPORT}

# guard(): the clipping norm, the flags, the 32-byte device state (fastgrnn_guard_state) and the reduction's workspace
_Guard = collections.namedtuple("_Guard", "max_norm flags state workspace")
# _segments(): the key it was built for, the ctypes segment array and its length, the tensors it points into (kept
# alive), the parameters that had a gradient, and the guard call's view of the same gradients (None without a guard)
_Table = collections.namedtuple("_Table", "key segs n held params guard_segs")


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
    _STATE_KEYS = ()                                  # the tensors of a parameter's state, in the segment's slot order
    _SEG = _lib.UpdateSeg                             # the library's segment structure and ...
    _ENTRY = "fastgrnn_hip_train_update"              # ... the call that takes it
    _ALL_STATE_KEYS = ()                              # where _slots() depends on the settings: every key it can name
    _REFUSED = ("maximize", "differentiable")         # torch's options that must stay off

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
        self._table = None                            # a _Table: rebuilt when an address moves
        self._guard = None                            # guard(): a _Guard

    # ---- what the subclasses say ----------------------------------------------------------------------------------
    def _ranges(self, g):
        """-> (ok, what the message says must hold, the values it shows)"""
        raise NotImplementedError

    def _hyper(self, group):
        raise NotImplementedError

    def _slots(self, group):
        """(slot, key) of every state tensor the group's settings use; the other slots of a segment stay NULL"""
        return tuple(enumerate(self._STATE_KEYS))

    def _new_state(self, p, key, group):
        return torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _set_states(self, sg, ptrs):
        sg.state0, sg.state1 = ptrs.get(0), ptrs.get(1)

    def _extra_args(self):
        """what the library call takes between ``iht_mode`` and the stream"""
        return ()

    def _check_group(self):
        g, name = self.param_groups[0], type(self).__name__
        g.setdefault("capturable", False)
        for k in self._REFUSED:
            if g.get(k):
                raise ValueError("%s does not implement %s=True" % (name, k))
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError("%s takes a float lr (the device scalar is lr_t)" % name)
        ok, rule, got = self._ranges(g)
        if not (float(g["lr"]) >= 0.0 and ok):
            raise ValueError("%s: lr >= 0, %s (got %r, %s)" % (name, rule, g["lr"], ", ".join("%r" % (v,) for v in got)))

    # ---- the gradient guard -----------------------------------------------------------------------------------------
    def guard(self, max_grad_norm=None, skip_nonfinite=True):
        """Put the gradient guard in front of every ``step()``: with ``max_grad_norm`` the gradients are scaled by
        ``min(1, max_grad_norm / (norm + 1e-6))`` (``clip_grad_norm_``'s rule, the 2-norm over all parameters; the
        ``.grad`` tensors themselves are not written), with ``skip_nonfinite`` a step whose gradient holds a NaN or an
        infinity is rejected: parameters, optimizer state and ``applied_t`` stay as they are, ``skipped_t`` counts it
        and the IHT phase still runs.  Call it once, before the first ``step()``; returns ``self``.

        Allocates the 32-byte device state and the workspace, and exposes the state as ``grad_norm_t``,
        ``clip_coef_t`` (float32), ``skip_t`` (int32: the last step's decision), ``applied_t`` and ``skipped_t``
        (int64) -- views, written by every step on the device.  Under a guard the rules take ``applied_t`` for their
        step count (bias corrections and the like); ``step_t`` still counts iterations, which is what a
        ``TrainSchedule`` reads."""
        name = type(self).__name__
        if self._guard is not None:
            raise RuntimeError("%s.guard() may be called once" % name)
        if int(self.step_t.item()) != 0:
            raise RuntimeError("%s.guard() must come before the first step() (step_t is %d)"
                               % (name, int(self.step_t.item())))
        if max_grad_norm is None and not skip_nonfinite:
            raise ValueError("%s.guard(): give max_grad_norm, or leave skip_nonfinite on -- with both off there is "
                             "nothing to guard" % name)
        max_norm = math.inf if max_grad_norm is None else float(max_grad_norm)
        if not max_norm > 0.0:                               # (a NaN fails the comparison)
            raise ValueError("%s.guard(): max_grad_norm must be > 0 (got %r)" % (name, max_grad_norm))
        state = torch.zeros(4, dtype=torch.int64, device=self._device)          # fastgrnn_guard_state
        n = len(self.param_groups[0]["params"])
        ws = torch.zeros(((8 * n + 255) // 256 * 256) // 8, dtype=torch.float64, device=self._device)
        self._guard = _Guard(max_norm, _lib.GUARD_SKIP_NONFINITE if skip_nonfinite else 0, state, ws)
        f32, i32 = state.view(torch.float32), state.view(torch.int32)
        self.grad_norm_t, self.clip_coef_t, self.skip_t = f32[0:1], f32[1:2], i32[2:3]
        self.applied_t, self.skipped_t = state[2:3], state[3:4]
        self._table = None
        return self

    @property
    def guarded(self):
        return self._guard is not None

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

    # ---- what a step carries over to the next (kws_amd.graph.RunSnapshot) ------------------------------------------
    def _state_tensors(self):
        """(parameter, key, tensor) of every state tensor the rule reads that exists so far"""
        keys = [k for _, k in self._slots(self.param_groups[0])]
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p) or {}
            for k in keys:
                if st.get(k) is not None:
                    yield p, k, st[k]

    def run_tensors(self):
        """The tensors from which a step reads what an earlier step wrote: the step count, the support masks, the
        guard's state and the rule's state tensors as far as they exist.  ``lr_t`` and ``iht_t`` are not among them:
        ``step()`` keeps host mirrors of both (``_lr_filled``, ``_iht_filled``) that a copy into the device side
        alone would leave stale, and whoever drives a captured step -- the caller, or a ``TrainSchedule`` -- rewrites
        both before every step anyway.  (The ``step`` / ``eta`` / ``mu`` entries that ``state_dict()`` leaves in
        ``state`` are exports for torch's layout; no step reads them.)"""
        held = [self.step_t] + [mask for _, mask in self._iht.values()]
        if self._guard is not None:
            held.append(self._guard.state)
        return held + [t for _, _, t in self._state_tensors()]

    def run_reset(self, held_ids):
        """State tensors that are not in the snapshot were created after it: back to what they are created with."""
        group = self.param_groups[0]
        for p, key, t in self._state_tensors():
            if id(t) not in held_ids:
                t.copy_(self._new_state(p, key, group))

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _init_state(self, p):
        st = self.state[p]
        group = self.param_groups[0]
        for _, k in self._slots(group):
            if st.get(k) is None:
                st[k] = self._new_state(p, k, group)
        return st

    def _segments(self):
        """The C segment table for the parameters that have a gradient, rebuilt whenever anything it points at has moved:
        a parameter's or gradient's address, or the identity of a state tensor or a mask (the table keeps those tensors
        referenced, so an identity is never recycled while the table lives).  Gradients are checked on every call."""
        ps = [p for p in self.param_groups[0]["params"] if p.grad is not None]
        slots = self._slots(self.param_groups[0])
        key = []
        for p in ps:
            g, st = p.grad, self.state.get(p) or self._init_state(p)
            if g.dtype is not torch.float32 or g.is_sparse or g.device != p.device or not g.is_contiguous():
                raise RuntimeError("%s: gradients must be dense contiguous float32 tensors on the parameter's device"
                                   % type(self).__name__)
            key.append((p.data_ptr(), g.data_ptr()) + tuple(id(st.get(k)) for _, k in slots)
                       + (id(self._iht[p][1]) if p in self._iht else 0,))
        if self._table is not None and self._table.key == key:
            return self._table.segs, self._table.n
        segs = (self._SEG * max(1, len(ps)))()
        held = []
        for sg, p in zip(segs, ps):
            st = self._init_state(p)
            sg.param, sg.grad, sg.n = p.data_ptr(), p.grad.data_ptr(), p.numel()
            self._set_states(sg, {slot: st[k].data_ptr() for slot, k in slots})
            held.extend(st[k] for _, k in slots)
            if p in self._iht:
                sg.keep_rank, mask = self._iht[p]
                sg.support, sg.iht = mask.data_ptr(), 1
                held.append(mask)
        gsegs = None
        if self._guard is not None:                           # the same gradients, as the guard call takes them
            gsegs = (_lib.GuardSeg * max(1, len(ps)))()
            for gs, p in zip(gsegs, ps):
                gs.grad, gs.n = p.grad.data_ptr(), p.numel()
        # (a state tensor created just now changes the key the next call computes: one more rebuild, then hits)
        self._table = _Table(key, segs, len(ps), held, ps, gsegs)
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
        ``step_t`` on the device and makes one library call -- two after ``guard()``: the guard, then the update under
        it."""
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
        entry, count = self._ENTRY, self.step_t
        with torch.cuda.device(self._device):
            if self._guard is not None:
                gd, count = self._guard, self._guard.state
                _call(_lib.load().fastgrnn_hip_grad_guard, "fastgrnn grad_guard", None, self._device, None,
                      self._table.guard_segs, n, C.c_double(gd.max_norm), gd.flags, count.data_ptr(),
                      gd.workspace.data_ptr(), gd.workspace.numel() * 8)
                entry += "_guarded"
            _call(getattr(_lib.load(), entry), entry.replace("fastgrnn_hip_", "fastgrnn "), None,
                  self._device, None, C.byref(hy), segs, n, self.lr_t.data_ptr(), count.data_ptr(),
                  self.iht_t.data_ptr(), *self._extra_args())
        # the library wrote through raw pointers: tell torch, so that whatever is keyed on a tensor's version (autograd's
        # saved-tensor check, the eval-mode BatchNorm fold cache) sees the step
        torch.autograd.graph.increment_version(self._table.params)
        return loss

    # ---- checkpoints: torch's layout, plus the masks under a key torch ignores ---------------------------------------
    def _export_step(self, t):
        for p in self.param_groups[0]["params"]:
            if p in self.state and self.state[p]:
                self.state[p]["step"] = torch.tensor(float(t))          # torch's: a float32 scalar on the host

    def _import_step(self, sd):
        steps = {int(float(st["step"])) for st in self.state.values() if st and "step" in st}
        if len(steps) > 1:
            raise ValueError("%s keeps one step count for all parameters (the checkpoint has %s)"
                             % (type(self).__name__, sorted(steps)))
        return steps.pop() if steps else 0

    def _rule_step(self):
        """the step count the rules see: the steps taken under a guard, else the iterations"""
        return int((self.applied_t if self._guard is not None else self.step_t).item())

    def state_dict(self):
        self._export_step(self._rule_step())
        sd = super().state_dict()
        order = {p: i for i, p in enumerate(self.param_groups[0]["params"])}
        sd["iht_support"] = {order[p]: mask.clone() for p, (_, mask) in self._iht.items()}
        sd["fused_step"] = int(self.step_t.item())
        if self._guard is not None:
            sd["guard"] = {"applied": int(self.applied_t.item()), "skipped": int(self.skipped_t.item())}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("%s takes one param group" % type(self).__name__)
        self._check_group()
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if st:
                for k in self._ALL_STATE_KEYS or self._STATE_KEYS:
                    if st.get(k) is not None:
                        st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
        t = self._import_step(state_dict)
        if self._guard is None:
            self.step_t.fill_(t)
        else:
            # the rules' count is `applied` (what the per-parameter `step` of a guarded checkpoint holds, and all a
            # torch.optim checkpoint has); the iterations are a guarded checkpoint's fused_step
            g = state_dict.get("guard") or {}
            applied = int(g.get("applied", t))
            skipped = int(g.get("skipped", 0))
            self._guard.state.zero_()
            self.applied_t.fill_(applied)
            self.skipped_t.fill_(skipped)
            self.step_t.fill_(int(state_dict["fused_step"]) if "guard" in state_dict and "fused_step" in state_dict
                              else applied + skipped)
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
    _REFUSED = ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize, foreach=foreach, capturable=capturable,
                                      differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _ranges(self, g):
        b1, b2 = g["betas"]
        return (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] > 0.0 and g["weight_decay"] >= 0.0,
                "betas in [0,1), eps > 0, weight_decay >= 0", (g["betas"], g["eps"], g["weight_decay"]))

    def _hyper(self, g):
        return _lib.UpdateHyper(_lib.ADAM, 0, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                float(g["weight_decay"]))


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD`` (momentum, dampening, nesterov, L2 weight decay) on ``fastgrnn_hip_train_update``."""
    _ALGO = _lib.SGD
    _STATE_KEYS = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, capturable=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, foreach=foreach,
                                      differentiable=differentiable, fused=fused, capturable=capturable))

    def _ranges(self, g):
        return (0.0 <= g["momentum"] < 1.0 and g["weight_decay"] >= 0.0, "momentum in [0,1), weight_decay >= 0",
                (g["momentum"], g["weight_decay"]))

    def _check_group(self):
        super()._check_group()
        g = self.param_groups[0]
        if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")      # torch's own rule

    def _hyper(self, g):
        return _lib.UpdateHyper(_lib.SGD, 1 if g["nesterov"] else 0, float(g["momentum"]), float(g["dampening"]), 0.0,
                                float(g["weight_decay"]))

    def _export_step(self, t):                               # torch.optim.SGD keeps no count ...
        pass

    def _import_step(self, sd):                              # ... so its checkpoints come without one
        if "fused_step" in sd:
            return int(sd["fused_step"])
        # torch.optim.SGD keeps no count: a buffer means the first step (b = g) is behind us
        have = [st.get("momentum_buffer") is not None for st in self.state.values() if st]
        if any(have) and not all(have):
            raise ValueError("FusedSGD keeps one step count for all parameters (some have a momentum buffer, some none)")
        return 1 if any(have) else 0


class _FusedOptim(_FusedOptimizer):
    """What the six rules of ``fastgrnn_hip_optim_update`` share: its segment structure and its ``scalars`` argument."""
    _SEG = _lib.OptimSeg
    _ENTRY = "fastgrnn_hip_optim_update"

    def _set_states(self, sg, ptrs):
        for slot, ptr in ptrs.items():
            sg.state[slot] = ptr

    def _extra_args(self):
        return (None,)                                       # scalars: ASGD's alone


class FusedRMSprop(_FusedOptim):
    """``torch.optim.RMSprop`` (momentum, centered, L2 weight decay) on ``fastgrnn_hip_optim_update``."""
    _ALGO = _lib.RMSPROP
    _ALL_STATE_KEYS = ("square_avg", "momentum_buffer", "grad_avg")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False,
                 capturable=False, foreach=None, maximize=False, differentiable=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered,
                                      weight_decay=weight_decay, capturable=capturable, foreach=foreach,
                                      maximize=maximize, differentiable=differentiable))

    def _ranges(self, g):
        g.setdefault("momentum", 0)
        g.setdefault("centered", False)
        return (g["alpha"] >= 0.0 and g["eps"] > 0.0 and g["momentum"] >= 0.0 and g["weight_decay"] >= 0.0,
                "alpha >= 0, eps > 0, momentum >= 0, weight_decay >= 0",
                (g["alpha"], g["eps"], g["momentum"], g["weight_decay"]))

    def _slots(self, g):                                     # torch creates the two optional buffers only where used
        return ((0, "square_avg"),) + (((1, "momentum_buffer"),) if g["momentum"] > 0 else ()) \
            + (((2, "grad_avg"),) if g["centered"] else ())

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.RMSPROP, _lib.RMSPROP_CENTERED if g["centered"] else 0,
                               (float(g["alpha"]), float(g["eps"]), float(g["momentum"])), float(g["weight_decay"]))


class FusedAdagrad(_FusedOptim):
    """``torch.optim.Adagrad`` (lr_decay, L2 weight decay, dense gradients) on ``fastgrnn_hip_optim_update``.  As
    torch's, it creates its state -- ``sum``, filled with ``initial_accumulator_value`` -- when it is constructed."""
    _ALGO = _lib.ADAGRAD
    _STATE_KEYS = ("sum",)

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10,
                 foreach=None, *, maximize=False, differentiable=False, fused=None, capturable=False):
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                                      initial_accumulator_value=initial_accumulator_value, foreach=foreach,
                                      maximize=maximize, differentiable=differentiable, fused=fused,
                                      capturable=capturable))
        for p in self.param_groups[0]["params"]:
            self._init_state(p)
            self.state[p]["step"] = torch.tensor(0.0)

    def _ranges(self, g):
        return (g["lr_decay"] >= 0.0 and g["eps"] > 0.0 and g["weight_decay"] >= 0.0
                and g["initial_accumulator_value"] >= 0.0,
                "lr_decay >= 0, eps > 0, weight_decay >= 0, initial_accumulator_value >= 0",
                (g["lr_decay"], g["eps"], g["weight_decay"], g["initial_accumulator_value"]))

    def _new_state(self, p, key, g):
        return torch.full_like(p, float(g["initial_accumulator_value"]), memory_format=torch.contiguous_format)

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.ADAGRAD, 0, (float(g["lr_decay"]), float(g["eps"])), float(g["weight_decay"]))


class FusedAdadelta(_FusedOptim):
    """``torch.optim.Adadelta`` (L2 weight decay) on ``fastgrnn_hip_optim_update``."""
    _ALGO = _lib.ADADELTA
    _STATE_KEYS = ("square_avg", "acc_delta")

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, foreach=None, *, capturable=False,
                 maximize=False, differentiable=False):
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, maximize=maximize,
                                      capturable=capturable, foreach=foreach, differentiable=differentiable))

    def _ranges(self, g):
        return (0.0 <= g["rho"] <= 1.0 and g["eps"] > 0.0 and g["weight_decay"] >= 0.0,
                "rho in [0,1], eps > 0, weight_decay >= 0", (g["rho"], g["eps"], g["weight_decay"]))

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.ADADELTA, 0, (float(g["rho"]), float(g["eps"])), float(g["weight_decay"]))


class FusedAdamax(_FusedOptim):
    """``torch.optim.Adamax`` (L2 weight decay) on ``fastgrnn_hip_optim_update``."""
    _ALGO = _lib.ADAMAX
    _STATE_KEYS = ("exp_avg", "exp_inf")

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, foreach=None, *, maximize=False,
                 differentiable=False, capturable=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=foreach,
                                      maximize=maximize, differentiable=differentiable, capturable=capturable))

    def _ranges(self, g):
        b1, b2 = g["betas"]
        return (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and g["eps"] > 0.0 and g["weight_decay"] >= 0.0,
                "betas in [0,1), eps > 0, weight_decay >= 0", (g["betas"], g["eps"], g["weight_decay"]))

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.ADAMAX, 0, (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])),
                               float(g["weight_decay"]))


class FusedASGD(_FusedOptim):
    """``torch.optim.ASGD`` on ``fastgrnn_hip_optim_update``.  ``eta`` and ``mu``, which torch keeps per parameter (all
    equal), live in ``scalars``: float32 ``[4]`` on the parameters' device, the pair ``scalars[2 (t & 1):][:2]`` being what
    step ``t`` left for step ``t + 1`` (the library's double buffer); ``state_dict()`` exports them under torch's keys."""
    _ALGO = _lib.ASGD
    _STATE_KEYS = ("ax",)

    def __init__(self, params, lr=1e-2, lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0, foreach=None, maximize=False,
                 differentiable=False, capturable=False):
        super().__init__(params, dict(lr=lr, lambd=lambd, alpha=alpha, t0=t0, weight_decay=weight_decay,
                                      foreach=foreach, maximize=maximize, differentiable=differentiable,
                                      capturable=capturable))
        self.scalars = torch.tensor([float(lr), 1.0] * 2, dtype=torch.float32, device=self._device)

    def _ranges(self, g):
        finite = all(math.isfinite(float(g[k])) for k in ("lambd", "alpha", "t0"))
        return (finite and g["weight_decay"] >= 0.0, "finite lambd, alpha and t0, weight_decay >= 0",
                (g["lambd"], g["alpha"], g["t0"], g["weight_decay"]))

    def _extra_args(self):
        return (self.scalars.data_ptr(),)

    def run_tensors(self):                                   # step t + 1 reads the pair that step t wrote
        return super().run_tensors() + [self.scalars]

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.ASGD, 0, (float(g["lambd"]), float(g["alpha"]), float(g["t0"])),
                               float(g["weight_decay"]))

    def _export_step(self, t):
        super()._export_step(t)
        # (before the first step the kernel reads neither: eta = lr_t, mu = 1, which is what torch starts from)
        eta, mu = self.scalars[2 * (t & 1):][:2].tolist() if t >= 1 else (float(self.lr_t), 1.0)
        for p in self.param_groups[0]["params"]:
            if p in self.state and self.state[p]:
                self.state[p]["eta"], self.state[p]["mu"] = torch.tensor(eta), torch.tensor(mu)

    def _import_step(self, sd):
        t = super()._import_step(sd)
        pairs = {(float(st["eta"]), float(st["mu"])) for st in self.state.values() if st and "eta" in st and "mu" in st}
        if len(pairs) > 1:
            raise ValueError("FusedASGD keeps one eta and mu for all parameters (the checkpoint has %s)" % sorted(pairs))
        eta, mu = pairs.pop() if pairs else (float(self.param_groups[0]["lr"]), 1.0)
        self.scalars.copy_(torch.tensor([eta, mu] * 2, dtype=torch.float32))
        return t


class FusedRprop(_FusedOptim):
    """``torch.optim.Rprop`` on ``fastgrnn_hip_optim_update``.  Every element has a step size of its own, which starts
    at ``lr`` when the state is created (the first step, or a checkpoint) and is adapted from the gradient's sign: the
    learning rate is not read again, so ``lr_t``, schedulers and a ``TrainSchedule`` have no effect on this rule."""
    _ALGO = _lib.RPROP
    _STATE_KEYS = ("prev", "step_size")

    def __init__(self, params, lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50), *, capturable=False, foreach=None,
                 maximize=False, differentiable=False):
        super().__init__(params, dict(lr=lr, etas=etas, step_sizes=step_sizes, foreach=foreach, maximize=maximize,
                                      capturable=capturable, differentiable=differentiable))

    def _ranges(self, g):
        (em, ep), (lo, hi) = g["etas"], g["step_sizes"]
        return (0.0 < em < 1.0 < ep and lo <= hi and not g.get("weight_decay"),
                "0 < etaminus < 1 < etaplus, step_min <= step_max, no weight_decay", (g["etas"], g["step_sizes"]))

    def _new_state(self, p, key, g):
        if key == "step_size":
            return torch.full_like(p, float(g["lr"]), memory_format=torch.contiguous_format)
        return torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _hyper(self, g):
        return _lib.OptimHyper(_lib.RPROP, 0, tuple(float(v) for v in tuple(g["etas"]) + tuple(g["step_sizes"])), 0.0)


def configure_optimizer(params, options, capturable=False):
    """The reference's ``configure_optimizer`` (trainClassifier.py:67-95) on the fused classes: ``options`` is a
    ``TrainingOptions``-shaped object -- ``optimizer`` (one of the eight names), ``learning_rate`` and
    ``optimizer_options`` (``OptimizerOptions``: trainingConfig.py:43-58) -- and every rule takes from it exactly what
    the reference passes to ``torch.optim``."""
    lr, oo = options.learning_rate, options.optimizer_options
    name = options.optimizer
    if name == "Adadelta":
        return FusedAdadelta(params, lr=lr, weight_decay=oo.weight_decay, rho=oo.rho, eps=oo.eps, capturable=capturable)
    if name == "Adagrad":
        return FusedAdagrad(params, lr=lr, weight_decay=oo.weight_decay, lr_decay=oo.lr_decay, capturable=capturable)
    if name == "Adam":
        return FusedAdam(params, lr=lr, weight_decay=oo.weight_decay, betas=oo.betas, eps=oo.eps, capturable=capturable)
    if name == "Adamax":
        return FusedAdamax(params, lr=lr, weight_decay=oo.weight_decay, betas=oo.betas, eps=oo.eps, capturable=capturable)
    if name == "ASGD":
        return FusedASGD(params, lr=lr, weight_decay=oo.weight_decay, lambd=oo.lambd, alpha=oo.alpha, t0=oo.t0,
                         capturable=capturable)
    if name == "RMSprop":
        return FusedRMSprop(params, lr=lr, weight_decay=oo.weight_decay, eps=oo.eps, alpha=oo.alpha,
                            momentum=oo.momentum, centered=oo.centered, capturable=capturable)
    if name == "Rprop":
        return FusedRprop(params, lr=lr, etas=oo.etas, step_sizes=oo.step_sizes, capturable=capturable)
    if name == "SGD":
        return FusedSGD(params, lr=lr, weight_decay=oo.weight_decay, momentum=oo.momentum, dampening=oo.dampening,
                        nesterov=oo.nesterov, capturable=capturable)
    raise ValueError("configure_optimizer: %r is none of Adadelta, Adagrad, Adam, Adamax, ASGD, RMSprop, Rprop, SGD"
                     % (name,))
