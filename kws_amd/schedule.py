"""The batch, the learning rate and the IHT phase of every trainer iteration, computed on the device from the step count.

A trainer iteration already runs on the device and captures in one graph (``RNNClassifierModel.train_step_audio``); what
the host still supplied between two replays were the batch's clip indices, the learning rate and the IHT phase.  All
three are functions of the iteration number, which lives in the fused optimizer's ``step_t``:

* ``TrainSchedule.advance()`` is one library call (``fastgrnn_hip_train_schedule``, include/fastgrnn_hip.h) that reads
  ``step_t`` and writes ``index:[B]`` (the batch of a shuffled epoch order without replacement: a keyed permutation of the
  clip numbers, new in every epoch, sharded over ``world`` ranks), ``optimizer.lr_t`` (one of the reference's five
  schedules, trainClassifier.py:97-123 and utils.py:116-143, or the constant rate), ``optimizer.iht_t``
  (trainClassifier.py:251-259, ``kws_amd.iht_phase``) and ``where = (epoch, i_batch, slot, 0)``;
* ``TrainSchedule.record(loss)`` files the loss and the learning rate under ``slot`` in two device logs;
* ``RNNClassifierModel.fit_audio`` captures ``advance`` + ``train_step_audio`` + ``record`` once and replays the graph
  ``num_epochs * ticks`` times: no host-to-device write, no loader thread, reproducible from ``seed``.

* ``TrainSchedule(..., rolling=True)`` is the reference's ``--rolling`` mode (trainClassifier.py:174-221): ``n_short``
  short epochs of 2, 3, .. iterations in front of the full ones, ``advance()`` through
  ``fastgrnn_hip_train_schedule_rolling`` with ``where = (epoch, i_batch, slot, fresh | zero << 1)``; the hidden-state bags
  that go with it are ``kws_amd.RollingBags``.

Two deliberate differences from the reference: an epoch has ``ticks = num_clips // (batch_size * world)`` whole batches
(drop_last; the reference's loader ends an epoch on a short batch, which a captured graph's fixed shapes cannot take, and
its ``ticks`` is the fraction ``num_clips / batch_size``), and ``"CosineAnnealingLR"`` is torch's CLOSED form (the
recursive one the reference steps differs from it by rounding and divides by zero at some non-integer ``T_max``).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .fastgrnn_cuda import _call
from .optim import _FusedOptimizer

LR_SCHEDULERS = tuple(_lib.LR_KINDS)


def _whole(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo:
        raise ValueError("%s must be an integer >= %d (got %r)" % (name, lo, v))
    return v


def _positive(v, name):
    v = float(v)
    if not (v > 0.0 and v != math.inf):
        raise ValueError("%s must be a finite positive number (got %r)" % (name, v))
    return v


class TrainSchedule:
    """``TrainSchedule(optimizer, num_clips, batch_size, num_epochs, seed=...)``: the run's position, batch, learning rate
    and IHT phase as functions of ``optimizer.step_t``.

    ``optimizer``: a ``FusedAdam`` / ``FusedSGD``, or any other fused optimizer of ``kws_amd.optim``, built with
    ``capturable=True`` (its ``lr_t`` then belongs to the caller, here to ``advance``); its ``lr`` is the schedules'
    base (peak) rate.  Under ``FusedRprop`` ``lr_t`` is written and ignored: that rule keeps a step size per element and
    reads no learning rate.  ``lr_scheduler``: ``None`` or one of the
    reference's names, with ``configure_lr``'s constants (``ticks`` as above): ``steps = 2 lr_peaks + 1``, ``stepsize =
    num_epochs / steps * ticks`` (TriangleLR), ``t_max = ticks * num_epochs / steps`` (CosineAnnealingLR), ``reset =
    int(num_epochs * ticks / 3)`` (ExponentialResettingLR), ``lr_min`` falling back to the base rate.  ``lr_lead = 1``
    is the reference's order -- ``scheduler.step()`` before ``optimizer.step()``, so iteration ``s`` runs at the
    schedule's ``s + 1`` --, ``lr_lead = 0`` torch's documented one.  ``sparsify`` turns the IHT phases on (``trim_level``:
    a threshold every so many batches of the middle third; the reference's default is 15).  ``world`` / ``rank``: each
    rank builds its own schedule and gets a disjoint share of every epoch.  ``log_len``: entries of ``loss_log`` /
    ``lr_log`` (default: one per iteration); iterations past it share the last entry.

    ``rolling=True``: the reference's rolling mode.  ``full_ticks = num_clips // (batch_size * world)`` must be at least 2
    (at 1 the reference's iteration count disagrees with its own loop), ``max_roll = min(full_ticks, max_rolling_length
    + 2, num_epochs + 2)``, ``n_short = max(0, max_roll - 2)``: epoch ``e < n_short`` trains ``e + 2`` batches of its
    order from cleared bags, the others ``full_ticks``, ``total_iterations = n_short (n_short + 3) / 2 + (num_epochs -
    n_short) full_ticks``.  ``ticks`` is then the reference's fraction ``total_iterations / num_epochs``
    (trainClassifier.py:187), from which ``configure_lr``'s constants are derived as there (``t_max =
    total_iterations / steps``).  ``bag_count``: rows of a hidden bag per batch row (the reference's 100).  Without
    ``rolling`` the two keywords are not read, ``full_ticks == ticks`` and ``n_short == 0``.

    Construction needs no GPU (the tensors live on the optimizer's device); ``advance`` does."""

    def __init__(self, optimizer, num_clips, batch_size, num_epochs, *, seed, lr_scheduler=None, lr_min=None, lr_peaks=1,
                 gamma=1.0, lr_step_size=1, lr_lead=1, sparsify=False, trim_level=15, world=1, rank=0, log_len=None,
                 rolling=False, max_rolling_length=100, bag_count=100):
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("TrainSchedule needs a kws_amd.FusedAdam or kws_amd.FusedSGD, or another fused optimizer of "
                            "kws_amd.optim (got %s): it writes the "
                            "optimizer's device scalars lr_t and iht_t" % type(optimizer).__name__)
        if not optimizer.param_groups[0].get("capturable"):
            raise ValueError("TrainSchedule needs an optimizer built with capturable=True: otherwise %s.step() overwrites "
                             "lr_t from param_groups" % type(optimizer).__name__)
        self.optimizer = optimizer
        self.num_clips = _whole(num_clips, "num_clips", 1)
        self.batch_size = _whole(batch_size, "batch_size", 1)
        self.num_epochs = _whole(num_epochs, "num_epochs", 1)
        self.world = _whole(world, "world", 1)
        self.rank = _whole(rank, "rank", 0)
        if self.rank >= self.world:
            raise ValueError("rank must be in 0..world-1 (got rank %d of %d)" % (self.rank, self.world))
        if self.batch_size * self.world > 2 ** 31 - 1 or self.num_clips > 2 ** 31 - 1:
            raise ValueError("num_clips and batch_size * world must fit int32")
        if self.num_clips < self.batch_size * self.world:
            raise ValueError("num_clips = %d holds no batch of %d clips on each of %d ranks (drop_last)"
                             % (self.num_clips, self.batch_size, self.world))
        self.seed = _whole(seed, "seed", 0)
        if self.seed >= 1 << 64:
            raise ValueError("seed must fit 64 bits (got %d)" % self.seed)
        if lr_scheduler not in _lib.LR_KINDS:
            raise ValueError("lr_scheduler must be one of %s (got %r)" % (", ".join(map(repr, LR_SCHEDULERS)), lr_scheduler))
        if lr_lead not in (0, 1):
            raise ValueError("lr_lead must be 0 or 1 (got %r)" % (lr_lead,))
        self.lr_scheduler, self.lr_lead = lr_scheduler, int(lr_lead)
        self.sparsify = bool(sparsify)
        self.trim_level = _whole(trim_level, "trim_level", 1)
        self.lr_base = float(optimizer.param_groups[0]["lr"])
        self.lr_min = self.lr_base if not lr_min else float(lr_min)          # configure_lr: `if not lr_min`
        if not (0.0 <= self.lr_min < math.inf and 0.0 <= self.lr_base < math.inf):
            raise ValueError("the learning rates must be finite and >= 0 (got lr %r, lr_min %r)" % (self.lr_base, lr_min))
        self.gamma = _positive(gamma, "gamma")
        self.lr_step_size = _whole(lr_step_size, "lr_step_size", 1)
        lr_peaks = lr_peaks if isinstance(lr_peaks, int) else float(lr_peaks)      # (the reference's --lr_peaks is a float)
        _positive(lr_peaks, "lr_peaks")
        # configure_lr's constants, in its order of operations
        self.full_ticks = self.num_clips // (self.batch_size * self.world)
        self.rolling = bool(rolling)
        self.steps = lr_peaks * 2 + 1
        if self.rolling:
            self.max_rolling_length = _whole(max_rolling_length, "max_rolling_length", 0)
            self.bag_count = _whole(bag_count, "bag_count", 1)
            if self.max_rolling_length > 2 ** 31 - 1 or self.batch_size * self.bag_count > 2 ** 31 - 1:
                raise ValueError("max_rolling_length and batch_size * bag_count must fit int32")
            if self.full_ticks < 2:
                raise ValueError("rolling training needs at least 2 batches per epoch and rank (num_clips = %d gives %d "
                                 "of %d clips on each of %d ranks)"
                                 % (self.num_clips, self.full_ticks, self.batch_size, self.world))
            max_roll = min(self.full_ticks, self.max_rolling_length + 2, self.num_epochs + 2)
            self.n_short = max(0, max_roll - 2)
            self.total_iterations = (self.n_short * (self.n_short + 3) // 2
                                     + (self.num_epochs - self.n_short) * self.full_ticks)
            self.ticks = self.total_iterations / self.num_epochs             # trainClassifier.py:187: a float
            self.t_max = self.total_iterations / self.steps                  # trainClassifier.py:114
            self.rolling_desc = _lib.RollingDesc(self.max_rolling_length, self.bag_count, 0, 0)
        else:
            self.n_short = 0
            self.ticks = self.full_ticks
            self.total_iterations = self.num_epochs * self.ticks
            self.t_max = self.ticks * self.num_epochs / self.steps
        self.stepsize = self.num_epochs / self.steps * self.ticks
        self.reset = int(self.num_epochs * self.ticks / 3)
        self.log_len = self.total_iterations if log_len is None else _whole(log_len, "log_len", 1)
        dev = optimizer._device
        self.device = dev
        self.index = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
        self.where = torch.zeros(4, dtype=torch.int64, device=dev)
        self.loss_log = torch.zeros(self.log_len, dtype=torch.float32, device=dev)
        self.lr_log = torch.zeros(self.log_len, dtype=torch.float32, device=dev)
        self.norm_log = self.skip_log = None                                 # a guarded optimizer's: _guard_logs()
        self._guard_logs()
        self.desc = _lib.ScheduleDesc(self.num_clips, self.batch_size, self.world, self.rank, self.seed, self.num_epochs,
                                      self.trim_level, int(self.sparsify), _lib.LR_KINDS[lr_scheduler], self.lr_lead, 0,
                                      self.log_len, self.lr_base, self.lr_min, self.gamma, self.stepsize, self.t_max,
                                      self.lr_step_size, self.reset)

    def advance(self):
        """Fill ``index``, ``optimizer.lr_t``, ``optimizer.iht_t`` and ``where`` for the iteration that ``optimizer.step_t``
        counts as done so far (0-based: the scalar as it stands before this iteration's ``step()``): one library call,
        no host decision on device data, nothing synchronises.  Follow it with ``train_step_audio(..., self.index, ...,
        iht=None)``, which leaves ``iht_t`` as written here."""
        opt = self.optimizer
        if self.device.type != "cuda":
            raise RuntimeError("TrainSchedule.advance() runs on the GPU (the optimizer is on %s); kws_amd has no CPU "
                               "fallback" % (self.device,))
        outs = (opt.step_t.data_ptr(), self.index.data_ptr(), opt.lr_t.data_ptr(), opt.iht_t.data_ptr(),
                self.where.data_ptr())
        with torch.cuda.device(self.device):
            if self.rolling:
                _call(_lib.load().fastgrnn_hip_train_schedule_rolling, "fastgrnn train_schedule_rolling",
                      "train_schedule_rolling", self.device, None, C.byref(self.desc), C.byref(self.rolling_desc), *outs)
            else:
                _call(_lib.load().fastgrnn_hip_train_schedule, "fastgrnn train_schedule", "train_schedule", self.device,
                      None, C.byref(self.desc), *outs)
        return self.index

    def epoch_start(self, epoch):
        """The 0-based iteration at which ``epoch`` begins."""
        short = min(epoch, self.n_short)
        return short * (short + 3) // 2 + (epoch - short) * self.full_ticks

    def position(self, s):
        """``(epoch, i_batch)`` of the 0-based iteration ``s`` on the host: what ``advance`` writes to ``where[:2]``."""
        s = max(int(s), 0)
        first_full = self.epoch_start(self.n_short)
        if s >= first_full:
            return self.n_short + (s - first_full) // self.full_ticks, (s - first_full) % self.full_ticks
        epoch = (math.isqrt(9 + 8 * s) - 3) // 2                     # the largest e with e (e + 3) / 2 <= s
        return epoch, s - self.epoch_start(epoch)

    def epoch_end(self, s):
        """Whether the 0-based iteration ``s`` (a negative one counts as 0) is the last of its epoch."""
        return self.position(max(int(s), 0) + 1)[1] == 0

    def _guard_logs(self):
        """``norm_log`` (float32) and ``skip_log`` (int32), ``[log_len]`` each, once the optimizer has a gradient guard;
        ``(None, None)`` without one.  They are allocated when the schedule is built on a guarded optimizer, or, where
        ``optimizer.guard()`` follows the schedule's construction, by the first call of this method -- ``record()``,
        ``epoch_log()`` and ``fit_audio`` make it.  That first call must not fall inside a graph capture (the tensors
        would belong to the capture's memory pool): it is refused there.  Call ``guard()`` before building the schedule,
        or ``record()`` once eagerly, or this method, before capturing."""
        if self.norm_log is None and getattr(self.optimizer, "guarded", False):
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TrainSchedule: the guard's logs would be allocated inside a graph capture -- call "
                                   "optimizer.guard() before building the schedule, or schedule._guard_logs() before "
                                   "the capture")
            self.norm_log = torch.zeros(self.log_len, dtype=torch.float32, device=self.device)
            self.skip_log = torch.zeros(self.log_len, dtype=torch.int32, device=self.device)
        return self.norm_log, self.skip_log

    def run_tensors(self):
        """The logs, whose slots hold what earlier iterations recorded (``kws_amd.graph.RunSnapshot``); asking for them
        allocates a guarded optimizer's two, ahead of any capture.  ``index`` and ``where`` are not carried over:
        ``advance()`` writes them before anything reads them."""
        return [self.loss_log, self.lr_log] + [t for t in self._guard_logs() if t is not None]

    def record(self, loss):
        """``loss_log[slot] = loss`` and ``lr_log[slot] = lr_t`` for the ``slot`` that ``advance`` wrote: two indexed
        copies addressed by the device scalar, no sync, capturable.  On a guarded optimizer also
        ``norm_log[slot] = grad_norm_t`` and ``skip_log[slot] = skip_t``, the guard's verdict on this iteration."""
        slot = self.where[2:3]
        self.loss_log.index_copy_(0, slot, loss.detach().reshape(1).to(torch.float32))
        self.lr_log.index_copy_(0, slot, self.optimizer.lr_t)
        norm_log, skip_log = self._guard_logs()
        if norm_log is not None:
            norm_log.index_copy_(0, slot, self.optimizer.grad_norm_t)
            skip_log.index_copy_(0, slot, self.optimizer.skip_t)

    def epoch_log(self, accuracies=None):
        """The reference's log (trainClassifier.py:272): one dict per epoch with the epoch's last loss, its last learning
        rate and ``accuracies[epoch]`` (None without), read from the two logs -- one device-to-host copy each.  On a
        guarded optimizer every dict also carries ``"skipped"``, the number of the epoch's iterations the guard
        rejected, and ``"grad_norm"``, the epoch's last gradient norm."""
        loss, lr = self.loss_log.cpu().tolist(), self.lr_log.cpu().tolist()
        norm_log, skip_log = self._guard_logs()
        if norm_log is not None:
            norm, skip = norm_log.cpu().tolist(), skip_log.cpu().tolist()
        out = []
        for epoch in range(self.num_epochs):
            slot = min(self.epoch_start(epoch + 1) - 1, self.log_len - 1)
            out.append({"epoch": epoch, "loss": loss[slot], "accuracy": accuracies[epoch] if accuracies else None,
                        "learning_rate": lr[slot]})
            if norm_log is not None:
                out[-1]["skipped"] = sum(skip[min(self.epoch_start(epoch), self.log_len):slot + 1])
                out[-1]["grad_norm"] = norm[slot]
        return out
