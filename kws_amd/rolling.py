"""The hidden-state bags of the reference's rolling training (model.py:135-156, trainClassifier.py:198-219) on the device.

In rolling mode a batch does not start from the zero state: after every iteration each layer's final states are scattered
into that layer's "hidden bag" (``batch_size * bag_count`` rows) at shuffled positions, and the next batch starts from
bag rows ``0 .. batch_size - 1``.  The reference does this on the host between two iterations (``rolling_step``: one
``np.random.shuffle`` of the bag's row numbers, an indexed store and a slice per layer); here the shuffle is a keyed
permutation of the iteration number and the whole exchange of all layers is one library call
(``fastgrnn_hip_rolling_exchange``, include/fastgrnn_hip.h) that reads ``optimizer.step_t`` on the device, so it is
captured in the training graph with the rest (``RNNClassifierModel.fit_audio`` on a ``TrainSchedule(..., rolling=True)``).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .fastgrnn_cuda import _call
from .schedule import TrainSchedule


class RollingBags:
    """``RollingBags(model, schedule)``: per layer ``l`` of ``model`` (a ``kws_amd.RNNClassifierModel`` of 1-3 layers) the
    persistent tensors ``state[l]:[B,H_l]`` (the previous iteration's final states), ``bag[l]:[B * bag_count, H_l]`` and
    ``h0[l]:[B,H_l]`` (the states the next iteration starts from), fp32 on the model's device, all zeros; ``B`` and
    ``bag_count`` are those of ``schedule``, a ``TrainSchedule`` built with ``rolling=True``.  An iteration is

        schedule.advance(); bags.exchange(); model.train_step_audio(...); bags.commit()

    The carried state lives here, not in ``model.hidden_states``: whatever runs the model between two iterations (a
    validation pass) cannot disturb it.  Construction needs no GPU; ``exchange`` does."""

    def __init__(self, model, schedule):
        if not isinstance(schedule, TrainSchedule) or not schedule.rolling:
            raise ValueError("RollingBags needs a kws_amd.TrainSchedule built with rolling=True")
        sizes = [int(h) for h in model.hidden_units_list[:model.num_layers]]
        if not 1 <= len(sizes) <= _lib.ROLLING_MAX_LAYERS:
            raise ValueError("RollingBags exchanges 1 to %d layers in one launch (the model has %d)"
                             % (_lib.ROLLING_MAX_LAYERS, len(sizes)))
        dev = next(model.parameters()).device
        if dev != schedule.device:
            raise ValueError("the model is on %s, the schedule's optimizer on %s" % (dev, schedule.device))
        self.model, self.schedule, self.device = model, schedule, dev
        B, M = schedule.batch_size, schedule.batch_size * schedule.bag_count
        new = lambda rows, h: torch.zeros(rows, h, dtype=torch.float32, device=dev)
        self.state = [new(B, h) for h in sizes]
        self.bag = [new(M, h) for h in sizes]
        self.h0 = [new(B, h) for h in sizes]
        self.desc = _lib.RollingDesc(schedule.max_rolling_length, schedule.bag_count, len(sizes), 0,
                                     (C.c_int32 * 4)(*sizes))
        self.bind()

    def bind(self):
        """Take the addresses of ``state``, ``bag`` and ``h0`` as they stand (after replacing one of the tensors)."""
        self._pointers = tuple((C.c_void_p * 3)(*[t.data_ptr() for t in group])
                               for group in (self.state, self.bag, self.h0))

    def tensors(self):
        """Every tensor an iteration writes here (what a capture's warm-up has to put back)."""
        return self.state + self.bag + self.h0

    run_tensors = tensors                                    # (kws_amd.graph.RunSnapshot's name for it)

    def exchange(self):
        """The bag exchange of the iteration that ``optimizer.step_t`` counts as done so far -- ``state`` into the bags at
        the iteration's shuffled rows, ``h0`` out of bag rows ``0 .. B-1``; zero states on an epoch's fresh start,
        cleared bags at the start of a short epoch -- in one library call, then ``model.hidden_states = h0``.  Nothing
        synchronises."""
        if self.device.type != "cuda":
            raise RuntimeError("RollingBags.exchange() runs on the GPU (the model is on %s); kws_amd has no CPU fallback"
                               % (self.device,))
        sched = self.schedule
        with torch.cuda.device(self.device):
            _call(_lib.load().fastgrnn_hip_rolling_exchange, "fastgrnn rolling_exchange", "rolling_exchange", self.device,
                  None, C.byref(sched.desc), C.byref(self.desc), sched.optimizer.step_t.data_ptr(),
                  C.byref(self._pointers[0]), C.byref(self._pointers[1]), C.byref(self._pointers[2]))
        self.model.hidden_states = list(self.h0)
        return self.h0

    def commit(self):
        """``state[l] = model.hidden_states[l]``, the final states of the step just run: one ``copy_`` per layer."""
        for dst, src in zip(self.state, self.model.hidden_states):
            dst.copy_(src)
