"""A training (or inference) step captured once in a HIP graph and replayed.

The operator behind ``FastGRNNCUDA`` makes no host-side decision that depends on data, allocates through torch's
allocator only and launches on the current stream, so forward + autograd backward of a whole model capture as they
are (``torch.cuda.CUDAGraph`` is a hipGraph on ROCm).  A replay costs the host about ten microseconds instead of the
130-270 us of the eager step, which takes the host out of the step time on a slow or busy core.
Shapes, flags and tensor addresses are frozen at capture: feed new batches by copying into the captured input
tensors (``x.copy_(batch)``), read results from the captured outputs / ``.grad`` tensors.

The warm-up calls before the capture are real steps.  ``GraphedStep(fn, undo=owners)`` puts back what they wrote, from
each owner's own list (``RunSnapshot``): an owner is any object with ``run_tensors()`` -- the tensors from which an
iteration reads a value that an earlier iteration wrote -- and, optionally, ``run_reset(held_ids)`` for what a list of
tensors cannot express.  The model, the fused optimizers, ``TrainSchedule`` and ``RollingBags`` are owners.
"""
import torch


class RunSnapshot:
    """Copies of every tensor in ``owner.run_tensors()`` of each of ``owners``, taken on construction.  ``restore()``
    copies them back and then calls ``owner.run_reset(held_ids)`` where an owner has one, ``held_ids`` being the
    ``id()`` of every tensor the snapshot holds: that is where an owner deals with what came into being after the
    snapshot (optimizer state that the first step creates) or is no tensor of its own (the model's carried hidden
    states).  Works on any device."""

    def __init__(self, owners):
        self.owners = list(owners)
        self.held = [(t, t.detach().clone()) for owner in self.owners for t in owner.run_tensors()]

    def restore(self):
        held_ids = {id(t) for t, _ in self.held}
        with torch.no_grad():
            for t, value in self.held:
                t.copy_(value)
            for owner in self.owners:
                if hasattr(owner, "run_reset"):
                    owner.run_reset(held_ids)


class GraphedStep:
    """``GraphedStep(fn)`` runs ``fn()`` a few times on a side stream (plan and workspace caches, lazy library
    state), captures one call, and replays it on every ``__call__``.  ``fn`` typically resets ``.grad`` to None and
    runs forward + backward; the gradient tensors allocated during capture stay alive and are overwritten in place
    by each replay.  ``outputs`` holds whatever ``fn`` returned during capture (static tensors).

    ``undo``: the owners (see ``RunSnapshot``) whose state the first replay should find as it stood before the
    warm-up, e.g. ``undo=(model, optimizer)``.  Empty by default: nothing is copied, and the warm-up's steps stay."""

    def __init__(self, fn, warmup=3, undo=()):
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedStep needs a GPU (HIP graph capture)")
        keep = RunSnapshot(undo) if undo else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outputs = fn()
        if keep is not None:
            keep.restore()

    def __call__(self):
        self.graph.replay()
        return self.outputs
