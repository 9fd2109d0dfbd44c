"""Numpy restatements for the rolling mode (include/fastgrnn_hip.h: fastgrnn_hip_train_schedule_rolling,
fastgrnn_hip_rolling_exchange): the position of an iteration in closed form, a transcription of the control flow of the
reference's loop (trainClassifier.py:174-221) to hold it against, the keyed permutation of the bag rows with its inverse
(``augment_cases.philox``, the Feistel pass of ``schedule_cases``), and the bag exchange written as the reference's
scatter-then-slice (model.py:145-156) next to the order-free form the kernel uses."""
import numpy as np

from tests import augment_cases as A
from tests import schedule_cases as K

BAG_TAG = 0xC0000000


def constants(N, B, world, num_epochs, max_rolling_length):
    """``(ticks_full, n_short, total_iterations)``."""
    ticks_full = N // (B * world)
    max_roll = min(ticks_full, max_rolling_length + 2, num_epochs + 2)
    n_short = max(0, max_roll - 2)
    return ticks_full, n_short, n_short * (n_short + 3) // 2 + (num_epochs - n_short) * ticks_full


def reference_total(N, B, world, num_epochs, max_rolling_length):
    """trainClassifier.py:175-186 on ``ticks = N // (B world)`` whole batches."""
    ticks = N // (B * world)
    rolling_length = 2
    max_roll = int(ticks)
    if max_roll > max_rolling_length + rolling_length:
        max_roll = max_rolling_length + rolling_length
    if num_epochs + rolling_length < max_roll:
        max_roll = num_epochs + rolling_length
    total = sum(range(rolling_length, max_roll))
    if num_epochs + rolling_length > max_roll:
        total += (num_epochs + rolling_length - max_roll) * ticks
    return total


def position(s, N, B, world, num_epochs, max_rolling_length):
    """``(epoch, i_batch, fresh, zero)`` of the 0-based iteration ``s`` (a negative one counts as 0)."""
    ticks_full, n_short, _ = constants(N, B, world, num_epochs, max_rolling_length)
    s = max(int(s), 0)
    epoch = 0
    while epoch < n_short and s >= epoch + 2:                        # short epoch e has e + 2 iterations
        s -= epoch + 2
        epoch += 1
    if epoch == n_short:
        epoch, s = epoch + s // ticks_full, s % ticks_full
    return epoch, s, s == 0 and epoch <= n_short, s == 0 and epoch < n_short


def literal_loop(N, B, world, num_epochs, max_rolling_length):
    """The control flow of trainClassifier.py:174-221 with ``options.rolling`` on a loader of ``N // (B world)`` whole
    batches: yields ``(epoch, i_batch, fresh, zero)`` per trained batch.  ``fresh``: ``hidden_states`` were None when
    ``rolling_step`` ran (model.py:150: nothing is scattered and the forward starts from zeros); ``zero``:
    ``init_hidden_bag`` ran since the previous batch."""
    ticks = N // (B * world)
    rolling_length = 2
    max_roll = int(ticks)
    if max_roll > max_rolling_length + rolling_length:
        max_roll = max_rolling_length + rolling_length
    if num_epochs + rolling_length < max_roll:
        max_roll = num_epochs + rolling_length
    hidden = None                                                    # (the constructor's init_hidden)
    for epoch in range(num_epochs):
        zeroed = False
        rolling_length += 1
        if rolling_length <= max_roll:
            zeroed = True                                            # init_hidden_bag
        for i_batch in range(ticks):
            if rolling_length <= max_roll:
                if (i_batch + 1) % rolling_length == 0:
                    hidden = None                                    # init_hidden
                    break
            yield epoch, i_batch, hidden is None, zeroed
            zeroed = False
            hidden = "carried"                                       # the forward leaves its last states


def _pass(x, half, mask, c1, c2, key, inverse):
    L, R = x >> np.uint32(half), x & mask
    for r in ((3, 2, 1, 0) if inverse else (0, 1, 2, 3)):
        if inverse:
            L, R = R ^ (A.philox((L, c1, c2, BAG_TAG | r), key)[0] & mask), L
        else:
            L, R = R, L ^ (A.philox((R, c1, c2, BAG_TAG | r), key)[0] & mask)
    return (L << np.uint32(half)) | R


def bag_perm(seed, s, q, M, inverse=False):
    """``pi_s`` (or its inverse) of bag row(s) ``q`` (an integer or an array, each below ``M``) at iteration ``s``."""
    half = K.domain_bits(M) // 2
    mask = np.uint32((1 << half) - 1)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    s = max(int(s), 0)
    s_lo, s_hi = s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF
    x = np.atleast_1d(np.asarray(q, dtype=np.int64)).astype(np.uint32)
    assert (x < M).all()
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        x[todo] = _pass(x[todo], half, mask, s_lo, s_hi, key, inverse)
        todo &= x >= M
    out = x.astype(np.int64)
    return out if np.ndim(q) else int(out[0])


def exchange(state, bag, s, seed, sched):
    """One layer's bag exchange at iteration ``s`` as the reference writes it (model.py:145-156; ``sched`` = ``(N, B,
    world, num_epochs, max_rolling_length)``): ``bag:[M,H]`` is updated in place -- cleared where the bags start over,
    an indexed store of ``state:[B,H]`` at the shuffled rows otherwise --, and the ``h0`` of the iteration is returned:
    zeros on a fresh start, else the slice ``bag[:B]`` taken AFTER the store."""
    _, _, fresh, zero = position(s, *sched)
    if zero:
        bag[:] = 0
    if fresh:
        return np.zeros_like(state)
    B, M = state.shape[0], bag.shape[0]
    bag[bag_perm(seed, s, np.arange(B), M), :] = state
    return bag[:B].copy()


class Exchange:
    """The stateful oracle over a run: ``bags[l]:[M,H_l]`` as uint32 bit patterns, zero at first.  ``step(s, states)``
    takes the previous iteration's final states (``[B,H_l]`` uint32 each) through ``exchange`` layer by layer and
    returns the ``h0`` of iteration ``s``."""

    def __init__(self, seed, B, bag_count, sizes, sched):
        self.seed, self.sched = seed, sched
        self.bags = [np.zeros((B * bag_count, h), dtype=np.uint32) for h in sizes]

    def step(self, s, states):
        return [exchange(st, bag, s, self.seed, self.sched) for st, bag in zip(states, self.bags)]


def h0_by_inverse(seed, s, B, M, state, bag_before):
    """The order-free form: ``h0[r] = state[pi_s^-1(r)]`` where that is a batch row, else the old ``bag[r]``; also the
    rows that came from ``state``."""
    src = bag_perm(seed, s, np.arange(B), M, inverse=True)
    from_state = src < B
    out = bag_before[:B].copy()
    out[from_state] = state[src[from_state]]
    return out, from_state
