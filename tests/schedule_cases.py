"""Numpy restatements for the device-side schedule (include/fastgrnn_hip.h: fastgrnn_hip_train_schedule): the keyed
permutation of an epoch's clip order (four Feistel rounds on ``augment_cases.philox``, cycle-walked), a batch's clip
numbers, the six learning-rate formulas in Python double, and the IHT phase through ``kws_amd.iht_phase``."""
import math

import numpy as np

from kws_amd import iht_phase
from kws_amd._lib import IHT_NONE, IHT_SUPPORT, IHT_THRESHOLD
from tests import augment_cases as A

SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 50, 255, 256, 257, 1023, 1025, 4097, 85511)
EPOCHS = (0, 1, (1 << 33) + 7)
KINDS = {None: 0, "TriangleLR": 1, "CosineAnnealingLR": 2, "ExponentialLR": 3, "StepLR": 4, "ExponentialResettingLR": 5}
PHASE_CODE = {"none": IHT_NONE, "threshold": IHT_THRESHOLD, "support": IHT_SUPPORT}


def domain_bits(N):
    """The smallest even k >= 2 with 2^k >= N."""
    k = 2
    while (1 << k) < N:
        k += 2
    return k


def epoch_perm(seed, epoch, q, N, count_passes=False):
    """Where position(s) ``q`` (an integer or an array, each below ``N``) of ``epoch``'s order point: clip numbers below
    ``N``.  With ``count_passes`` also the longest walk, in passes."""
    half = domain_bits(N) // 2
    mask = np.uint32((1 << half) - 1)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    e_lo, e_hi = epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF
    x = np.atleast_1d(np.asarray(q, dtype=np.int64)).astype(np.uint32)
    assert (x < N).all()
    todo, passes = np.ones(x.shape, dtype=bool), 0
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint32(half), v & mask
        for r in range(4):
            p = A.philox((R, e_lo, e_hi, 0x80000000 | r), key)[0]
            L, R = R, L ^ (p & mask)
        x[todo] = (L << np.uint32(half)) | R
        todo &= x >= N
        passes += 1
    out = x.astype(np.int64)
    out = out if np.ndim(q) else int(out[0])
    return (out, passes) if count_passes else out


def position(step, N, B, world=1):
    """``(epoch, i_batch, ticks)`` of the 0-based iteration ``step`` (a negative one counts as 0)."""
    ticks = N // (B * world)
    s = max(int(step), 0)
    return s // ticks, s % ticks, ticks


def batch_index(seed, step, N, B, world=1, rank=0):
    """``index:[B]`` int32 of iteration ``step`` on ``rank``."""
    epoch, i_batch, _ = position(step, N, B, world)
    q = (i_batch * world + rank) * B + np.arange(B, dtype=np.int64)
    return epoch_perm(seed, epoch, q, N).astype(np.int32)


def constants(lr_base, num_epochs, ticks, lr_peaks=1, lr_min=None, gamma=1.0, lr_step_size=1):
    """The reference's ``configure_lr`` constants (trainClassifier.py:97-123) as ``lr_at``'s keywords."""
    steps = lr_peaks * 2 + 1
    return dict(lr_base=float(lr_base), lr_min=float(lr_min) if lr_min else float(lr_base), gamma=float(gamma),
                stepsize=num_epochs / steps * ticks, t_max=ticks * num_epochs / steps, step_size=int(lr_step_size),
                reset=int(num_epochs * ticks / 3))


def lr_at(kind, it, lr_base, lr_min=None, gamma=1.0, stepsize=1.0, t_max=1.0, step_size=1, reset=0):
    """The learning rate of schedule ``kind`` (a name of ``KINDS`` or its code) at the schedule's iteration ``it``, in
    Python double: the header's formulas as the reference and torch's closed forms spell them."""
    kind = KINDS.get(kind, kind)
    lr_min = lr_base if lr_min is None else lr_min
    it = int(it)
    if kind == 0:
        return float(lr_base)
    if kind == 1:                                                    # utils.py:124-130
        cycle = math.floor(1 + it / (2 * stepsize))
        x = abs(it / stepsize - 2 * cycle + 1)
        return lr_min + (lr_base - lr_min) * gamma ** (it / 3) * x
    if kind == 2:                                                    # CosineAnnealingLR._get_closed_form_lr
        return lr_min + (lr_base - lr_min) * (1 + math.cos(math.pi * it / t_max)) / 2
    if kind == 3:
        return lr_base * gamma ** it
    if kind == 4:
        return lr_base * gamma ** (it // step_size)
    if kind == 5:                                                    # utils.py:138-143
        return lr_base * gamma ** (it - reset if it > reset else it)
    raise ValueError(kind)


def lr_bound(lr_base):
    """The issue's bound on a device learning rate against ``lr_at``, as a function of the value compared:
    ``max(1 fp32 ulp, 1e-12 lr_base)``."""
    return lambda want: max(float(np.spacing(np.float32(abs(want)))), 1e-12 * lr_base)


def phase(epoch, num_epochs, i_batch, trim_level, sparsify=True):
    """``train_update``'s code of the IHT phase, through ``kws_amd.iht_phase``."""
    return PHASE_CODE[iht_phase(epoch, num_epochs, i_batch, trim_level)] if sparsify else IHT_NONE


def phase_by_integers(epoch, num_epochs, i_batch, trim_level):
    """The header's integer rule."""
    if 3 * epoch < num_epochs:
        return IHT_NONE
    if 3 * epoch < 2 * num_epochs:
        return IHT_THRESHOLD if i_batch % trim_level == 0 else IHT_SUPPORT
    return IHT_SUPPORT
