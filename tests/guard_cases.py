"""The gradient guard restated in numpy and Python floats (tests/test_guard_cpu.py, tests/test_hip_guard.py): what
fastgrnn_hip_grad_guard writes into its 32-byte state for given gradients, as include/fastgrnn_hip.h defines it.

    S     = the sum of g^2 over every element of every segment.  A Python float is a double and the square of an fp32
            value is exact in it, so math.fsum over the squares is the correctly rounded S.
    norm  = (float)sqrt(S)
    skip  = skip_nonfinite and not isfinite(S)
    coef  = 0 when skip;  1 when max_norm is inf;  else (float)min(1, max_norm / (sqrt(S) + 1e-6)), a NaN staying a NaN
            (torch.clamp keeps it; tests/test_guard_cpu.py holds this to clip_grad_norm_ itself)
    applied, skipped: exactly one of them goes up by one.

Bounds used by the GPU tests, from the formats alone: the kernel's S is a sum of N exact terms in double in another
order, so it differs from fsum's by at most N 2^-53 relative (N <= 33 * 2^22: below 2^-25 of an fp32 ulp after the square
root halves it); norm and coef are each one rounding to fp32 of a double that is that close to the restatement's, so
they lie within ONE fp32 ulp of it (the double may sit next to a rounding boundary)."""
import functools
import math

import numpy as np

SEG_SIZES = (1, 1023, 1024, 1025, 4097)      # one element; around the workgroup's 1024 threads; one past its 4-load round
MIXED_SIZES = tuple(range(5, 38))            # 33 segments: one more than a launch takes
BAD_VALUES = (float("nan"), float("inf"), float("-inf"))


def sumsq(grads):
    """S: the correctly rounded double sum of the exact squares (nan / inf as IEEE gives them)"""
    parts = []
    for g in grads:
        a = np.asarray(g, dtype=np.float32).astype(np.float64).reshape(-1)
        with np.errstate(over="ignore", invalid="ignore"):
            parts.extend((a * a).tolist())
    if any(math.isnan(v) for v in parts):
        return float("nan")
    return math.fsum(parts)


def restate(grads, max_norm=math.inf, skip_nonfinite=True, applied=0, skipped=0):
    """-> dict(S, norm, coef, skip, applied, skipped); norm and coef are numpy float32"""
    S = sumsq(grads)
    root = math.sqrt(S) if not math.isnan(S) else float("nan")
    skip = bool(skip_nonfinite and not math.isfinite(S))
    if skip:
        coef = 0.0
    elif max_norm == math.inf:
        coef = 1.0
    else:
        c = max_norm / (root + 1e-6)
        coef = 1.0 if c > 1.0 else c                 # (a NaN fails the comparison and stays)
    return {"S": S, "norm": np.float32(root), "coef": np.float32(coef), "skip": int(skip),
            "applied": applied + (0 if skip else 1), "skipped": skipped + (1 if skip else 0)}


def ulps_apart(a, b):
    """the distance of two finite fp32 values of one sign in units of the last place (0: the same bits)"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


@functools.lru_cache(maxsize=None)
def gradient(n, seed, scale=1.0):
    """a read-only fp32 gradient of n elements"""
    g = (scale * np.random.default_rng(7000 + 31 * seed + n).standard_normal(n)).astype(np.float32)
    g.setflags(write=False)
    return g
