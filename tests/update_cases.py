"""Operands, fp64 oracles and bounds for fastgrnn_hip_train_update (tests/test_update_cpu.py, tests/test_hip_update.py).

The oracles are the formulas of include/fastgrnn_hip.h evaluated in numpy fp64 on the fp32 inputs.  The bounds are
derived, not tuned: every output is a chain of at most about seven fp32 roundings of terms whose magnitudes are known,
so with u = 2^-24 an output may differ from the fp64 value by 8u times the sum of the magnitudes of its terms (the
update with every term replaced by its absolute value -- not |p' - p|: beta1 m + (1-beta1) g cancels).  A faithful fp32
implementation (torch.optim on the CPU, foreach=False) stays within 4.8u (Adam) and 3.4u (SGD) of the same fp64 values
over n up to 200 000, steps 1 .. 100 001, wd 0 / 1e-5 and gradient scales 1e-3 .. 30; every test asserts torch's own
fp32 step against the bound before it holds the kernel to it.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
BOUND = 8 * U
SIZES = (1, 1023, 1024, 1025, 3 * 1024 + 7, 65536)     # one element; around the workgroup's 1024 threads; 64 per thread
STEPS = (1, 2, 1000)
WDS = (0.0, 1e-5)
SPARSITIES = (0.05, 0.3, 0.5, 1.0)
ADAM = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8)
SGD = dict(lr=0.05, momentum=0.9, dampening=0.0)
ALGOS = ("adam", "sgd", "sgd_nesterov")


def lr32(lr):
    """the learning rate the kernel sees: the device scalar is fp32"""
    return float(np.float32(lr))


# ---- fp64 oracles ------------------------------------------------------------------------------------------------------
def adam_oracle(p, g, m, v, lr, betas, eps, wd, t):
    """-> (p', m', v', bound_p, bound_m, bound_v), all float64; inputs are taken as they are (fp32 values)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    g1 = g + wd * p
    gabs = np.abs(g) + wd * np.abs(p)
    m1 = b1 * m + (1 - b1) * g1
    v1 = b2 * v + (1 - b2) * g1 * g1
    step_size = lr / (1 - b1 ** t)
    denom = np.sqrt(v1) / math.sqrt(1 - b2 ** t) + eps
    p1 = p - step_size * m1 / denom
    mabs = b1 * np.abs(m) + (1 - b1) * gabs
    return p1, m1, v1, BOUND * (np.abs(p) + step_size * mabs / denom), BOUND * mabs, BOUND * v1


def sgd_oracle(p, g, b, lr, momentum, dampening, wd, nesterov, t):
    """-> (p', b', bound_p, bound_b), all float64.  t == 1: torch initialises the buffer with the gradient, undamped."""
    p, g, b = (np.asarray(a, dtype=np.float64) for a in (p, g, b))
    g1 = g + wd * p
    gabs = np.abs(g) + wd * np.abs(p)
    if t == 1:
        b1, babs = g1, gabs
    else:
        b1 = momentum * b + (1 - dampening) * g1
        babs = momentum * np.abs(b) + (1 - dampening) * gabs
    d = g1 + momentum * b1 if nesterov else b1
    dabs = gabs + momentum * babs if nesterov else babs
    return p - lr * d, b1, BOUND * (np.abs(p) + lr * dabs), BOUND * babs


def keep_rank_oracle(n, s):
    """ceil((1-s)(n-1)) in double, clamped: numpy's 'higher' percentile index (kws_amd/utils.py:27-28)"""
    return min(max(int(math.ceil((1.0 - float(s)) * (n - 1) - 1e-12)), 0), n - 1)


def threshold_oracle(a, s):
    """-> (th, thresholded copy): th the magnitude of 0-based rank keep_rank; strictly smaller magnitudes go to zero"""
    a = np.asarray(a)
    mag = np.abs(a).reshape(-1)
    th = np.sort(mag)[keep_rank_oracle(mag.size, s)]
    return th, np.where(np.abs(a) < th, np.zeros_like(a), a)


def iht_phase_reference(sparsify, epoch, num_epochs, i_batch, trim_level):
    """trainClassifier.py:251-259, transcribed branch for branch"""
    called = "none"
    if sparsify:
        if epoch >= num_epochs / 3:
            if epoch < (2 * num_epochs) / 3:
                if i_batch % trim_level == 0:
                    called = "threshold"
                else:
                    called = "support"
            else:
                called = "support"
    return called


# ---- threshold cases with the answer typed out: (name, values, s, rank, threshold, result) --------------------------
THRESHOLD_CASES = [
    ("all_equal", [0.5, -0.5, 0.5, -0.5, 0.5], 0.4, 3, 0.5, [0.5, -0.5, 0.5, -0.5, 0.5]),
    ("half_zeros", [0.0, 3.0, -0.0, -2.0, 0.0, 1.0, 0.0, 4.0], 0.5, 4, 1.0, [0.0, 3.0, -0.0, -2.0, 0.0, 1.0, 0.0, 4.0]),
    ("half_zeros_keep_two", [0.0, 3.0, -0.0, -2.0, 0.0, 1.0, 0.0, 4.0], 0.25, 6, 3.0, [0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0]),
    ("s_one_rank_zero", [3.0, -1.0, 2.0, 0.25], 1.0, 0, 0.25, [3.0, -1.0, 2.0, 0.25]),
    ("rank_n_minus_1", [3.0, -1.0, 2.0, 0.25, -5.0], 0.0, 4, 5.0, [0.0, 0.0, 0.0, 0.0, -5.0]),
    ("tiny_s_rank_n_minus_1", [3.0, -1.0, 2.0, 0.25, -5.0], 1e-9, 4, 5.0, [0.0, 0.0, 0.0, 0.0, -5.0]),
    ("n_one", [-0.75], 0.3, 0, 0.75, [-0.75]),
    ("between_ranks_goes_higher", [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 0.5, 3, 4.0, [0.0, 0.0, 0.0, 4.0, 5.0, 6.0]),
]


# ---- seeded operands -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segment(n, t, seed, gscale=1.0):
    """fp32 numpy operands of one segment at step t: p, g, m, v (Adam) and b (SGD).  Step 1 starts from zero state."""
    rng = np.random.default_rng(1000 * seed + n % 997 + 7 * t)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (gscale * rng.standard_normal(n)).astype(np.float32)
    if t == 1:
        m = np.zeros(n, np.float32)
        v = np.zeros(n, np.float32)
        b = np.zeros(n, np.float32)
    else:
        m = (0.3 * gscale * rng.standard_normal(n)).astype(np.float32)
        v = (gscale * gscale * (0.05 + rng.random(n))).astype(np.float32)
        b = (2.0 * gscale * rng.standard_normal(n)).astype(np.float32)
    return p, g, m, v, b


def hyper(algo, wd):
    if algo == "adam":
        return dict(ADAM, weight_decay=wd)
    return dict(SGD, weight_decay=wd, nesterov=(algo == "sgd_nesterov"))


def oracle(algo, wd, t, p, g, m, v, b):
    """-> dict of (value64, bound) per output name: 'p', and 'm', 'v' (Adam) or 'b' (SGD)"""
    h = hyper(algo, wd)
    if algo == "adam":
        p1, m1, v1, bp, bm, bv = adam_oracle(p, g, m, v, lr32(h["lr"]), h["betas"], h["eps"], wd, t)
        return {"p": (p1, bp), "m": (m1, bm), "v": (v1, bv)}
    p1, b1, bp, bb = sgd_oracle(p, g, b, lr32(h["lr"]), h["momentum"], h["dampening"], wd, h["nesterov"], t)
    return {"p": (p1, bp), "b": (b1, bb)}


def torch_cpu_step(algo, wd, t, p, g, m, v, b, dtype=torch.float32):
    """The same step by torch.optim on the CPU (foreach=False) -> dict of numpy outputs named as oracle()'s."""
    h = hyper(algo, wd)
    q = torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dtype))
    q.grad = torch.from_numpy(np.array(g)).to(dtype)
    if algo == "adam":
        opt = torch.optim.Adam([q], foreach=False, **h)
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m)).to(dtype),
                        "exp_avg_sq": torch.from_numpy(np.array(v)).to(dtype)}
        opt.step()
        return {"p": q.detach().numpy(), "m": opt.state[q]["exp_avg"].numpy(), "v": opt.state[q]["exp_avg_sq"].numpy()}
    opt = torch.optim.SGD([q], foreach=False, **h)
    if t > 1:
        opt.state[q] = {"momentum_buffer": torch.from_numpy(np.array(b)).to(dtype)}
    opt.step()
    return {"p": q.detach().numpy(), "b": opt.state[q]["momentum_buffer"].numpy()}


def worst(got, ref):
    """max over the elements of |got - value64| / bound, per output name (a bound of zero allows no error)"""
    out = {}
    for k, (val, bound) in ref.items():
        err = np.abs(np.asarray(got[k], dtype=np.float64) - val)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        out[k] = float(ratio.max())
    return out


# ---- adversarial magnitude sets for the radix select: the values the parameters must hold AFTER the update ----------
ADVERSARIAL = ("all_equal", "two_values", "byte0", "byte1", "byte2", "byte3", "half_zeros")


@functools.lru_cache(maxsize=None)
def adversarial(name, n):
    """fp32 target values (random signs): only the named byte of the magnitude's bit pattern varies, so that radix
    pass alone decides; half_zeros holds +0.0 and -0.0."""
    rng = np.random.default_rng(n + sum(map(ord, name)))
    if name == "all_equal":
        bits = np.full(n, np.float32(0.37).view(np.uint32), dtype=np.uint32)
    elif name == "two_values":
        bits = np.where(rng.random(n) < 0.5, np.float32(0.37).view(np.uint32), np.float32(0.3700001).view(np.uint32))
        bits = bits.astype(np.uint32)
    elif name.startswith("byte"):
        k = int(name[4])
        base = np.uint32(0x3F2A5C17)                                    # 0.66..: every byte non-trivial
        lo, hi = (1, 0x7F) if k == 3 else (0, 256)                      # byte 3: exponents 0x01 .. 0x7e, finite normals
        digit = rng.integers(lo, hi, n).astype(np.uint32)
        bits = (base & ~np.uint32(0xFF << (8 * k))) | (digit << np.uint32(8 * k))
        bits = bits.astype(np.uint32)
    elif name == "half_zeros":
        vals = (0.1 * rng.standard_normal(n)).astype(np.float32)
        vals[rng.permutation(n)[: n // 2]] = 0.0
        bits = vals.view(np.uint32) & np.uint32(0x7FFFFFFF)
    else:
        raise KeyError(name)
    sign = (rng.random(n) < 0.5).astype(np.uint32) << np.uint32(31)
    return (bits | sign).astype(np.uint32).view(np.float32)


def adversarial_operands(target):
    """(p, g) with p - 1 * g == target exactly under SGD at step 1, lr = 1, wd = 0: zeros (of either sign) stay in p with
    g = +0 (fma(-1, +0, p) keeps p's sign of zero), everything else comes from g = -target with p = +0."""
    zero = target == 0
    p = np.where(zero, target, np.float32(0.0)).astype(np.float32)
    g = np.where(zero, np.float32(0.0), -target).astype(np.float32)
    return p, g
