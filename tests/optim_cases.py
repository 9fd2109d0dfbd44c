"""Operands, fp64 oracles and bounds for fastgrnn_hip_optim_update (tests/test_optim_cpu.py, tests/test_hip_optim.py):
RMSprop, Adagrad, Adadelta, Adamax, ASGD and Rprop as torch.optim computes them (foreach=False).

The oracles are the formulas of include/fastgrnn_hip.h in numpy fp64 on the fp32 inputs.  The bounds follow
tests/update_cases.py: with u = 2^-24 an output may differ from the fp64 value by k u times the sum of the MAGNITUDES of
its terms (the update with every term replaced by its absolute value -- not k u times the value: mu b + g'/d, the two
lerps and ax + mu (p' - ax) cancel).

k = 8 wherever the chain of roundings is no longer than Adam's (update_cases.BOUND): RMSprop, Adagrad, Adamax, ASGD,
Rprop.  Two refinements, both from the formulas and not from any result:

* centered RMSprop divides by sqrt(v' - a'^2): the radicand cancels, so the relative error of v' and a'^2 reaches it
  multiplied by (v' + a'^2) / (v' - a'^2), and the term g'/d carries that factor in its bound.  grad_avg is drawn with
  |a| <= 0.5 sqrt(v), which keeps the factor below 1.7 on these operands (1.693 at most; a freely drawn a makes
  v' - a'^2 negative and torch itself returns NaN).
* Adadelta's chain is longer, and its second state squares the result.  Counting first-order roundings of a faithful
  fp32 evaluation without contraction, each relative to the magnitude of its term, weight decay off: g'^2 1, times
  (1-rho) 2, plus rho v (1 on its own term) 3 for v'; + eps 4, the square root halves that and rounds, 3; sqrt(a + eps)
  1.5; the quotient 5.5; times g', Delta = 6.5; p' = p - lr Delta: 8.5 on that term.  Delta^2 doubles: 14, times
  (1-rho) 15, plus rho a 16.  With weight decay g' = g + wd p carries one rounding more, which reaches Delta once
  directly and once through v' (doubled by the square, halved by the root): Delta 8.5, p' 10.5, acc_delta 20.
  Hence k = 16 for p' and for acc_delta without weight decay, k = 20 for acc_delta with it, and the plain 8 for
  square_avg, whose chain is Adam's.  (torch's fp32 step reaches 8.5 u on acc_delta on these operands, 8.1 u at rho = 0.)

Rprop decides by signs: g and prev are drawn with magnitudes above 1e-6, so the fp32 product cannot underflow, with
exact zeros planted in both; prev' is compared exactly and step_size to 8 u (one rounding; torch holds the etas in fp32).
ASGD's next eta and mu are one rounding of a double to fp32 each: 2 u of the value (the rounding, and the double
evaluation's own error orders below it).

Every test that holds the kernel to a bound first asserts torch's fp32 CPU step against the same bound on the same
operands.
"""
import functools

import numpy as np
import torch

from tests import update_cases as U

u = U.U
BOUND = U.BOUND                       # 8 u
K_ADADELTA = 16
K_ADADELTA_ACC_WD = 20
SIZES, STEPS, WDS = U.SIZES, U.STEPS, U.WDS

# rule -> (torch class, constructor arguments, the state keys in the library's slot order (None: slot unused))
RULES = {
    "rmsprop": ("RMSprop", dict(lr=0.01, alpha=0.99, eps=1e-8), ("square_avg", None, None)),
    "rmsprop_mom": ("RMSprop", dict(lr=0.01, alpha=0.99, eps=1e-8, momentum=0.9), ("square_avg", "momentum_buffer", None)),
    "rmsprop_centered": ("RMSprop", dict(lr=0.01, alpha=0.99, eps=1e-8, centered=True), ("square_avg", None, "grad_avg")),
    "rmsprop_centered_mom": ("RMSprop", dict(lr=0.01, alpha=0.99, eps=1e-8, momentum=0.9, centered=True),
                             ("square_avg", "momentum_buffer", "grad_avg")),
    "adagrad": ("Adagrad", dict(lr=0.01, lr_decay=0.0, eps=1e-10), ("sum", None, None)),
    "adagrad_decay": ("Adagrad", dict(lr=0.01, lr_decay=1e-3, eps=1e-10), ("sum", None, None)),
    "adadelta": ("Adadelta", dict(lr=1.0, rho=0.9, eps=1e-6), ("square_avg", "acc_delta", None)),
    "adadelta_rho0": ("Adadelta", dict(lr=1.0, rho=0.0, eps=1e-8), ("square_avg", "acc_delta", None)),   # the reference's default
    "adamax": ("Adamax", dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8), ("exp_avg", "exp_inf", None)),
    "asgd": ("ASGD", dict(lr=0.01, lambd=1e-4, alpha=0.75, t0=1e6), ("ax", None, None)),      # every step below t0: mu = 1
    "asgd_avg": ("ASGD", dict(lr=0.01, lambd=1e-2, alpha=0.75, t0=1.0), ("ax", None, None)),  # steps 3.. above t0: mu < 1
    "rprop": ("Rprop", dict(lr=0.01, etas=(0.5, 1.2), step_sizes=(1e-6, 50.0)), ("prev", "step_size", None)),
}
ALGO = {"RMSprop": 2, "Adagrad": 3, "Adadelta": 4, "Adamax": 5, "ASGD": 6, "Rprop": 7}


def wds_of(rule):
    return (0.0,) if rule == "rprop" else WDS                 # (Rprop takes no weight decay)


CASES = [(rule, t, wd) for rule in RULES for t in STEPS for wd in wds_of(rule)]


def kind(rule):
    return RULES[rule][0]


def keys(rule):
    return [k for k in RULES[rule][2] if k]


def hyper(rule, wd):
    h = dict(RULES[rule][1])
    if rule != "rprop":
        h["weight_decay"] = wd
    return h


def c_hyper(rule, wd):
    from kws_amd import _lib
    h = hyper(rule, wd)
    k = kind(rule)
    vals = {"RMSprop": lambda: (h["alpha"], h["eps"], h.get("momentum", 0.0)),
            "Adagrad": lambda: (h["lr_decay"], h["eps"]),
            "Adadelta": lambda: (h["rho"], h["eps"]),
            "Adamax": lambda: (h["betas"][0], h["betas"][1], h["eps"]),
            "ASGD": lambda: (h["lambd"], h["alpha"], h["t0"]),
            "Rprop": lambda: tuple(h["etas"]) + tuple(h["step_sizes"])}[k]()
    return _lib.OptimHyper(ALGO[k], 1 if h.get("centered") else 0, tuple(float(v) for v in vals), float(wd))


def f32(x):
    return float(np.float32(x))


def asgd_scalars(h, t):
    """(eta, mu) as step t left them, in fp32 (t = 0: the initial lr, 1): torch's formulas, the lr the device sees"""
    if t < 1:
        return f32(h["lr"]), 1.0
    lr = f32(h["lr"])
    return f32(lr / (1.0 + h["lambd"] * lr * t) ** h["alpha"]), f32(1.0 / max(1.0, t - h["t0"]))


# ---- seeded operands ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segment(rule, n, t, seed):
    """fp32 numpy operands of one segment at step t: dict with p, g and the rule's state tensors by torch's keys (ASGD:
    also the floats eta, mu that step t-1 left).  p and g are update_cases.segment's; step 1 starts from the state torch
    creates."""
    p, g, _, v, b = U.segment(n, t, seed)
    rng = np.random.default_rng(500009 + 1000 * seed + n % 997 + 7 * t)
    k, h = kind(rule), RULES[rule][1]
    first = t == 1
    zeros = np.zeros(n, np.float32)
    out = {"p": p, "g": g}
    if k == "RMSprop":
        out["square_avg"] = v
        if "momentum" in h:
            out["momentum_buffer"] = zeros if first else b
        if h.get("centered"):
            out["grad_avg"] = zeros if first else (0.5 * np.sqrt(v) * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    elif k == "Adagrad":
        out["sum"] = zeros if first else (v * np.float32(t - 1)).astype(np.float32)
    elif k == "Adadelta":
        out["square_avg"] = v
        out["acc_delta"] = zeros if first else (0.01 * rng.random(n)).astype(np.float32)
    elif k == "Adamax":
        out["exp_avg"] = zeros if first else (0.3 * rng.standard_normal(n)).astype(np.float32)
        out["exp_inf"] = zeros if first else (0.05 + np.abs(rng.standard_normal(n))).astype(np.float32)
    elif k == "ASGD":
        out["ax"] = zeros if first else (0.1 * rng.standard_normal(n)).astype(np.float32)
        out["eta"], out["mu"] = asgd_scalars(h, t - 1)
    else:
        away = lambda a: np.where(np.abs(a) < 1e-6, np.float32(0.5), a).astype(np.float32)
        g = away(g).copy()
        g[rng.random(n) < 0.05] = 0.0                                      # exact zeros: sign 0, the step size stays
        out["g"] = g
        if first:
            out["prev"], out["step_size"] = zeros, np.full(n, h["lr"], np.float32)
        else:
            prev = away(rng.standard_normal(n).astype(np.float32)).copy()
            prev[rng.random(n) < 0.05] = 0.0
            lo, hi = h["step_sizes"]
            out["prev"] = prev
            out["step_size"] = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32).clip(lo, hi)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- fp64 oracles: -> dict of (value64, bound) per output name ('p' and the state keys; ASGD: 'eta', 'mu' too) ----------
def oracle(rule, wd, t, ops):
    k, h = kind(rule), hyper(rule, wd)
    o = {n: np.asarray(a, dtype=np.float64) for n, a in ops.items()}
    p, g = o["p"], o["g"]
    lr = f32(h["lr"])
    g1 = g + wd * p
    gabs = np.abs(g) + wd * np.abs(p)
    if k == "RMSprop":
        al, eps, mom = h["alpha"], h["eps"], h.get("momentum", 0.0)
        v1 = al * o["square_avg"] + (1 - al) * g1 * g1
        out = {"square_avg": (v1, BOUND * (al * o["square_avg"] + (1 - al) * gabs * gabs))}
        if h.get("centered"):
            a = o["grad_avg"]
            a1 = a + (1 - al) * (g1 - a)
            out["grad_avg"] = (a1, BOUND * (np.abs(a) + (1 - al) * (gabs + np.abs(a))))
            rad = v1 - a1 * a1
            cancel = (v1 + a1 * a1) / rad
        else:
            rad, cancel = v1, 1.0
        d = np.sqrt(rad) + eps
        step, sabs = g1 / d, cancel * gabs / d
        if mom > 0:
            b = o["momentum_buffer"]
            step, sabs = mom * b + step, mom * np.abs(b) + sabs
            out["momentum_buffer"] = (step, BOUND * sabs)
        out["p"] = (p - lr * step, BOUND * (np.abs(p) + lr * sabs))
        return out
    if k == "Adagrad":
        clr = lr / (1 + (t - 1) * h["lr_decay"])
        s1 = o["sum"] + g1 * g1
        d = np.sqrt(s1) + h["eps"]
        return {"sum": (s1, BOUND * (o["sum"] + gabs * gabs)), "p": (p - clr * g1 / d, BOUND * (np.abs(p) + clr * gabs / d))}
    if k == "Adadelta":
        rho, eps = h["rho"], h["eps"]
        v, a = o["square_avg"], o["acc_delta"]
        v1 = rho * v + (1 - rho) * g1 * g1
        ratio = np.sqrt(a + eps) / np.sqrt(v1 + eps)
        dl, dabs = ratio * g1, ratio * gabs
        k_acc = (K_ADADELTA if wd == 0 else K_ADADELTA_ACC_WD) * u
        return {"square_avg": (v1, BOUND * (rho * v + (1 - rho) * gabs * gabs)),
                "acc_delta": (rho * a + (1 - rho) * dl * dl, k_acc * (rho * a + (1 - rho) * dabs * dabs)),
                "p": (p - lr * dl, K_ADADELTA * u * (np.abs(p) + lr * dabs))}
    if k == "Adamax":
        (b1, b2), eps = h["betas"], h["eps"]
        m, un = o["exp_avg"], o["exp_inf"]
        m1 = m + (1 - b1) * (g1 - m)
        mabs = np.abs(m) + (1 - b1) * (gabs + np.abs(m))
        u1 = np.maximum(b2 * un, np.abs(g1) + eps)
        clr = lr / (1 - b1 ** t)
        return {"exp_avg": (m1, BOUND * mabs), "exp_inf": (u1, BOUND * np.maximum(b2 * un, gabs + eps)),
                "p": (p - clr * m1 / u1, BOUND * (np.abs(p) + clr * mabs / u1))}
    if k == "ASGD":
        eta, mu, ax = float(ops["eta"]), float(ops["mu"]), o["ax"]
        p1 = p * (1 - h["lambd"] * eta) - eta * g1
        pabs = np.abs(p) * abs(1 - h["lambd"] * eta) + eta * gabs
        if mu == 1.0:
            ax1, axabs = p1, pabs
        else:
            ax1, axabs = ax + mu * (p1 - ax), np.abs(ax) + mu * (pabs + np.abs(ax))
        eta1 = lr / (1 + h["lambd"] * lr * t) ** h["alpha"]
        mu1 = 1 / max(1.0, t - h["t0"])
        return {"p": (p1, BOUND * pabs), "ax": (ax1, BOUND * axabs),
                "eta": (np.float64(eta1), 2 * u * eta1), "mu": (np.float64(mu1), 2 * u * mu1)}
    (em, ep), (lo, hi) = h["etas"], h["step_sizes"]
    s = np.sign(g * o["prev"])
    st1 = np.clip(o["step_size"] * np.where(s > 0, ep, np.where(s < 0, em, 1.0)), lo, hi)
    g2 = np.where(s < 0, 0.0, g)
    return {"prev": (g2, np.zeros_like(g2)), "step_size": (st1, BOUND * st1),
            "p": (p - np.sign(g2) * st1, BOUND * (np.abs(p) + st1))}


def torch_state(rule, t, ops, dtype=torch.float32):
    """the state dictionary torch.optim holds for a parameter with these operands BEFORE step t (step 1: none yet)"""
    if t == 1 and kind(rule) != "Adagrad":
        return None
    st = {k: torch.from_numpy(np.array(ops[k])).to(dtype) for k in keys(rule)}
    st["step"] = torch.tensor(float(t - 1))
    if kind(rule) == "ASGD":
        st["eta"], st["mu"] = torch.tensor(ops["eta"], dtype=dtype), torch.tensor(ops["mu"], dtype=dtype)
    return st


def torch_cpu_step(rule, wd, t, ops, dtype=torch.float32):
    """The same step by torch.optim on the CPU (foreach=False) -> dict of numpy outputs named as oracle()'s.  torch
    gets the learning rate the device scalar holds (the fp32 value), as the oracle does."""
    h = dict(hyper(rule, wd), lr=f32(RULES[rule][1]["lr"]))
    q = torch.nn.Parameter(torch.from_numpy(np.array(ops["p"])).to(dtype))
    q.grad = torch.from_numpy(np.array(ops["g"])).to(dtype)
    opt = getattr(torch.optim, kind(rule))([q], foreach=False, **h)
    st = torch_state(rule, t, ops, dtype)
    if st is not None:
        opt.state[q] = st
    opt.step()
    out = {"p": q.detach().numpy()}
    out.update({k: opt.state[q][k].numpy() for k in keys(rule)})
    if kind(rule) == "ASGD":
        out.update(eta=np.float64(opt.state[q]["eta"]), mu=np.float64(opt.state[q]["mu"]))
    return out


worst = U.worst
