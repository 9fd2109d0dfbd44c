"""The cases that hold the generic scans (kernel path 0, kws_amd/csrc/kernels_generic.hip) to the oracle at the shapes
only they serve, shared by tests/test_generic_cases_cpu.py (the references against each other, the workspace and LDS
arithmetic against the library; no GPU) and tests/test_hip_generic.py (the kernels against the references).

Three things are restated here from what the kernels hold, not from the launchers' code:

  lds_bytes(d, direction)        the dynamic LDS of a scan: the forward keeps two copies of the state tile [BT, H], the
                                 frame tile [BT, F] and the two rank-space tiles [BT, rw], [BT, ru]; the backward keeps
                                 d_h and d_pre [BT, H] each, the two bias sums [H], d_mh [BT, ru] and two partial sums
                                 per thread.  A direction fits while that is at most LDS_MAX.
  backward_workspace_need(d)     what the backward stores between its kernels: d_pre [T*B, H], two bias partials [nwg, H]
                                 and the scalars' [nwg, 2], mx / d_mx [T*B, rw], mh / d_mh [T*B, ru], and one split-K
                                 partial per SPLITK_CHUNK rows of the LARGEST weight-gradient product it forms (d_w
                                 H x F, d_u H x H, d_w2 H x rw, d_w1 rw x F, d_u2 H x ru, d_u1 ru x H); every buffer
                                 256-byte aligned, as the workspace is.
  forward_workspace_need(d)      the two transposed weight matrices ([rw or F, H] and [ru or H, H]).

TABLE holds the seam cases (sigmoid gate, tanh update), PAIRS the 36 (gate, update) pairs dense and factorised.
build(case) returns the seeded operands, the fp64 numpy oracle's results on them and, for the pairs, what torch
autograd makes of the torch CPU port's forward: a backward that shares nothing with the oracle's hand-written one
(whose algebra, the derivative from the output included, is the kernel's).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import fastgrnn_oracle as O

BT = 8                    # utterances per workgroup of both scans
NTHREADS = 256
LDS_MAX = 160 * 1024      # bytes of LDS one workgroup can hold on gfx950
SPLITK_CHUNK = 2048       # rows of T*B per split-K partial
ROWS_TILED_MAX_N = 64     # launch_rows: N <= 64 takes gemm_rows_tiled, above it the plain gemm_rows
F64 = 1                   # fastgrnn_dtype of fp64 (anything else here is four bytes wide)

NAMES = ["sigmoid", "relu", "tanh", "quantTanh", "quantSigm", "quantSigm4"]
# where a piecewise-linear nonlinearity's derivative jumps, as values of its argument
KINKS = {"relu": (0.0,), "quantTanh": (-1.0, 1.0), "quantSigm": (-1.0, 1.0), "quantSigm4": (-2.0, 2.0)}
KINK_MARGIN = 1e-6

Case = namedtuple("Case", "name T B F H rw ru dtype gate update why")


def _case(T, B, F, H, rw, ru, dtype, why, gate="sigmoid", update="tanh", prefix=""):
    name = "%sT%dB%dF%dH%dr%d-%d-%s" % (prefix, T, B, F, H, rw, ru, dtype)
    return Case(name, T, B, F, H, rw, ru, dtype, gate, update, why)


# ---- the arithmetic of the launchers, restated -------------------------------------------------------------------------

def _es(d):
    return 8 if d.dtype in (F64, "f64") else 4


def _align256(n):
    return -(-n // 256) * 256


def _ranks(d):
    return (d.w_rank, d.u_rank) if hasattr(d, "w_rank") else (d.rw, d.ru)


def lds_bytes(d, direction):
    """dynamic LDS of the forward (direction 0) or backward (1) scan of ``d`` (anything with F, H, w_rank / rw, u_rank /
    ru and dtype)"""
    rw, ru = _ranks(d)
    if direction:
        elems = BT * d.H + BT * d.H + d.H + d.H + BT * ru + 2 * NTHREADS
    else:
        elems = 2 * BT * d.H + BT * d.F + BT * rw + BT * ru
    return elems * _es(d)


def lds_fits(d, direction):
    return lds_bytes(d, direction) <= LDS_MAX


_Shape = namedtuple("_Shape", "F H rw ru dtype")


def largest_h(direction, F, rw, ru, dtype):
    """the largest H whose scan in that direction still fits the LDS (lds_bytes grows with H)"""
    H = 1
    while lds_fits(_Shape(F, H + 1, rw, ru, dtype), direction):
        H += 1
    return H


def products(d):
    """(M, N) of every weight-gradient product the backward forms through the split-K partials"""
    F, H = d.F, d.H
    rw, ru = _ranks(d)
    out = [(H, rw), (rw, F)] if rw else [(H, F)]
    out += [(H, ru), (ru, H)] if ru else [(H, H)]
    return out


def backward_workspace_need(d):
    es, TB = _es(d), d.T * d.B
    nwg = -(-d.B // BT)
    nsplit = -(-TB // SPLITK_CHUNK)
    rw, ru = _ranks(d)
    buffers = [TB * d.H, nwg * d.H, nwg * d.H, nwg * 2, TB * rw, TB * rw, TB * ru, TB * ru,
               nsplit * max(m * n for m, n in products(d))]
    return sum(_align256(n * es) for n in buffers)


def forward_workspace_need(d):
    es = _es(d)
    rw, ru = _ranks(d)
    return _align256((rw or d.F) * d.H * es) + _align256((ru or d.H) * d.H * es)


# ---- the seam cases ----------------------------------------------------------------------------------------------------

H_BOTH_FIT_F64 = min(largest_h(0, 1, 0, 0, F64), largest_h(1, 1, 0, 0, F64))   # F = 1, dense: the backward's limit

TABLE = (
    # H trips: `for (n = tid; n < H; n += nth)` -- one partial wave, two waves, three, a second trip of one unit, of 44
    [_case(3, 9, 13, H, 0, 0, dt, "H trips: H = %d against 64-thread waves / 256 threads" % H)
     for H in (63, 65, 130, 257, 300) for dt in ("f32", "f64")] +
    [_case(3, 9, 13, 520, 0, 0, "f64", "three trips; the fp64 forward takes 67 KiB of LDS, the backward 77 KiB"),
     _case(3, 9, 13, 520, 0, 0, "f32", "three trips in fp32"),
     _case(2, 9, 1, H_BOTH_FIT_F64, 0, 0, "f64", "the largest fp64 H both directions' LDS admits at F = 1: five trips")] +
    # K chunks of gemm_rows_tiled (KC = 64) over H: one chunk and one element, two chunks and two elements
    [_case(3, 9, 13, H, 0, 5, "f32", "ragged last K chunk of mh / dmh: K = H = %d, factorised U" % H) for H in (65, 130)] +
    [_case(3, 9, 13, 130, 0, 5, "f64", "ragged last K chunk in fp64")] +
    # d_x = d_pre . W: N = F on either side of launch_rows' seam, K = H = 24
    [_case(3, 9, F, 24, 0, 0, "f32", "launch_rows N = F = %d (tiled up to 64, plain gemm_rows above)" % F)
     for F in (1, 64, 65, 300)] +
    [_case(3, 9, 65, 24, 0, 0, "f64", "launch_rows N = F = 65 in fp64")] +
    # mx / dmx with N = rw, d_x with K = rw and N = F = 80 (plain); mh / dmh with N = ru
    [_case(3, 9, 80, 72, rw, 0, "f32", "launch_rows N = rw = %d; d_x on gemm_rows with K = rw" % rw) for rw in (1, 64, 65)] +
    [_case(3, 9, 13, 72, 0, ru, "f32", "launch_rows N = ru = %d" % ru) for ru in (1, 64, 65)] +
    [_case(3, 9, 80, 72, 65, 65, "f64", "both ranks past the tiled GEMM's 64 columns, fp64")] +
    # ranks above H: the rw x F / ru x H products are the largest the split-K partials hold
    [_case(3, 5, F, 8, rw, ru, dt, "rank above H: the largest split-K product is a factor's")
     for F, rw, ru in ((32, 16, 0), (13, 0, 20), (32, 16, 20)) for dt in ("f32", "f64")] +
    # split-K: T*B against SPLITK_CHUNK
    [_case(T, B, 13, 24, 0, 0, "f32", "split-K: T*B = %d against chunks of 2048" % (T * B))
     for T, B in ((23, 89), (4, 512), (1, 2049), (2, 2048))] +
    [_case(4, 512, 13, 24, 4, 5, "f32", "split-K: T*B = 2048 exactly, factorised")] +
    # the batch tile
    [_case(2, B, 13, 24, 0, 0, "f32", "B = %d against the tile of 8 utterances" % B) for B in (7, 8, 9)]
)

# the 36 pairs, dense and factorised, fp64
PAIRS = [_case(4, 9, 13, 24, rw, ru, "f64", "pair", gate=g, update=u, prefix="%s.%s-" % (g, u))
         for g in NAMES for u in NAMES for rw, ru in ((0, 0), (4, 5))]
# every update nonlinearity under the sigmoid and the quantSigm gate, dense, in fp32
PAIRS_F32 = [_case(4, 9, 13, 24, 0, 0, "f32", "pair", gate=g, update=u, prefix="%s.%s-" % (g, u))
             for g in ("sigmoid", "quantSigm") for u in NAMES]

BY_NAME = {c.name: c for c in TABLE + PAIRS + PAIRS_F32}
assert len(BY_NAME) == len(TABLE) + len(PAIRS) + len(PAIRS_F32)


# ---- operands and references -------------------------------------------------------------------------------------------

def preactivations(p, x, h0, hs):
    """W.x_t + U.h_{t-1} along the states ``hs``, [T, B, H]"""
    hprev = np.concatenate([h0[None], hs[:-1]], 0)
    return np.stack([O._pre(x[t], hprev[t], p) for t in range(x.shape[0])], 0)


def kink_distance(p, x, h0, gate, update):
    """the smallest distance of any gate / update argument of the sequence from a kink of its nonlinearity, under the
    fp64 oracle (inf where neither is piecewise linear), and per unit [2, H]"""
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x64, h64 = np.asarray(x, np.float64), np.asarray(h0, np.float64)
    hs, _, _ = O.unroll_forward(x64, p64, h64, gate=gate, update=update)
    pre = preactivations(p64, x64, h64, hs)
    H = pre.shape[-1]
    per_unit = np.full((2, H), np.inf)
    for i, (nl, bias) in enumerate(((gate, "bias_gate"), (update, "bias_update"))):
        a = (pre + p64[bias].reshape(1, 1, H)).reshape(-1, H)
        for k in KINKS.get(nl, ()):
            per_unit[i] = np.minimum(per_unit[i], np.abs(a - k).min(axis=0))
    return float(per_unit.min()), per_unit


def keep_off_the_kinks(p, x, h0, gate, update, margin=KINK_MARGIN):
    """Nudge the two biases, unit by unit, until no argument of a piecewise-linear nonlinearity lies within ``margin``
    of a kink (the recurrence moves with the bias, so a few rounds).  Returns the moved copy of ``p``."""
    p = {k: v.copy() for k, v in p.items()}
    for _ in range(50):
        _, per_unit = kink_distance(p, x, h0, gate, update)
        close = per_unit < 2 * margin
        if not close.any():
            return p
        p["bias_gate"][0, close[0]] += p["bias_gate"].dtype.type(64 * margin)
        p["bias_update"][0, close[1]] += p["bias_update"].dtype.type(64 * margin)
    raise AssertionError("could not move %s / %s off the kinks (margin %g)" % (gate, update, margin))


def operands(c):
    """Seeded parameters (seed 5) and data (seed 7) of a case in its dtype.  Matrices are halved, and scaled down further
    where H or F is large, so that pre-activations and states stay O(1) for every nonlinearity."""
    dt = np.float64 if c.dtype == "f64" else np.float32
    p = O.make_params(c.F, c.H, c.rw or None, c.ru or None, dt, seed=5, randomize_scalars=True)
    for k, fan in (("w", c.F), ("w1", c.F), ("u", c.H), ("u1", c.H), ("w2", c.rw), ("u2", c.ru)):
        if k in p:
            p[k] = (0.5 * min(1.0, (64.0 / fan) ** 0.5) * p[k]).astype(dt)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((c.T, c.B, c.F)).astype(dt)
    h0 = (0.5 * rng.standard_normal((c.B, c.H))).astype(dt)
    G = rng.standard_normal((c.T, c.B, c.H)).astype(dt)
    if c.gate in KINKS or c.update in KINKS:
        p = keep_off_the_kinks(p, x, h0, c.gate, c.update)
    return p, x, h0, G


def oracle(p, x, h0, G, gate, update, dtype=np.float64):
    """the numpy oracle run in ``dtype`` on the given values: hs, zs, cs, grads (with the scalar gradients' term sums)"""
    q = {k: np.asarray(v, dtype) for k, v in p.items()}
    x, h0, G = np.asarray(x, dtype), np.asarray(h0, dtype), np.asarray(G, dtype)
    hs, zs, cs = O.unroll_forward(x, q, h0, gate=gate, update=update)
    g = O.unroll_backward(G, x, hs, zs, cs, q, h0, gate=gate, update=update, diagnostics=True)
    return hs, zs, cs, g


def port_autograd(p, x, h0, G, gate, update):
    """hs and every gradient from torch autograd through the torch CPU port's forward, in fp64, in the operator's
    [out, in] layout and under the operator's names"""
    import torch
    from oracle.fastgrnn_torch_port import FastGRNNCellPort, unroll
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    rw, ru = ("w1" in p), ("u1" in p)
    F, H = x.shape[-1], h0.shape[-1]
    cell = FastGRNNCellPort(F, H, gate, update, wRank=p["w1"].shape[0] if rw else None,
                            uRank=p["u1"].shape[0] if ru else None, dtype=torch.float64)
    names = {"w": "W", "u": "U", "w1": "W1", "w2": "W2", "u1": "U1", "u2": "U2"}
    with torch.no_grad():
        for k, attr in names.items():
            if k in p:
                getattr(cell, attr).copy_(t(p[k]).t())         # the port keeps the CPU cell's [in, out]
        for k in ("bias_gate", "bias_update", "zeta", "nu"):
            getattr(cell, k).copy_(t(p[k]))
    xt, ht = t(x).requires_grad_(True), t(h0).requires_grad_(True)
    hs = unroll(cell, xt, ht)
    (hs * t(G)).sum().backward()
    g = {"d_x": xt.grad.numpy(), "d_h0": ht.grad.numpy()}
    for k, attr in names.items():
        if k in p:
            g["d_" + k] = getattr(cell, attr).grad.t().contiguous().numpy()
    for k in ("bias_gate", "bias_update", "zeta", "nu"):
        g["d_" + k] = getattr(cell, k).grad.numpy()
    return hs.detach().numpy(), g


Built = namedtuple("Built", "case p x h0 G hs zs cs grads port_hs port_grads")


@functools.lru_cache(maxsize=None)
def build(name, port=False):
    """The operands of the case and the references on them, computed once: the fp64 oracle, and with ``port`` torch
    autograd through the port.  Callers leave the arrays as they are."""
    c = BY_NAME[name]
    p, x, h0, G = operands(c)
    hs, zs, cs, g = oracle(p, x, h0, G, c.gate, c.update)
    port_hs, port_g = port_autograd(p, x, h0, G, c.gate, c.update) if port else (None, None)
    return Built(c, p, x, h0, G, hs, zs, cs, g, port_hs, port_g)


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|): the measure of tests/support.py's check_grads"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max()) / max(1.0, float(np.abs(ref).max()))


def grad_names(g):
    return [k for k in g if not k.startswith("_")]
