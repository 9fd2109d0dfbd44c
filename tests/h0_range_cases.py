"""The case table of tests/test_hip_h0_range.py: which calls are run with an initial state outside fp16's range.

Every split-precision forward scan for a gate that keeps z in [0,1] has two bodies, chosen per workgroup on the device:
the fp16 two-plane state product where the workgroup's 16 rows of h0 satisfy max|h0| + T + 2 < 3e4, and the
three-bf16-plane product otherwise.  A case is a configuration (entry point, shape, gate, sequence type,
output contract, layout) with one pattern of h0 and a sequence length.  No kernel is launched here and nothing in this
module needs a GPU: tests/test_h0_range_cases_cpu.py holds every case's descriptor to kernel path 2 and the table to
the axes each family has to cover.

Families
  A  dense H=128 / F=32 through forward_unroll          B  dense H=128 with F=64 / 256 (the frame product P is a GEMM)
  C  dense H=256 / F=32 (MODE 1 -> MODE 2 launches)      D  dense H=256 with F=64 / 128 (P behind the flag words)
  E  forward_unroll_affine                               F  forward_windows, plain and affine
  G  forward_windows_train                               H  routes through copies (factors multiplied out, zero-extension)
  I  control: the low-rank H=256 scan (no fp16 form)     J  the backward on hs of order 1e5
  K  the module FastGRNNCUDA(32, 256)
"""
import functools
from collections import namedtuple

import numpy as np

from kws_amd import _lib
from oracle import fastgrnn_oracle as O

B = 37                    # two full tiles of 16 utterances and a ragged one of 5
T_DEFAULT = 5             # odd (either parity of the fp16 double buffer) and longer than the t + 2 prefetch clamp
SCALE = 1.0e5             # the large magnitude; U is multiplied by 1 / SCALE so that U.h stays O(1)
SMALL = 0.3               # rows inside fp16's range: SMALL * N(0,1)
NONFINITE_ROW = 3         # in the first tile

# entry: unroll | affine | windows | train_windows | backward | module
# contract: hs (want_gates=False) | gates (the reference's z_s, h_prime_s) | preact (FLAG_SAVE_PREACT) | last (FLAG_HS_LAST)
# layout: tm | bm (FLAG_BATCH_MAJOR) | bft (FLAG_X_BFT)
# ref: x3 (bit-equality with the FLAG_FWD_BF16X3 run, isolation against the run with the large rows zeroed) |
#      unroll (bit-equality with forward_unroll / forward_unroll_affine on the gathered windows) | oracle (fp64 only)
Cfg = namedtuple("Cfg", "family entry H F gate update bf16 contract layout rw ru zext affine ref")
Case = namedtuple("Case", "cfg pattern T")

CORNERS = {"corner_b15_last": (15, -1), "corner_b16_first": (16, 0), "corner_b36_last": (36, -1), "corner_b0_mid": (0, None)}
BASIC = ["ragged_tile"] + list(CORNERS)
EXTRA = ["middle_tile", "threshold_29992", "threshold_29993", "nonfinite_nan", "nonfinite_inf", "nonfinite_nan_element"]
PATTERNS = BASIC + EXTRA
# (the seed of a pattern's small rows: the order in which the patterns were added, so that a new one leaves the data
# of the others as it was)
_SEED = {n: i for i, n in enumerate(sorted(PATTERNS[:-1]) + PATTERNS[-1:])}
BOUNDED_GATES = ("sigmoid", "quantSigm", "quantSigm4")


def cfg(family, H, F, contract="hs", layout="tm", gate="sigmoid", update="tanh", bf16=False, entry="unroll", rw=0, ru=0,
        zext=False, affine=False, ref="x3"):
    return Cfg(family, entry, H, F, gate, update, bf16, contract, layout, rw, ru, zext, affine, ref)


def h0_pattern(name, H, batch=B):
    """(h0 [batch,H] float32, rows that hold a large or non-finite element, whether their tiles take the fallback).
    The signs of the large values are random: the device-side maximum is one of magnitudes."""
    rng = np.random.default_rng(1000 * H + _SEED[name])
    h0 = (SMALL * rng.standard_normal((batch, H))).astype(np.float32)
    big = lambda shape: (SCALE * rng.uniform(0.5, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if name == "ragged_tile":
        rows = list(range(32, batch))
        h0[32:] = big((batch - 32, H))
    elif name in CORNERS:
        b, n = CORNERS[name]
        n = H // 2 if n is None else n % H
        h0[b, n] = SCALE * (-1.0 if (b + n) % 2 else 1.0)
        rows = [b]
    elif name == "middle_tile":
        rows = list(range(16, 32))
        h0[16:32] = big((16, H))
    elif name in ("threshold_29992", "threshold_29993"):
        # with T = 5:  29992 + 5 + 2 = 29999 < 3e4 (the fp16 path at the top of its range);  29993 + 7 = 30000 is not
        h0[20, 5] = -float(name[-5:])
        rows = [20]
    elif name in ("nonfinite_nan", "nonfinite_inf"):
        h0[NONFINITE_ROW] = np.nan if name == "nonfinite_nan" else np.inf
        rows = [NONFINITE_ROW]
    elif name == "nonfinite_nan_element":
        # One NaN among finite values.  fwd_scan_h256 tests every element of h0 and falls back.  fwd_scan_split_w8 (H=128)
        # takes fmaxf over a lane's four units first, which returns the other operand for a NaN: the tile keeps the fp16
        # form.  Either way the row is NaN from the first step on (U.h sums over it) and the other rows are untouched.
        h0[NONFINITE_ROW, 7] = np.nan
        return h0, [NONFINITE_ROW], H > 128
    else:
        raise KeyError(name)
    return h0, rows, name != "threshold_29992"


def _configs():
    c = []
    # A: four contracts, three layouts, both sequence types, the three bounded gates, the quantTanh update
    A = [dict(), dict(contract="gates"), dict(contract="preact"), dict(contract="last"),
         dict(layout="bm"), dict(contract="gates", layout="bm"), dict(contract="preact", layout="bft"),
         dict(contract="last", layout="bft"), dict(bf16=True), dict(bf16=True, contract="preact", layout="bm"),
         dict(gate="quantSigm"), dict(gate="quantSigm", contract="preact", layout="bft"),
         dict(gate="quantSigm4", contract="gates"), dict(gate="quantSigm4", contract="last", layout="bm"),
         dict(gate="quantSigm4", bf16=True), dict(update="quantTanh"), dict(update="quantTanh", contract="preact")]
    c += [cfg("A", 128, 32, **k) for k in A]
    # B: P in the workspace (hs), in c_s (gates), in z_s overwritten in place (preact), in the workspace again (last)
    c += [cfg("B", 128, 64), cfg("B", 128, 64, "gates", "bft"), cfg("B", 128, 64, "preact"), cfg("B", 128, 64, "last"),
          cfg("B", 128, 256, "hs", "bft"), cfg("B", 128, 256, "gates"), cfg("B", 128, 256, "preact", "bft"),
          cfg("B", 128, 256, "last", "bm"), cfg("B", 128, 256, bf16=True), cfg("B", 128, 64, "preact", "bm", bf16=True),
          cfg("B", 128, 64, "preact", gate="quantSigm")]
    # C: the MODE 1 -> MODE 2 pair; under FLAG_X_BFT the transposed copy sits behind the flag words
    c += [cfg("C", 256, 32), cfg("C", 256, 32, "gates"), cfg("C", 256, 32, "preact"), cfg("C", 256, 32, "last"),
          cfg("C", 256, 32, "hs", "bm"), cfg("C", 256, 32, "preact", "bm"), cfg("C", 256, 32, "hs", "bft"),
          cfg("C", 256, 32, "preact", "bft"), cfg("C", 256, 32, "last", "bft"), cfg("C", 256, 32, bf16=True),
          cfg("C", 256, 32, "preact", "bm", bf16=True), cfg("C", 256, 32, gate="quantSigm"),
          cfg("C", 256, 32, "preact", gate="quantSigm4"), cfg("C", 256, 32, "gates", gate="quantSigm4")]
    # D: P behind the flag words
    c += [cfg("D", 256, 64), cfg("D", 256, 64, "preact", "bft"), cfg("D", 256, 64, "last", "bm"),
          cfg("D", 256, 128, "hs", "bft"), cfg("D", 256, 128, "gates"), cfg("D", 256, 128, "preact", "bm"),
          cfg("D", 256, 128, bf16=True), cfg("D", 256, 64, "preact", bf16=True)]
    # E: per-unit scales (H=256: update scales in LDS, gate scales in registers in MODE 0 / 2)
    c += [cfg("E", 128, 32, entry="affine", affine=True), cfg("E", 128, 32, "last", "bm", entry="affine", affine=True),
          cfg("E", 128, 256, "hs", "bft", entry="affine", affine=True), cfg("E", 128, 256, "last", entry="affine", affine=True),
          cfg("E", 256, 32, "hs", "bm", entry="affine", affine=True), cfg("E", 256, 32, "last", entry="affine", affine=True),
          cfg("E", 256, 64, entry="affine", affine=True), cfg("E", 256, 64, "last", "bft", entry="affine", affine=True)]
    # F: the entry point refuses FLAG_FWD_BF16X3: the same bits as the existing forward on the gathered windows
    for H, F in ((128, 32), (256, 32), (256, 64)):
        for affine in (False, True):
            c += [cfg("F", H, F, contract, layout, entry="windows", affine=affine, ref="unroll")
                  for contract, layout in (("hs", "tm"), ("hs", "bm"), ("last", "tm"))]
    # G: the WIN scan that saves the pre-activation (H=256) and the gathered route (H=128)
    c += [cfg("G", 256, 32, "preact", entry="train_windows", ref="unroll"),
          cfg("G", 256, 64, "preact", "bm", entry="train_windows", ref="unroll"),
          cfg("G", 256, 64, "preact", entry="train_windows", ref="unroll"),
          cfg("G", 128, 32, "preact", entry="train_windows", ref="unroll"),
          cfg("G", 128, 32, "preact", "bm", entry="train_windows", ref="unroll")]
    # H: factors multiplied out onto the dense scans; zero-extension (the padded units of h0 are zeros beside 1e5)
    c += [cfg("H", 128, 32, rw=8, ru=8), cfg("H", 256, 32, rw=32, ru=32), cfg("H", 100, 32, zext=True),
          cfg("H", 200, 40, zext=True)]
    return c


CONFIGS = _configs()
CONTROL = cfg("I", 256, 32, rw=16, ru=16, ref="oracle")
BACKWARD = [cfg("J", 128, 32, "preact", entry="backward", ref="oracle"),
            cfg("J", 256, 32, "preact", entry="backward", ref="oracle"),
            cfg("J", 128, 256, "preact", entry="backward", ref="oracle")]
MODULE = cfg("K", 256, 32, "preact", entry="module", ref="oracle")
# middle_tile, threshold and nonfinite: once per kernel file, once more for fwd_scan_h256 under PREIN, and the NaN of
# bf16 outputs on each file
EXTRA_ON = [cfg("A", 128, 32), cfg("C", 256, 32), cfg("D", 256, 64)]
EXTRA_NAN_BF16 = [cfg("A", 128, 32, bf16=True), cfg("C", 256, 32, bf16=True)]
# T = 1 and T = 2 (the prologue's load_x(Tn > 1 ? 1 : 0) and the prefetch clamp): one configuration per kernel family
SHORT_ON = [cfg("A", 128, 32), cfg("B", 128, 64), cfg("C", 256, 32), cfg("D", 256, 64),
            cfg("E", 256, 32, "hs", "bm", entry="affine", affine=True),
            cfg("F", 256, 32, "hs", "tm", entry="windows", ref="unroll"),
            cfg("G", 256, 32, "preact", entry="train_windows", ref="unroll")]


def _cases():
    out = [Case(c, pat, T_DEFAULT) for c in CONFIGS for pat in BASIC]
    out += [Case(c, pat, T_DEFAULT) for c in EXTRA_ON for pat in EXTRA]
    out += [Case(c, "nonfinite_nan", T_DEFAULT) for c in EXTRA_NAN_BF16]
    out += [Case(c, "ragged_tile", T) for c in SHORT_ON for T in (1, 2)]
    out += [Case(CONTROL, "ragged_tile", T_DEFAULT)]
    return out


CASES = _cases()
BACKWARD_CASES = [Case(c, "ragged_tile", T_DEFAULT) for c in BACKWARD]
MODULE_CASE = Case(MODULE, "ragged_tile", T_DEFAULT)
ALL_CASES = CASES + BACKWARD_CASES + [MODULE_CASE]
assert all(c.cfg in CONFIGS for c in CASES if c.cfg is not CONTROL), "EXTRA_ON / SHORT_ON name configurations of the table"


def case_id(case):
    c = case.cfg
    parts = [c.family, c.entry, "H%dF%d" % (c.H, c.F), c.gate, c.contract, c.layout]
    parts += ["uq"] if c.update == "quantTanh" else []
    parts += ["bf16"] if c.bf16 else []
    parts += ["aff"] if c.affine else []
    parts += ["r%d" % c.rw] if c.rw else []
    parts += ["zext"] if c.zext else []
    return "-".join(parts + [case.pattern, "T%d" % case.T])


def call_flags(c):
    """The flags of the call under test (for the windowed entry points: of their descriptor)."""
    f = {"tm": 0, "bm": _lib.FLAG_BATCH_MAJOR, "bft": _lib.FLAG_X_BFT}[c.layout]
    if c.contract == "last":
        f |= _lib.FLAG_HS_LAST
    if c.contract == "preact" and c.entry != "train_windows":       # (the training calls over windows refuse the flag)
        f |= _lib.FLAG_SAVE_PREACT
    if c.affine:
        f |= _lib.FLAG_PREACT_AFFINE
    if c.zext:
        f |= _lib.FLAG_ZERO_EXTEND
    return f


def descriptor(case, extra_flags=0):
    c = case.cfg
    return _lib.Desc(case.T, B, c.F, c.H, c.rw, c.ru, _lib.NONLINEARITY[c.gate], _lib.NONLINEARITY[c.update],
                     _lib.BF16_IO if c.bf16 else _lib.F32, call_flags(c) | extra_flags)


def directions(case):
    return (0, 1) if case.cfg.entry in ("backward", "module") else (0,)


def tiles_of(rows):
    return sorted({r // 16 for r in rows})


# ---- the data of the cases (numpy only; shared by the GPU tests and the CPU check of the backward's bound) ----------
@functools.lru_cache(maxsize=None)
def cell_params(H, F, rw=0, ru=0):
    """O.make_params with randomised scalars; U (its outer factor for a factorised cell) multiplied by 1 / SCALE, as
    tests/test_hip_guards.py does: U.h stays O(1) while |h| is around SCALE."""
    p = O.make_params(F, H, rw or None, ru or None, dtype=np.float32, seed=5 + H + F, randomize_scalars=True)
    k = "u2" if ru else "u"
    p[k] = (p[k] / SCALE).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def frames(F, batch=B):
    """x ~ N(0,1), [T_DEFAULT, batch, F]; shorter cases take its first frames"""
    return np.random.default_rng(77 + F).standard_normal((T_DEFAULT, batch, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def output_gradient(H):
    return np.random.default_rng(99 + H).standard_normal((T_DEFAULT, B, H)).astype(np.float32)


def as64(p):
    return {k: v.astype(np.float64) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def backward_reference(H, F):
    """(gradients of the fp64 oracle with diagnostics, of the oracle run in fp32, max|G|) for family J"""
    p, x, G = cell_params(H, F), frames(F), output_gradient(H)
    h0 = h0_pattern("ragged_tile", H)[0]
    hs_o, zs_o, cs_o = O.unroll_forward(x.astype(np.float64), as64(p), h0.astype(np.float64))
    g_o = O.unroll_backward(G.astype(np.float64), x.astype(np.float64), hs_o, zs_o, cs_o, as64(p), h0.astype(np.float64),
                            diagnostics=True)
    hs_32, zs_32, cs_32 = O.unroll_forward(x, p, h0)
    g_32 = O.unroll_backward(G, x, hs_32, zs_32, cs_32, p, h0)
    return g_o, g_32, float(np.abs(G).max())


def gradient_limit(k, g_o, g_32, gscale, oracle_term=True):
    """the bound expression of tests/test_hip_fuzz.py::test_random_configuration_against_the_oracle"""
    v = g_o[k]
    lim = max(5e-5 * float(np.abs(v).max()), 1e-6 * gscale)
    if k in ("d_zeta", "d_nu"):
        lim = max(lim, 2e-7 * g_o["_abs_" + k[2:]])
    if oracle_term:
        lim = max(lim, 4.0 * float(np.abs(g_32[k].reshape(v.shape) - v).max()))
    return lim
