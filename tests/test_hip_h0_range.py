"""The out-of-fp16-range h0 fallback of every split-precision forward kernel family.

A forward scan for a gate that keeps z in [0,1] runs the state product U.h on fp16 two-plane operands unless the
workgroup's 16 rows of h0 fail max|h0| + T + 2 < 3e4 (or hold a NaN); then it runs the three-bf16-plane product: the
scan(std::false_type) arm of fwd_scan_split_w8, the MODE 2 launch of fwd_scan_h256.  FLAG_FWD_BF16X3 selects that
product for the whole call -- the same lambda from the same source -- so a workgroup that falls back must produce the
bits of the FLAG_FWD_BF16X3 run.  tests/h0_range_cases.py is the case table (B = 37: two full tiles and a ragged one;
T = 5, 1 and 2; h0 patterns that put the large values in the ragged tile, in one corner element of a tile, in the
middle tile, at the threshold itself, or make them NaN / inf -- a whole row, or one NaN element); tests/test_h0_range_cases_cpu.py holds the table to the
axes it has to cover.

Per case, for the call `got` with the case's flags:
 (a) on the tiles that fall back, every output (hs, z_s / h_prime_s, the saved pre-activation, h_T) equals, bit for
     bit, the same call with FLAG_FWD_BF16X3;
 (b) on the other tiles it equals, bit for bit, the default-flag call in which the large rows of h0 are zeros (the
     choice is per workgroup and does not leak; every utterance keeps its position);
 (c) sigmoid gate: hs against the fp64 oracle, rel = |a - ref| / max(1, |ref|) <= max(2e-5, 4 rel of the numpy oracle
     in fp32) (+ 2^-8 for a bf16 hs) -- the convention of tests/test_hip_fuzz.py.  quantSigm / quantSigm4 are held to
     (a), (b) and finiteness only: kink crossings between fp32 and fp64 put the same check at 1e-4 .. 7e-4 for them;
 (e) FLAG_SAVE_PREACT: the saved tensor against W.x_t + U.h_{t-1} recomputed in fp64 from the oracle's hs, elementwise
     against the magnitude sum S = |W|.|x_t| + |U|.|h_{t-1}|:  max |pre - pre64| / S <= 4 x the same figure of a numpy
     float32 evaluation of the product;
 the windowed entry points refuse FLAG_FWD_BF16X3: their (a) and (b) is bit-equality with forward_unroll /
 forward_unroll_affine on the gathered windows with the same h0 (and a sentinel block behind hs); (c) and (e) apply.
The low-rank H=256 scan has no fp16 form and is the control (c alone); the backward and the module see hs of order 1e5
under the gradient bound of tests/test_hip_fuzz.py::test_random_configuration_against_the_oracle.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kws_amd import FastGRNNCUDA, _lib, fastgrnn_cuda
from oracle import fastgrnn_oracle as O
from tests import h0_range_cases as HC
from tests import support as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = HC.B
SP, BM, BFT, LAST, X3 = (_lib.FLAG_SAVE_PREACT, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_X_BFT, _lib.FLAG_HS_LAST,
                         _lib.FLAG_FWD_BF16X3)
R = 61                    # rows of the frame pool of the windowed cases
SENTINEL = -7777.0


# ---- operands, computed once and left unchanged ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cell(H, F, rw, ru):
    p = HC.cell_params(H, F, rw, ru)
    e = torch.empty(0)
    P = {k: e for k in ("w", "u", "w1", "w2", "u1", "u2")}
    P.update({k: S.to_dev(v) for k, v in p.items()})
    return p, P


@functools.lru_cache(maxsize=None)
def _scales(H):
    """gate / update scales of the affine cells: around 1, a different factor per block of 16 units"""
    rng = np.random.default_rng(300 + H)
    block = np.repeat(np.array([(0.5, 1.0, 2.0, 0.75, 1.5, 1.0, 0.6, 1.25)[k % 8] for k in range(H // 16)]), 16)
    sg = (block * (1.0 + 0.1 * rng.standard_normal(H))).astype(np.float32)
    sc = (block[::-1] * (1.0 + 0.1 * rng.standard_normal(H))).astype(np.float32)
    return sg, sc, S.to_dev(sg), S.to_dev(sc)


@functools.lru_cache(maxsize=None)
def _pool(F):
    pool = np.random.default_rng(1000 + F).standard_normal((R, F)).astype(np.float32)
    return pool, S.to_dev(pool)


@functools.lru_cache(maxsize=None)
def _starts(T):
    """overlapping, repeated and out of order; both ends of the pool, one of them in the ragged tile"""
    rng = np.random.default_rng(5)
    s = rng.integers(0, R - T + 1, B)
    s[3], s[20], s[36], s[7] = 0, R - T, s[1], min(s[6] + 1, R - T)
    s = s[rng.permutation(B)].astype(np.int32)
    assert s.min() == 0 and s.max() == R - T and (np.diff(s) < 0).any()
    return s, S.to_dev(s)


@functools.lru_cache(maxsize=None)
def _x(F, T, bf16, windows):
    """(the frames the kernels see as float32 numpy [T,B,F], the same as a time-major device tensor of the call's type)"""
    if windows:
        pool, s = _pool(F)[0], _starts(T)[0]
        x = np.stack([pool[s + t] for t in range(T)])
    else:
        x = HC.frames(F)[:T]
    xt = torch.from_numpy(np.ascontiguousarray(x))
    if bf16:
        xt = xt.to(torch.bfloat16)
    return xt.float().numpy(), xt.to(DEV)


def _laid_out(x_tm, layout):
    return {"tm": x_tm, "bm": x_tm.transpose(0, 1), "bft": x_tm.permute(1, 2, 0)}[layout].contiguous()


def _scan(x, p, h0, gate, update, sg=None, sc=None):
    """hs of the cell in the dtype of x: the oracle, or its formula with per-unit pre-activation scales"""
    if sg is None:
        return O.unroll_forward(x, p, h0, gate=gate, update=update)[0]
    dt = x.dtype
    H = h0.shape[1]
    sz, sn = O._sigmoid(p["zeta"].astype(dt)).reshape(()), O._sigmoid(p["nu"].astype(dt)).reshape(())
    h, hs = h0.astype(dt), np.empty((x.shape[0], x.shape[1], H), dt)
    for t in range(x.shape[0]):
        pre = O._pre(x[t], h, p)
        z = O.nonlinearity(sg.astype(dt) * pre + p["bias_gate"].reshape(1, H), gate)
        c = O.nonlinearity(sc.astype(dt) * pre + p["bias_update"].reshape(1, H), update)
        h = (z * h + (sz * (1.0 - z) + sn) * c).astype(dt)
        hs[t] = h
    return hs


@functools.lru_cache(maxsize=None)
def _oracle(H, F, rw, ru, gate, update, affine, bf16, windows, pattern, T):
    """(hs of the fp64 oracle, hs of the same numpy code in fp32), both [T,B,H]; a non-finite row of h0 runs as zeros
    (utterances are independent; that row is judged by itself)"""
    x = _x(F, T, bf16, windows)[0]
    p = HC.cell_params(H, F, rw, ru)
    h0, rows, _ = HC.h0_pattern(pattern, H)
    if pattern.startswith("nonfinite"):
        h0 = h0.copy()
        h0[rows] = 0.0
    sg, sc = _scales(H)[:2] if affine else (None, None)
    hs_o = _scan(x.astype(np.float64), HC.as64(p), h0.astype(np.float64), gate, update,
                 None if sg is None else sg.astype(np.float64), None if sc is None else sc.astype(np.float64))
    hs_32 = _scan(x, p, h0, gate, update, sg, sc)
    assert np.isfinite(hs_o).all() and np.isfinite(hs_32).all()
    return hs_o, hs_32


def _oracle_of(case):
    c = case.cfg
    return _oracle(c.H, c.F, c.rw, c.ru, c.gate, c.update, c.affine, c.bf16, c.entry in ("windows", "train_windows"),
                   case.pattern, case.T)


# ---- calls ----------------------------------------------------------------------------------------------------------
def _forward(c, T, h0, flags, x_tm):
    """forward_unroll / forward_unroll_affine of configuration c with `flags` on time-major frames x_tm: the outputs as
    a list of tensors with the utterance in front ([B,T,H] or [B,H])"""
    _, P = _cell(c.H, c.F, c.rw, c.ru)
    layout = "bft" if flags & BFT else ("bm" if flags & BM else "tm")
    x = _laid_out(x_tm, layout)
    if c.affine:
        _, _, sg, sc = _scales(c.H)
        outs = [fastgrnn_cuda.forward_unroll_affine(x, P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"],
                                                    sg, sc, S.to_dev(h0), _lib.NONLINEARITY[c.gate],
                                                    _lib.NONLINEARITY[c.update], flags=flags)]
    else:
        outs = S.forward_unroll(x, S.to_dev(h0), P, c.gate, update=c.update, want_gates=c.contract == "gates", flags=flags)
    return [_by_utterance(o, flags) for o in outs]


def _by_utterance(o, flags):
    return o if (o.dim() == 2 or flags & BM) else o.transpose(0, 1)


def _output_names(c):
    return {"hs": ["hs"], "gates": ["hs", "z_s", "h_prime_s"], "preact": ["hs", "pre"], "last": ["h_T"]}[c.contract]


def _windows(c, T, h0, flags):
    """one call of fastgrnn_hip_forward_windows into a caller-owned hs with a sentinel block behind it and a NaN tail
    behind the pool; the output with the utterance in front"""
    lib = _lib.load()
    _, P = _cell(c.H, c.F, 0, 0)
    sg, sc = _scales(c.H)[2:] if c.affine else (None, None)
    pool = torch.cat([_pool(c.F)[1], torch.full((T, c.F), float("nan"), device=DEV)])
    starts, h0 = _starts(T)[1], S.to_dev(h0)
    d = _lib.Desc(T, B, c.F, c.H, 0, 0, _lib.NONLINEARITY[c.gate], _lib.NONLINEARITY[c.update], _lib.F32, flags)
    assert lib.fastgrnn_hip_windows_supported(C.byref(d)) == 1
    nbytes = int(lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    shape = (B + 1, c.H) if flags & LAST else ((B + 1, T, c.H) if flags & BM else (T + 1, B, c.H))
    buf = torch.full(shape, SENTINEL, device=DEV)
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())          # noqa: E731
    prm = _lib.Params(ptr(P["w"]), ptr(P["u"]), None, None, None, None, ptr(P["bias_gate"]), ptr(P["bias_update"]),
                      ptr(P["zeta"]), ptr(P["nu"]))
    st = lib.fastgrnn_hip_forward_windows(C.byref(d), C.byref(prm), ptr(sg), ptr(sc), ptr(pool), R, ptr(starts), ptr(h0),
                                          ptr(buf), ptr(ws) if nbytes else None, nbytes,
                                          C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert st == 0, _lib.status_string(st)
    torch.cuda.synchronize()
    hs, tail = (buf[:B], buf[B:]) if flags & (LAST | BM) else (buf[:T], buf[T:])
    assert bool((tail == SENTINEL).all()), "wrote beyond hs"
    assert not bool(torch.isnan(buf).any()), "read beyond the pool"
    return [_by_utterance(hs, flags)]


# ---- checks ---------------------------------------------------------------------------------------------------------
def _check_hs_against_oracle(case, hs, skip_rows=()):
    """(c): hs [B,T,H] or h_T [B,H] of a sigmoid-gate case"""
    c = case.cfg
    hs_o, hs_32 = _oracle_of(case)
    got = hs.to(torch.float64).cpu().numpy()
    if got.ndim == 2:
        ref, ref32 = hs_o[-1], hs_32[-1]
    else:
        got, ref, ref32 = got.transpose(1, 0, 2), hs_o, hs_32
    keep = np.ones(B, bool)
    keep[list(skip_rows)] = False
    got, ref, ref32 = got[..., keep, :], ref[..., keep, :], ref32[..., keep, :]
    rel = lambda a: float((np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max())     # noqa: E731
    lim = max(2e-5, 4.0 * rel(ref32)) + (2.0 ** -8 if hs.dtype == torch.bfloat16 else 0.0)
    print("%s: hs rel %.3g, fp32 oracle %.3g, bound %.3g" % (HC.case_id(case), rel(got), rel(ref32), lim))
    assert rel(got) <= lim, (HC.case_id(case), rel(got), lim)
    return lim


def _check_saved_preactivation(case, pre):
    """(e): the saved tensor [B,T,H] of a dense FLAG_SAVE_PREACT case.  Measured on an MI355X over the 112 such cases of
    the table: the kernels' e lies between 9.7e-8 and 4.3e-7, numpy's float32 figure between 1.8e-7 and 3.1e-7, the
    largest ratio is 1.71 (dense H=256 / F=32, corner_b16_first) against the 4 allowed."""
    c = case.cfg
    p = HC.cell_params(c.H, c.F, c.rw, c.ru)
    x = _x(c.F, case.T, c.bf16, c.entry == "train_windows")[0]
    hs_o = _oracle_of(case)[0]
    h0 = HC.h0_pattern(case.pattern, c.H)[0]
    hprev = np.concatenate([h0[None].astype(np.float64), hs_o[:-1]])
    w, u = p["w"].astype(np.float64), p["u"].astype(np.float64)
    pre64 = x.astype(np.float64) @ w.T + hprev @ u.T
    mag = np.abs(x).astype(np.float64) @ np.abs(w).T + np.abs(hprev) @ np.abs(u).T
    pre32 = x @ p["w"].T + hprev.astype(np.float32) @ p["u"].T
    assert pre32.dtype == np.float32
    e32 = float((np.abs(pre32 - pre64) / mag).max())
    got = pre.to(torch.float64).cpu().numpy().transpose(1, 0, 2)
    e = float((np.abs(got - pre64) / mag).max())
    print("%s: saved pre-activation e %.3g, numpy float32 %.3g" % (HC.case_id(case), e, e32))
    assert e <= 4.0 * e32, (HC.case_id(case), e, e32)


@pytest.mark.parametrize("case", HC.CASES, ids=HC.case_id)
def test_forward_with_h0_outside_the_fp16_range(case):
    c, T = case.cfg, case.T
    h0, rows, falls = HC.h0_pattern(case.pattern, c.H)
    nonfinite = case.pattern.startswith("nonfinite")
    flags = HC.call_flags(c)
    windowed = c.entry in ("windows", "train_windows")
    x_tm = _x(c.F, T, c.bf16, windowed)[1]
    _, P = _cell(c.H, c.F, c.rw, c.ru)
    if c.entry == "windows":
        got = _windows(c, T, h0, flags)
    elif c.entry == "train_windows":
        hs, saved = fastgrnn_cuda.forward_windows_train(_pool(c.F)[1], _starts(T)[1], T, P["w"], P["u"], P["bias_gate"],
                                                        P["bias_update"], P["zeta"], P["nu"], S.to_dev(h0),
                                                        _lib.NONLINEARITY[c.gate], batch_major=bool(flags & BM))
        got = [_by_utterance(hs, flags), _by_utterance(saved, flags)]
    else:
        got = _forward(c, T, h0, flags, x_tm)
    names = _output_names(c)
    assert len(got) == len(names)

    # finiteness: a tile that took the fp16 path with 1e5 in it overflows
    fine = torch.ones(B, dtype=torch.bool, device=DEV)
    if nonfinite:
        fine[rows] = False
    for n, o in zip(names, got):
        assert o.shape[0] == B
        assert bool(torch.isfinite(o[fine].float()).all()), (HC.case_id(case), n, "non-finite output")
        if nonfinite:           # the row stays visible at every step (bf16: tests/test_hip_guards.py, NaN stays NaN)
            bad = o[rows].float()
            assert bool((~torch.isfinite(bad) if case.pattern == "nonfinite_inf" else torch.isnan(bad)).all()), (n, "row lost")

    fallback = torch.zeros(B, dtype=torch.bool, device=DEV)
    if falls:
        for tile in HC.tiles_of(rows):
            fallback[16 * tile:16 * tile + 16] = True
    if c.ref == "x3" and (falls or nonfinite):
        # (nonfinite_nan_element on H=128: the tile keeps the fp16 form -- tests/h0_range_cases.py -- and no tile falls
        # back; the NaN is in its row at every step, above, and every other row is that of the call without it, below)
        x3 = _forward(c, T, h0, flags | X3, x_tm) if falls else got
        h0_small = h0.copy()
        h0_small[rows] = 0.0
        small = _forward(c, T, h0_small, flags, x_tm)
        for n, g, a, b in zip(names, got, x3, small):
            # (a) the same arithmetic as the three-plane call, tile by tile
            S.assert_same_bits(g[fallback & fine], a[fallback & fine],
                               "%s %s: fallback tile differs from FWD_BF16X3" % (HC.case_id(case), n))
            # (b) per workgroup: the other tiles are those of the call without the large rows
            rest = ~fallback & fine
            S.assert_same_bits(g[rest], b[rest], "%s %s: a tile inside the range changed" % (HC.case_id(case), n))
    elif c.ref == "unroll":
        # the windowed scans change addresses, not arithmetic: the bits of the existing forward on the gathered windows
        want = _forward(c, T, h0, flags | (SP if c.entry == "train_windows" else 0), x_tm)
        for n, g, a in zip(names, got, want):
            S.assert_same_bits(g, a, "%s %s: differs from the forward on the gathered windows" % (HC.case_id(case), n))

    if c.gate == "sigmoid":
        _check_hs_against_oracle(case, got[0], rows if nonfinite else ())
    if c.contract == "preact" and not nonfinite:
        _check_saved_preactivation(case, got[1])


@pytest.mark.parametrize("case", HC.BACKWARD_CASES, ids=HC.case_id)
def test_backward_on_hidden_states_of_order_1e5(case):
    """hs feeds the dU GEMM and the z * g chain: every gradient against O.unroll_backward in fp64 under the bound
    expression of tests/test_hip_fuzz.py (tests/test_h0_range_cases_cpu.py: the fp32 oracle alone is inside it)."""
    c, T = case.cfg, case.T
    p, P = _cell(c.H, c.F, 0, 0)
    h0 = HC.h0_pattern(case.pattern, c.H)[0]
    x = _x(c.F, T, False, False)[1]
    G = HC.output_gradient(c.H)
    outs = S.forward_unroll(x, S.to_dev(h0), P, "sigmoid", flags=SP)
    assert float(outs[0].abs().max()) > 1e4
    _check_hs_against_oracle(case, outs[0].transpose(0, 1))
    gr = S.backward_of(outs, S.to_dev(G), x, S.to_dev(h0), P, "sigmoid", flags=SP, biases=True)
    _check_gradients(case, {n: v.cpu().numpy() for n, v in zip(S.GRAD_NAMES[:8], gr)})


def _check_gradients(case, g):
    g_o, g_32, gscale = HC.backward_reference(case.cfg.H, case.cfg.F)
    for k, v in g_o.items():
        if k.startswith("_"):
            continue
        got = g[k].reshape(v.shape)
        err = float(np.abs(got - v).max())
        lim = HC.gradient_limit(k, g_o, g_32, gscale)
        print("%s %s: error %.3g, bound %.3g (max |ref| %.3g)" % (HC.case_id(case), k, err, lim, float(np.abs(v).max())))
        assert np.isfinite(got).all() and err <= lim, (HC.case_id(case), k, err, lim)


def test_module_forward_and_backward_with_a_large_hidden_state():
    """FastGRNNCUDA(32, 256) called with a hiddenState of order 1e5 that wants its gradient (the streaming detector's
    carried state): hs, the loss sum(hs * G) and every gradient against the oracle chain."""
    case = HC.MODULE_CASE
    c, T = case.cfg, case.T
    p, _ = _cell(c.H, c.F, 0, 0)
    m = FastGRNNCUDA(c.F, c.H, device=DEV)
    S.copy_cell_params(m, p)
    x = _x(c.F, T, False, False)[1].clone().requires_grad_(True)
    h0 = S.to_dev(HC.h0_pattern(case.pattern, c.H)[0]).requires_grad_(True)
    G = HC.output_gradient(c.H)
    hs = m(x, h0)
    loss = (hs * S.to_dev(G)).sum()
    loss.backward()
    lim = _check_hs_against_oracle(case, hs.detach().transpose(0, 1))
    hs_o = _oracle_of(case)[0]
    loss_o = float((hs_o * G).sum())
    # Each of the T*B*H terms hs * G may be off by lim * |G| * max(1, |hs|) (the bound hs was just held to).  The terms'
    # errors are roundings of different elements with G of either sign: taken as independent the sum's error has a
    # standard deviation of at most lim times the root-sum-square of those magnitudes; four of them.  (The worst case,
    # every term off the same way, is sqrt(T*B*H) = 218 times the root-sum-square: that bound would hold anything.)
    rss = float(np.sqrt(((G.astype(np.float64) * np.maximum(1.0, np.abs(hs_o))) ** 2).sum()))
    err = abs(float(loss.detach()) - loss_o)
    print("%s loss: error %.3g, bound %.3g (loss %.6g)" % (HC.case_id(case), err, 4.0 * lim * rss, loss_o))
    assert err <= 4.0 * lim * rss, (float(loss.detach()), loss_o, err, 4.0 * lim * rss)
    grads = {"d_x": x.grad, "d_h0": h0.grad, "d_w": m.W.grad, "d_u": m.U.grad, "d_bias_gate": m.bias_gate.grad,
             "d_bias_update": m.bias_update.grad, "d_zeta": m.zeta.grad, "d_nu": m.nu.grad}
    _check_gradients(case, {k: v.cpu().numpy() for k, v in grads.items()})
