"""The generic scans (kernel path 0, FLAG_FORCE_GENERIC) against the references at the shapes only they serve: the
cases of tests/generic_cases.py, whose references and margins tests/test_generic_cases_cpu.py holds.

Bounds are those tests/test_hip_parity.py holds this path to: fp64 hidden states and gates to 1e-12, gradients to
1e-10; fp32 hidden states to 1e-5 of max(1, |ref|), gradients to 2e-5 with the scalar-term rule.  Where a long dot
product makes the reference's own lower-precision run lose more (H >= 300 in fp32: the numpy oracle run in fp32; the
largest fp64 H: the oracle against torch autograd through the port), the limit is the larger of the bound and four times
that loss, the rule of tests/test_hip_fuzz.py -- computed from the references alone.  Each case prints its error over
its limit."""
import copy
import warnings

import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import generic_cases as GC
from tests import support as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNCUDA, fastgrnn_cuda

GEN = S.FLAG_FORCE_GENERIC
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}


def _run(b, flags=GEN):
    """forward and backward of a built case through the operators, on path 0 in both directions: the forward's three
    outputs and the backward's twelve"""
    c = b.case
    for direction in (0, 1):
        assert fastgrnn_cuda.kernel_path(c.T, c.B, c.F, c.H, c.rw, c.ru, S.NONLINEARITY[c.gate], S.NONLINEARITY[c.update],
                                         dtype=TORCH_DT[c.dtype], direction=direction, flags=flags) == 0, (c.name, direction)
    outs, grads = S.fwd_bwd(S.to_dev(b.x), S.to_dev(b.h0), S.to_dev(b.G), S.cell_tensors(b.p), c.gate, update=c.update,
                            flags=flags)
    torch.cuda.synchronize()
    assert all(o.dtype == TORCH_DT[c.dtype] for o in outs)
    return outs, grads


def _state_err(got, ref):
    """max |got - ref| / max(1, |ref|), element by element"""
    return float((np.abs(got.cpu().numpy().astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _own_loss(b):
    """What the reference itself loses on the case: for fp32 the numpy oracle run in fp32 against the fp64 one; for fp64
    the oracle against torch autograd through the port.  (state loss, {gradient: absolute loss})"""
    c = b.case
    if c.dtype == "f32":
        hs32, _, _, g32 = GC.oracle(b.p, b.x, b.h0, b.G, c.gate, c.update, np.float32)
        other_hs, other = hs32.astype(np.float64), g32
    else:
        other_hs, other = GC.port_autograd(b.p, b.x, b.h0, b.G, c.gate, c.update)
    state = float((np.abs(other_hs - b.hs) / np.maximum(1.0, np.abs(b.hs))).max())
    return state, {k: float(np.abs(np.asarray(other[k], np.float64).reshape(np.shape(b.grads[k])) - b.grads[k]).max())
                   for k in GC.grad_names(b.grads)}


def _long_dot_product(c):
    return (c.dtype == "f32" and c.H >= 300) or (c.dtype == "f64" and c.H > 1000)


def _check_against(b, outs, grads, ref_grads, tag):
    """the project bounds, or four times the reference's own loss where the case has a long dot product"""
    c = b.case
    f64 = c.dtype == "f64"
    state_tol, grad_tol = (1e-12, 1e-10) if f64 else (1e-5, 2e-5)
    own_state, own = _own_loss(b) if _long_dot_product(c) else (0.0, {})
    report, bad = [], []
    for name, got, ref in (("hs", outs[0], b.hs), ("z", outs[1], b.zs), ("c", outs[2], b.cs)):
        lim = max(state_tol, 4.0 * own_state)
        err = _state_err(got, ref)
        report.append("%s %.2g/%.2g=%.2f%s" % (name, err, lim, err / lim, "" if lim == state_tol else " (4x own loss)"))
        if not err <= lim:
            bad.append(name)
    named = {n: g for n, g in zip(S.GRAD_NAMES, grads) if g.numel()}
    for k in GC.grad_names(ref_grads):
        ref = np.asarray(ref_grads[k], np.float64)
        scale = max(1.0, float(np.abs(ref).max()))
        lim = project = grad_tol * scale
        if not f64 and k in ("d_zeta", "d_nu"):
            lim = project = max(lim, S.SCALAR_TERM_TOL * float(b.grads["_abs_" + k[2:]]))
        lim = max(lim, 4.0 * own.get(k, 0.0))
        err = float(np.abs(named[k].cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max())
        report.append("%s %.2g/%.2g=%.2f%s" % (k, err, lim, err / lim, "" if lim == project else " (4x own loss)"))
        if not err <= lim:
            bad.append(k)
    print("%s lds fwd/bwd %d/%d B: %s" % (tag, GC.lds_bytes(c, 0), GC.lds_bytes(c, 1), "; ".join(report)))
    assert not bad, (tag, bad, report)


@pytest.mark.parametrize("name", [c.name for c in GC.TABLE])
def test_seam_case_against_the_oracle(name):
    b = GC.build(name)
    outs, grads = _run(b)
    if not _long_dot_product(b.case):
        # the project's bounds through the project's checker, as tests/test_hip_parity.py applies them
        f64 = b.case.dtype == "f64"
        S.check_grads(grads, b.grads, tol=1e-10 if f64 else 2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=name)
    _check_against(b, outs, grads, b.grads, name)


@pytest.mark.parametrize("name", [c.name for c in GC.PAIRS])
def test_nonlinearity_pair_in_fp64_against_port_autograd(name):
    """every (gate, update) pair, dense and factorised: hidden states and every gradient against torch autograd through
    the port (no argument is within 1e-6 of a kink, which fp64 cannot cross), z and c against the oracle"""
    b = GC.build(name, True)
    outs, grads = _run(b)
    assert _state_err(outs[0], b.port_hs) <= 1e-12, name
    assert _state_err(outs[1], b.zs) <= 1e-12 and _state_err(outs[2], b.cs) <= 1e-12, name
    errs = S.check_grads(grads, b.port_grads, tol=1e-10, scalar_term_tol=S.SCALAR_TERM_TOL, tag=name)
    assert sorted(errs) == sorted(GC.grad_names(b.grads))
    print("%s: hs %.2g, worst gradient %.2g of 1e-10" % (name, _state_err(outs[0], b.port_hs), max(errs.values())))


@pytest.mark.parametrize("name", [c.name for c in GC.PAIRS_F32])
def test_nonlinearity_pair_in_fp32(name):
    """every update nonlinearity under the sigmoid and the quantSigm gate in fp32.  A piecewise-linear member's derivative
    jumps, and fp32 may land on the other side of a kink than fp64: the backward is then compared with the oracle run on
    the kernel's own z and c (the same mask), as test_quant_tanh_update_on_the_matrix_pipe does."""
    b = GC.build(name)
    c = b.case
    outs, grads = _run(b)
    for got, ref in zip(outs, (b.hs, b.zs, b.cs)):
        assert _state_err(got, ref) <= 1e-5, name
    if c.gate in GC.KINKS or c.update in GC.KINKS:
        hs, zs, cs = (o.cpu().numpy() for o in outs)
        ref = O.unroll_backward(b.G, b.x, hs, zs, cs, b.p, b.h0, gate=c.gate, update=c.update, diagnostics=True)
        errs = S.check_grads(grads, ref, tol=5e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=name)
    else:
        errs = S.check_grads(grads, b.grads, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=name)
    print("%s: worst gradient %.2g" % (name, max(errs.values())))


@pytest.mark.parametrize("name", ["T3B9F13H300r0-0-f32", "T3B9F80H72r65-65-f64", "T4B512F13H24r4-5-f32"])
def test_two_runs_have_the_same_bits(name):
    """no atomics on this path: fixed-order sums in the scan, the split-K partials and their reduction"""
    b = GC.build(name)
    first, second = _run(b), _run(b)
    for what, one, two in (("forward", first[0], second[0]), ("backward", first[1], second[1])):
        for i, (a, a2) in enumerate(zip(one, two)):
            S.assert_same_bits(a, a2, "%s %s output %d" % (name, what, i))


# ---- the modules ---------------------------------------------------------------------------------------------------------

def _module_and_port(F, H, rank, dtype):
    from oracle.fastgrnn_torch_port import FastGRNNCellPort
    torch.manual_seed(3)
    cell = FastGRNNCellPort(F, H, wRank=rank, uRank=rank, dtype=torch.float64)
    with torch.no_grad():
        for n in ("U", "U1"):                                   # keep U.h of 300 units O(1)
            if hasattr(cell, n):
                getattr(cell, n).mul_(0.4)
        cell.bias_gate.add_(0.3 * torch.randn_like(cell.bias_gate)); cell.zeta.fill_(0.4); cell.nu.fill_(-3.0)
        if dtype == torch.float32:                              # the port keeps the fp32 values, in fp64
            for p in cell.parameters():
                p.copy_(p.float().double())
    m = FastGRNNCUDA(F, H, wRank=rank, uRank=rank, device=S.DEV).to(dtype)
    with torch.no_grad():
        for n in ("W", "U", "W1", "W2", "U1", "U2"):           # the port keeps the CPU cell's [in, out]
            if hasattr(cell, n):
                getattr(m, n).copy_(getattr(cell, n).t().to(dtype))
        for n in ("bias_gate", "bias_update", "zeta", "nu"):
            getattr(m, n).copy_(getattr(cell, n).to(dtype))
    return m, cell


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rank", [None, 70], ids=["dense", "r70"])
def test_module_beyond_the_fast_paths_against_port_autograd(rank, dtype):
    """FastGRNNCUDA(F = 20, H = 300), dense and with both ranks 70: forward and autograd backward against torch autograd
    through the port in fp64 (on the module's values)"""
    from oracle.fastgrnn_torch_port import unroll
    T, B, F, H = 5, 11, 20, 300
    m, cell = _module_and_port(F, H, rank, dtype)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(T, B, F, generator=g).to(dtype)
    G = torch.randn(T, B, H, generator=g).to(dtype)
    names = ("W1", "W2", "U1", "U2") if rank else ("W", "U")

    def port_run(cell, dt):
        xc = x.detach().clone().to(dt).requires_grad_(True)
        hs_c = unroll(cell, xc)
        (hs_c * G.to(dt)).sum().backward()
        g = {"d_x": xc.grad.double().numpy()}
        g.update({"d_" + n: getattr(cell, n).grad.t().contiguous().double().numpy() for n in names})
        g.update({"d_" + n: getattr(cell, n).grad.double().numpy() for n in ("bias_gate", "bias_update", "zeta", "nu")})
        return hs_c.detach().double().numpy(), g

    hs_ref, ref = port_run(cell, torch.float64)
    xg = x.detach().clone().to(S.DEV).requires_grad_(True)
    hs_g = m(xg)
    (hs_g * G.to(S.DEV)).sum().backward()
    torch.cuda.synchronize()
    assert hs_g.dtype == dtype and xg.is_leaf
    f64 = dtype == torch.float64
    state_tol, grad_tol = (1e-12, 1e-10) if f64 else (1e-5, 2e-5)
    own_state, own = 0.0, {}
    if not f64:                  # H = 300 in fp32: what the port itself loses when it runs in fp32 (see the module docstring)
        hs32, g32 = port_run(copy.deepcopy(cell).float(), torch.float32)
        own_state = float((np.abs(hs32 - hs_ref) / np.maximum(1.0, np.abs(hs_ref))).max())
        own = {k: float(np.abs(g32[k] - ref[k]).max()) for k in ref}
    err = _state_err(hs_g.detach(), hs_ref)
    assert err <= max(state_tol, 4.0 * own_state), (err, own_state)
    got = {"d_x": xg.grad}
    got.update({"d_" + n: getattr(m, n).grad for n in names + ("bias_gate", "bias_update", "zeta", "nu")})
    report, bad = [], []
    for k, r in ref.items():
        lim = max(grad_tol * max(1.0, float(np.abs(r).max())), 4.0 * own.get(k, 0.0))
        e = float(np.abs(got[k].cpu().double().numpy().reshape(r.shape) - r).max())
        report.append("%s %.2g/%.2g" % (k, e, lim))
        if not e <= lim:
            bad.append(k)
    print("module rank %s %s: hs %.2g; %s" % (rank, dtype, err, "; ".join(report)))
    assert not bad, (bad, report)


def test_module_warns_once_per_signature_that_it_runs_on_the_generic_scan():
    T, B, F, H = 8, 520, 20, 300                      # (the warning is for T * B >= 4096: a size where the cliff matters)
    m, _ = _module_and_port(F, H, None, torch.float32)
    x = torch.randn(T, B, F, generator=torch.Generator().manual_seed(1)).to(S.DEV)
    x512 = x[:, :512].contiguous()
    fastgrnn_cuda._cliff_warned.clear()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with torch.no_grad():
            for _ in range(3):
                m(x512)
            m(x)
            m(x512)
    torch.cuda.synchronize()
    msgs = [str(w.message) for w in seen if "runs on the generic" in str(w.message)]
    assert len(msgs) == 2 and all("forward" in s_ and "H=300" in s_ for s_ in msgs), msgs
    assert "B=512" in msgs[0] and "B=520" in msgs[1], msgs


def test_module_outside_the_lds_limit_raises_and_leaves_the_device_clean():
    H = GC.largest_h(0, 1, 0, 0, "f64") + 1           # the fp64 forward no longer fits
    m = FastGRNNCUDA(1, H, device=S.DEV).double()
    x = torch.zeros(2, 3, 1, dtype=torch.float64, device=S.DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        m(x)
    torch.cuda.synchronize()
    # the backward's limit is lower: a training step at the largest forward H is refused in its backward, with nothing run
    m = FastGRNNCUDA(1, H - 1, device=S.DEV).double()
    hs = m(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="not supported"):
        hs.sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hs).all())
