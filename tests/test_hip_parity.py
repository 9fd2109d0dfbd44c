"""GPU parity tests: the HIP path (through the C ABI via kws_amd.fastgrnn_cuda) against
(a) the committed golden vectors produced by the reference's own CPU cell and
(b) the numpy oracle on seeded inputs, plus size-independent properties at the
BASELINE.json sizes.  Run with ``-m gpu`` on an MI355X.

Tolerances (north_star: 1e-5 fp32 against the reference's CPU path):
  * hidden states fp32: max|d| <= 1e-5 absolute (|h| <~ 2).
  * gradients fp32: max|d| / max(1, max|ref|) <= 2e-5.  Gradients are sums over up to
    T*B terms whose fp32 summation order differs from ATen's; the reference's own fp32
    CPU result differs from its fp64 result by the same order (checked below).
  * fp64: 1e-12 / 1e-10.
  * d_zeta / d_nu in fp32: additionally 2e-7 of the sum of their terms' magnitudes (S.SCALAR_TERM_TOL).

How a bound becomes a limit -- the one gradient checker, the scalar-term rule and its justification -- is in
tests/support.py; each call below states its own bound.
"""
import zlib

import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import layer_cases as LC
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNCUDA, FastGRNNCUDACell, fastgrnn_cuda


def run_hip(x, h0, G, p, gate="sigmoid", update="tanh", flags=0):
    """forward_unroll + backward_unroll through the operator module; numpy in/out."""
    (hs, zs, cs), outs = S.fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), S.cell_tensors(p), gate, update=update,
                                   flags=flags)
    torch.cuda.synchronize()
    g = {n: o.cpu().numpy() for n, o in zip(S.GRAD_NAMES, outs) if o.numel()}
    return hs.cpu().numpy(), zs.cpu().numpy(), cs.cpu().numpy(), g


@pytest.mark.parametrize("flags", [0, S.FLAG_FORCE_F32_MFMA, S.FLAG_FORCE_GENERIC], ids=["dispatch", "f32mfma", "generic"])
def test_golden_vectors(golden, flags):
    """HIP vs the reference CPU cell's own outputs (tests/golden/*.npz)."""
    f64 = golden["dtype"] == "f64"
    hs, zs, cs, g = run_hip(golden["x"], golden["h0"], golden["G"], golden["params"],
                            golden["gate"], golden["update"], flags)
    assert np.abs(hs - golden["hs"]).max() <= (1e-12 if f64 else 1e-5), golden["name"]
    ref = dict(golden["dparams"]); ref["d_x"] = golden["dx"]; ref["d_h0"] = golden["dh0"]
    if not f64:     # the sums of |terms| of d_zeta / d_nu, which the fixtures do not carry
        g_o = S.oracle64(golden["x"], golden["G"], golden["params"], golden["h0"], golden["gate"], golden["update"])[3]
        ref["_abs_zeta"], ref["_abs_nu"] = g_o["_abs_zeta"], g_o["_abs_nu"]
    S.check_grads(g, ref, tol=1e-10 if f64 else 2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=golden["name"])


CASES = [
    # T, B, F, H, rw, ru, gate
    (99, 64, 32, 128, 0, 0, "sigmoid"),     # config (1) plumbing shape
    (99, 50, 32, 128, 0, 0, "sigmoid"),     # ragged against the 16-utterance tile
    # tanh / relu gates are not contractive (|z| is not < 1): rounding differences are
    # amplified step over step and a relu-gated state overflows within tens of frames, so
    # these cases stay short -- they test the arithmetic, not fp32 chaos
    (12, 50, 32, 128, 0, 0, "tanh"),
    (6, 33, 32, 128, 0, 0, "relu"),
    (99, 32, 32, 256, 16, 16, "sigmoid"),   # config (4) shape, small batch
    (9, 5, 13, 24, 0, 3, "sigmoid"),
    (5, 5, 13, 24, 4, 0, "relu"),
    (3, 1, 1, 1, 0, 0, "sigmoid"),          # degenerate sizes
    (1, 7, 32, 128, 0, 0, "sigmoid"),       # T = 1
    (2, 1, 32, 128, 0, 0, "sigmoid"),       # one utterance, even T (no virtual pairing step)
    (3, 16, 32, 128, 0, 0, "tanh"),         # exactly one full tile, odd T
    (2, 17, 32, 256, 16, 16, "sigmoid"),    # low-rank kernels: ragged second tile, T = 2
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%dB%dF%dH%dr%d-%d%s" % c)
@pytest.mark.parametrize("flags", [0, S.FLAG_FORCE_F32_MFMA, S.FLAG_FORCE_GENERIC], ids=["dispatch", "f32mfma", "generic"])
def test_seeded_vs_oracle_fp32(case, flags):
    T, B, F, H, rw, ru, gate = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    p = O.make_params(F, H, rw or None, ru or None, np.float32, seed=11, randomize_scalars=True)
    if gate == "relu":
        # keep z = relu(pre + b_z) around 0..1 so the state does not blow up by 1e8 in 6 frames
        for k in ("w", "u", "w1", "w2", "u1", "u2"):
            if k in p:
                p[k] = (0.3 * p[k]).astype(np.float32)
        p["bias_gate"] = (0.3 * p["bias_gate"] - 0.1).astype(np.float32)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    if gate == "relu":
        p = S.keep_relu_gates_off_the_kink(p, x, h0)
    hs, zs, cs, g = run_hip(x, h0, G, p, gate, flags=flags)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0, gate)
    # 1e-5 absolute while |h| <= 1, relative beyond (a tanh/relu gate does not bound h)
    assert (np.abs(hs - hs_o) / np.maximum(1.0, np.abs(hs_o))).max() <= 1e-5
    assert (np.abs(zs - zs_o) / np.maximum(1.0, np.abs(zs_o))).max() <= 1e-5 and np.abs(cs - cs_o).max() <= 1e-5
    # relu included: its derivative jumps at zero, but no gate pre-activation of these cases comes within 1e-4 of the
    # kink (S.keep_relu_gates_off_the_kink), 1e2 times what fp32 and fp64 can differ by there -- the masks agree, and the
    # comparison is the fp64 one of every other gate.  (Round 2 compared the relu cases with the oracle run in fp32 on
    # the kernel's OWN z: a same-mask self-consistency check.)
    S.check_grads(g, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=case)


@pytest.mark.parametrize("lowrank", [False, True])
def test_seeded_vs_oracle_fp64(lowrank):
    T, B, F, H = 12, 9, 10, 24
    rng = np.random.default_rng(3)
    p = O.make_params(F, H, 4 if lowrank else None, 5 if lowrank else None, np.float64, seed=5, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)); h0 = 0.5 * rng.standard_normal((B, H)); G = rng.standard_normal((T, B, H))
    hs, zs, cs, g = run_hip(x, h0, G, p)
    hs_o, zs_o, cs_o = O.unroll_forward(x, p, h0)
    g_o = O.unroll_backward(G, x, hs_o, zs_o, cs_o, p, h0)
    assert np.abs(hs - hs_o).max() <= 1e-12
    S.check_grads(g, g_o, tol=1e-10, scalar_term_tol=S.SCALAR_TERM_TOL, tag="fp64")


@pytest.mark.parametrize("B", [64, 45, 1, 16])
def test_preact_mode_vs_oracle(B):
    """FLAG_SAVE_PREACT (kernel path 2): forward saves W.x+U.h only; backward recomputes z, h_prime."""
    T, F, H = 99, 32, 128
    if fastgrnn_cuda.kernel_path(T, B, F, H, direction=1) != 2:
        pytest.skip("split-precision path not dispatched for this shape")
    rng = np.random.default_rng(21)
    p = O.make_params(F, H, dtype=np.float32, seed=13, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    (hs, pre), outs = S.fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), S.cell_tensors(p), "sigmoid",
                                flags=S.FLAG_SAVE_PREACT, biases=True)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(hs.cpu().numpy() - hs_o).max() <= 1e-5
    assert np.abs(pre.cpu().numpy() - S.dense_preactivation64(x, p, h0, hs_o)).max() <= 1e-5
    S.check_grads(outs, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag="preact")


@pytest.mark.parametrize("T,B,gate,rw,ru", [(1, 16, 0, 16, 16), (6, 37, 0, 16, 16), (7, 64, 0, 16, 16), (9, 130, 0, 16, 16),
                                            (4, 21, 1, 16, 16), (5, 48, 2, 16, 16), (7, 37, 0, 8, 8), (6, 64, 0, 16, 8),
                                            (5, 33, 2, 5, 12), (4, 16, 0, 1, 1)])
def test_lowrank_preact_contract_vs_oracle(T, B, gate, rw, ru):
    """config-(4) shape (H=256, wRank=uRank=16) and the other ranks up to 16 (rnn.py:783-798; zero-extended to 16 in
    the kernels) under FLAG_SAVE_PREACT: the forward saves the pre-activation and the rank-space vector
    [U1.h | W1.x]; the backward is the split-precision low-rank scan + split-K weight-gradient GEMMs.  All twelve
    outputs against the fp64 oracle."""
    F, H = 32, 256
    GN = ["sigmoid", "relu", "tanh"]
    rng = np.random.default_rng(300 + T + B)
    p = O.make_params(F, H, rw, ru, dtype=np.float32, seed=17, randomize_scalars=True)
    if gate == 1:      # relu gate: keep z around 0..1 (see test_seeded_vs_oracle_fp32)
        for k in ("w1", "w2", "u1", "u2"):
            p[k] = (0.55 * p[k]).astype(np.float32)     # the product of two factors scales by 0.3
        p["bias_gate"] = (0.3 * p["bias_gate"] - 0.1).astype(np.float32)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, rw, ru, gate, direction=1, flags=S.FLAG_SAVE_PREACT) == 2
    assert fastgrnn_cuda.kernel_path(T, B, F, H, rw, ru, gate, direction=1) != 2
    (hs, pre, m), outs = S.fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), S.cell_tensors(p), gate,
                                   flags=S.FLAG_SAVE_PREACT, biases=True)
    assert m.shape == (T * B, 32)                 # [U1.h | W1.x], each zero-extended to 16 columns, time-major
    m4 = m.cpu().numpy().reshape(T, B, 32)
    assert not m4[..., ru:16].any() and not m4[..., 16 + rw:].any()
    m_k = np.concatenate([m4[..., :ru], m4[..., 16:16 + rw]], -1)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    x64, h64 = x.astype(np.float64), h0.astype(np.float64)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0, GN[gate])
    hprev = np.concatenate([h64[None], hs_o[:-1]], 0)
    m_o = np.concatenate([hprev @ p64["u1"].T, x64 @ p64["w1"].T], -1)
    pre_o = m_o[..., ru:] @ p64["w2"].T + m_o[..., :ru] @ p64["u2"].T
    rel = lambda a, ref: (np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max()
    assert rel(hs.cpu().numpy(), hs_o) <= 1e-5
    assert rel(m_k, m_o) <= 1e-5
    assert rel(pre.cpu().numpy(), pre_o) <= 1e-5
    tol = 2e-5
    if gate == 1:      # same mask as the HIP path: the oracle in fp32 on the kernel's own states
        hsn = hs.cpu().numpy()
        zk = np.maximum(pre.cpu().numpy() + p["bias_gate"], 0).astype(np.float32)
        ck = np.tanh(pre.cpu().numpy() + p["bias_update"]).astype(np.float32)
        g_o = O.unroll_backward(G, x, hsn, zk, ck, p, h0, gate=GN[gate])
        tol = 5e-5
    assert outs[6].numel() == 0 and outs[7].numel() == 0
    S.check_grads(outs, g_o, tol=tol, scalar_term_tol=S.SCALAR_TERM_TOL, tag="lowrank-preact")


def test_single_step_operators():
    """forward / backward (fastgrnn_cuda.cpp:73-145) == T=1 oracle."""
    B, F, H = 37, 32, 128
    rng = np.random.default_rng(8)
    p = O.make_params(F, H, dtype=np.float32, seed=2, randomize_scalars=True)
    x = rng.standard_normal((B, F)).astype(np.float32)
    h = rng.standard_normal((B, H)).astype(np.float32)
    G = rng.standard_normal((B, H)).astype(np.float32)
    P = S.cell_tensors(p)
    new_h, z, c = fastgrnn_cuda.forward(S.to_dev(x), P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"],
                                        S.to_dev(h), 0, P["w1"], P["w2"], P["u1"], P["u2"])
    outs = fastgrnn_cuda.backward(S.to_dev(G), S.to_dev(x), S.to_dev(h), P["zeta"], P["nu"], P["w"], P["u"], z, c,
                                  P["w1"], P["w2"], P["u1"], P["u2"], 0)
    assert len(outs) == 12 and outs[8].numel() == 0 and outs[6].shape == (H, F) and outs[0].shape == (B, F)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    hs_o, zs_o, cs_o = O.unroll_forward(x[None].astype(np.float64), p64, h.astype(np.float64))
    g_o = O.unroll_backward(G[None].astype(np.float64), x[None].astype(np.float64), hs_o, zs_o, cs_o, p64, h.astype(np.float64))
    assert np.abs(new_h.cpu().numpy() - hs_o[0]).max() <= 1e-5
    assert np.abs(outs[0].cpu().numpy() - g_o["d_x"][0]).max() <= 2e-5
    assert np.abs(outs[5].cpu().numpy() - g_o["d_h0"]).max() <= 2e-5
    assert np.abs(outs[7].cpu().numpy() - g_o["d_u"]).max() <= 2e-5 * max(1, np.abs(g_o["d_u"]).max())


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("lowrank", [False, True, "config4", "dense256", "dense256f64"])
def test_module_autograd_matches_cpu_port(batch_first, lowrank):
    """FastGRNNCUDA (rnn.py:738-826) forward+autograd vs the torch CPU port of
    FastGRNNCell + BaseRNN loop (the reference's CPU path)."""
    from oracle.fastgrnn_torch_port import FastGRNNCellPort, unroll
    T, B, F, H = 30, 21, 32, 128
    torch.manual_seed(0)
    rw = ru = 8 if lowrank else None
    if lowrank == "config4":             # BASELINE configs[3] shape: the low-rank split-precision kernels
        H, rw, ru = 256, 16, 16
    if lowrank in ("dense256", "dense256f64"):   # the default stack's first layer (trainingConfig.py:12-15, :36): the
        F = 64 if lowrank == "dense256f64" else F    # H = 256 scans, [B,T,.] indexed in place under batch_first
        H, rw, ru, lowrank = 256, None, None, False
    if H == 256 and rw is None and batch_first:
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=S.FLAG_SAVE_PREACT | S.FLAG_BATCH_MAJOR) == 2
    cell = FastGRNNCellPort(F, H, wRank=rw, uRank=ru)
    with torch.no_grad():
        cell.bias_gate.add_(0.3 * torch.randn_like(cell.bias_gate)); cell.zeta.fill_(0.4); cell.nu.fill_(-3.0)
    m = FastGRNNCUDA(F, H, wRank=rw, uRank=ru, batch_first=batch_first, device=DEV)
    with torch.no_grad():
        if lowrank:
            m.W1.copy_(cell.W1.t()); m.W2.copy_(cell.W2.t()); m.U1.copy_(cell.U1.t()); m.U2.copy_(cell.U2.t())
        else:
            m.W.copy_(cell.W.t()); m.U.copy_(cell.U.t())
        m.bias_gate.copy_(cell.bias_gate); m.bias_update.copy_(cell.bias_update)
        m.zeta.copy_(cell.zeta); m.nu.copy_(cell.nu)
    x = torch.randn(T, B, F)
    G = torch.randn(T, B, H)
    xc = x.clone().requires_grad_(True)
    hs_c = unroll(cell, xc)
    (hs_c * G).sum().backward()
    xg = (x.transpose(0, 1).contiguous() if batch_first else x).to(DEV).requires_grad_(True)
    hs_g = m(xg)
    Gg = (G.transpose(0, 1) if batch_first else G).to(DEV)
    (hs_g * Gg).sum().backward()
    hs_gn = hs_g.detach().cpu()
    if batch_first:
        assert hs_gn.shape == (B, T, H)
        hs_gn = hs_gn.transpose(0, 1)
    assert (hs_gn - hs_c.detach()).abs().max() <= 1e-5
    dx = xg.grad.cpu()
    if batch_first:
        dx = dx.transpose(0, 1)
    assert (dx - xc.grad).abs().max() <= 2e-5
    pairs = ([(m.W1, cell.W1), (m.W2, cell.W2), (m.U1, cell.U1), (m.U2, cell.U2)] if lowrank
             else [(m.W, cell.W), (m.U, cell.U)])
    for a, b in pairs:
        scale = max(1.0, float(b.grad.abs().max()))
        assert (a.grad.cpu() - b.grad.t()).abs().max() / scale <= 2e-5
    for a, b in ((m.bias_gate, cell.bias_gate), (m.bias_update, cell.bias_update), (m.zeta, cell.zeta), (m.nu, cell.nu)):
        scale = max(1.0, float(b.grad.abs().max()))
        assert (a.grad.cpu() - b.grad).abs().max() / scale <= 2e-5


def test_cell_module_single_step_autograd():
    B, F, H = 8, 32, 128
    torch.manual_seed(1)
    c = FastGRNNCUDACell(F, H, device=DEV)
    x = torch.randn(B, F, device=DEV, requires_grad=True)
    h = torch.randn(B, H, device=DEV, requires_grad=True)
    out = c(x, h)
    out.sum().backward()
    W, U = c.W.detach().cpu().double(), c.U.detach().cpu().double()
    xd, hd = x.detach().cpu().double(), h.detach().cpu().double()
    pre = xd @ W.t() + hd @ U.t()
    z = torch.sigmoid(pre + 1.0); cc = torch.tanh(pre + 1.0)
    ref = z * hd + (torch.sigmoid(torch.tensor(1.0).double()) * (1 - z) + torch.sigmoid(torch.tensor(-4.0).double())) * cc
    assert (out.detach().cpu().double() - ref).abs().max() <= 1e-5
    assert x.grad is not None and h.grad is not None and c.U.grad.shape == (H, H)


def test_error_behaviour_mirrors_check_input():
    """fastgrnn_cuda.cpp:69-71: non-CUDA / non-contiguous operands raise RuntimeError."""
    F, H, T, B = 32, 128, 4, 6
    p = O.make_params(F, H)
    P = S.cell_tensors(p)
    x = torch.randn(T, B, F, device=DEV)
    h0 = torch.zeros(B, H, device=DEV)
    args = lambda xx, hh: (xx, P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"], hh, 0,
                           P["w1"], P["w2"], P["u1"], P["u2"])
    with pytest.raises(RuntimeError, match="contiguous"):
        fastgrnn_cuda.forward_unroll(*args(torch.randn(B, T, F, device=DEV).transpose(0, 1), h0))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fastgrnn_cuda.forward_unroll(*args(x.cpu(), h0))
    with pytest.raises(RuntimeError, match="shape"):
        fastgrnn_cuda.forward_unroll(*args(x, torch.zeros(B + 1, H, device=DEV)))
    with pytest.raises(RuntimeError, match="nonlinearity"):
        fastgrnn_cuda.forward_unroll(x, P["w"], P["u"], P["bias_gate"], P["bias_update"], P["zeta"], P["nu"], h0, 17,
                                     P["w1"], P["w2"], P["u1"], P["u2"])


def test_runs_on_current_stream_and_is_reentrant():
    """Launches go to torch's current stream (reference used the legacy default stream,
    SURVEY section 0.5): two side streams produce the same result as the default stream."""
    T, B, F, H = 20, 40, 32, 128
    p = O.make_params(F, H, seed=4)
    P = S.cell_tensors(p)
    x = torch.randn(T, B, F, device=DEV)
    h0 = torch.zeros(B, H, device=DEV)
    call = lambda: S.forward_unroll(x, h0, P, "sigmoid")[0]
    base = call()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(call())
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, base)


# ---- BASELINE.json sizes: size-independent properties --------------------------------------

def _northstar(B, seed=0):
    T, F, H = 99, 32, 128
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, F, generator=g).to(DEV)
    G = torch.randn(T, B, H, generator=g).to(DEV)
    p = O.make_params(F, H, seed=seed)
    return x, G, p, S.cell_tensors(p)


def _fwd(x, P, h0=None, flags=0):
    h0 = torch.zeros(x.shape[1], P["u"].shape[0] if P["u"].numel() else P["u2"].shape[0], device=DEV) if h0 is None else h0
    return S.forward_unroll(x, h0, P, "sigmoid", flags=flags)


def _bwd(G, x, hs, zs, cs, P, h0, flags=0):
    return S.backward_unroll(G, x, hs, zs, cs, h0, P, "sigmoid", flags=flags)


def test_full_size_batch_independence_and_generic_agreement():
    """B=4096 (config 2): every utterance's hidden states are independent of its batch
    neighbours (bitwise vs a re-run on a ragged slice), the dispatched path agrees with
    the generic path, and a sampled slice agrees with the fp64 oracle."""
    B = 4096
    x, G, p, P = _northstar(B)
    hs, zs, cs = _fwd(x, P)
    # 48 utterances at a tile-misaligned offset: same (full-tile) kernel build, different
    # tile neighbours -> bitwise equal.  45 utterances run the ragged-tile build, whose
    # epilogue may contract fma differently -> equal to rounding.
    lo, hi = 1003, 1003 + 48
    hs_s, _, _ = _fwd(x[:, lo:hi].contiguous(), P)
    assert torch.equal(hs[:, lo:hi], hs_s)
    hs_r, _, _ = _fwd(x[:, lo:hi - 3].contiguous(), P)
    assert (hs[:, lo:hi - 3] - hs_r).abs().max() <= 2e-6
    hs_g, zs_g, cs_g = _fwd(x, P, flags=S.FLAG_FORCE_GENERIC)
    assert (hs - hs_g).abs().max() <= 1e-5
    hs_o, _, _ = S.oracle64_forward(x[:, lo:hi].cpu().numpy(), p, None)
    assert np.abs(hs[:, lo:hi].cpu().numpy() - hs_o).max() <= 1e-5


def test_full_size_backward_linearity_and_shard_sum():
    """B=4096 (metric shape): backward is linear in grad_hs, and parameter gradients of
    the whole batch equal the sum over two batch shards (the data-parallel identity of
    SURVEY section 8e); d_x of a shard equals the shard of d_x."""
    B = 4096
    x, G, p, P = _northstar(B, seed=1)
    h0 = torch.zeros(B, 128, device=DEV)
    hs, zs, cs = _fwd(x, P, h0)
    g1 = _bwd(G, x, hs, zs, cs, P, h0)
    g2 = _bwd(2.0 * G, x, hs, zs, cs, P, h0)
    for a, b in zip(g1, g2):
        if a.numel():
            assert (2.0 * a - b).abs().max() <= 2e-6 * max(1.0, float(b.abs().max()))   # scaling by 2 is exact in every plane
    half = B // 2
    parts = []
    for sl in (slice(0, half), slice(half, B)):
        xs = x[:, sl].contiguous(); Gs = G[:, sl].contiguous(); hz = h0[sl].contiguous()
        hs_s, zs_s, cs_s = _fwd(xs, P, hz)
        parts.append(_bwd(Gs, xs, hs_s, zs_s, cs_s, P, hz))
    for i in (1, 2, 3, 4, 6, 7):   # d_bias_z, d_bias_h, d_zeta, d_nu, d_w, d_u
        s = parts[0][i] + parts[1][i]
        # each side is within 2e-5 of the fp64 oracle (tests/test_hip_fullsize.py): two valid fp32 summation
        # orders may differ by twice that
        assert (s - g1[i]).abs().max() <= 4e-5 * max(1.0, float(g1[i].abs().max())), i
    assert torch.allclose(torch.cat([parts[0][0], parts[1][0]], 1), g1[0], atol=1e-6, rtol=0)
    # the generic path AND the dispatched one against the fp64 oracle on the whole batch
    gg = _bwd(G, x, hs, zs, cs, P, h0, flags=S.FLAG_FORCE_GENERIC)
    g_o = S.oracle64(x.cpu().numpy(), G.cpu().numpy(), p, None)[3]
    for tag, got in (("dispatch", g1), ("generic", gg)):
        S.check_grads(got, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=tag)


def test_lowrank_config4_shape_vs_oracle_sample():
    """config (4): H=256, wRank=uRank=16, B=4096; sampled utterances vs fp64 oracle."""
    T, B, F, H, r = 99, 4096, 32, 256, 16
    p = O.make_params(F, H, r, r, seed=9)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, F, generator=g).to(DEV)
    hs, zs, cs = _fwd(x, P)
    idx = [0, 17, 2048, 4095]
    hs_o, _, _ = S.oracle64_forward(x[:, idx].cpu().numpy(), p, None)
    assert np.abs(hs[:, idx].cpu().numpy() - hs_o).max() <= 1e-5


def test_run_to_run_bitwise_repeatability():
    """The scans are deterministic by construction (fixed-order reductions, no atomics): repeated runs
    on the same inputs must agree bit for bit.  A difference means an on-chip race -- e.g. a load
    landing in a register that an in-flight MFMA still reads (seen while prototyping a two-role
    backward)."""
    T = 99
    # (H, rank, B, flags, F): 8-wave kernels under both saved-tensor contracts, the low-rank pair, the 4-wave
    # forward, the fp32-MFMA path, the headline batch, and the stack's layers (wide input; H = 256)
    SP, W4, F32 = S.FLAG_SAVE_PREACT, S.FLAG_FWD_4WAVE, S.FLAG_FORCE_F32_MFMA
    for (H, r, B, flags, F) in ((128, 0, 1024, SP, 32), (256, 16, 512, SP, 32), (128, 0, 1008, 0, 32), (128, 0, 1024, SP | W4, 32),
                                (128, 0, 512, F32, 32), (256, 16, 512, 0, 32), (128, 0, 4096, SP, 32), (128, 0, 1024, SP, 256),
                                (256, 0, 1024, SP, 32), (256, 0, 1000, 0, 32)):
        p = O.make_params(F, H, r or None, r or None, seed=21)
        P = S.cell_tensors(p)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(T, B, F, generator=g).to(DEV)
        G = torch.randn(T, B, H, generator=g).to(DEV)
        h0 = torch.zeros(B, H, device=DEV)
        first = None
        for rep in range(12):
            outs, gr = S.fwd_bwd(x, h0, G, P, "sigmoid", flags=flags, biases=True)
            allo = [o for o in list(outs) + list(gr) if o.numel()]
            if first is None:
                first = [o.clone() for o in allo]
            else:
                for k, (a, b) in enumerate(zip(allo, first)):
                    assert torch.equal(a, b), (H, F, r, B, flags, rep, k)


@pytest.mark.parametrize("B,preact", [(37, True), (64, True), (48, False), (1, True)])
def test_batch_major_layout_equals_time_major(B, preact):
    """FLAG_BATCH_MAJOR (N1: the trainer's batch_first layout indexed in place, rnn.py:812-813,823-825):
    same arithmetic per utterance, so every output equals the time-major run bit for bit."""
    T, F, H = 23, 32, 128
    BATCH_MAJOR, SAVE_PREACT = S.FLAG_BATCH_MAJOR, S.FLAG_SAVE_PREACT
    p = O.make_params(F, H, seed=4, randomize_scalars=True)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(T, B, F, generator=g).to(DEV)
    G = torch.randn(T, B, H, generator=g).to(DEV)
    h0 = (0.3 * torch.randn(B, H, generator=g)).to(DEV)
    base = SAVE_PREACT if preact else 0

    def run(xi, Gi, flags):
        outs, gr = S.fwd_bwd(xi, h0, Gi, P, "sigmoid", flags=flags, biases=preact)
        return list(outs), list(gr)

    o_t, g_t = run(x, G, base)
    o_b, g_b = run(x.transpose(0, 1).contiguous(), G.transpose(0, 1).contiguous(), base | BATCH_MAJOR)
    for a, b in zip(o_t, o_b):
        assert b.shape == (B, T, H) and torch.equal(a, b.transpose(0, 1))
    assert g_b[0].shape == (B, T, F) and torch.equal(g_t[0], g_b[0].transpose(0, 1))
    for a, b in zip(g_t[1:8], g_b[1:8]):
        assert torch.equal(a, b)
    # not available off the split-precision path: the caller transposes instead
    assert fastgrnn_cuda.kernel_path(T, B, 20, 100, 0, 0, 0, direction=0, flags=base | BATCH_MAJOR) != 2
    with pytest.raises(RuntimeError):
        S.forward_unroll(x.transpose(0, 1).contiguous(), h0, P, "sigmoid", flags=BATCH_MAJOR | S.FLAG_FORCE_GENERIC)


@pytest.mark.parametrize("F,H", [(32, 128), (32, 256), (64, 256), (256, 128), (64, 128)],
                         ids=["F32H128", "F32H256", "F64H256", "F256H128", "F64H128"])
@pytest.mark.parametrize("B,batch_major", [(64, False), (37, False), (48, True)])
def test_bf16_sequences_fp32_master_grads(B, batch_major, F, H):
    """BASELINE config "fwd+bwd training step, bf16 with fp32 master grads" (parity unpinned by the
    reference, which has no such type): x, hs, grad_hs, d_x are bf16 in HBM; state, parameters, the
    saved pre-activation and every parameter gradient are fp32.  Checked against the fp64 oracle run
    on the SAME rounded tensors: hs and d_x to bf16 rounding (2^-8 relative), the fp32 outputs to the
    fp32 tolerances of the other tests."""
    LC.bf16_master_grads_case(31, B, batch_major, F, H)   # (H = 256: the first layer of the default stack, round 3)


@pytest.mark.parametrize("F,H,batch_first", [(32, 128, False), (32, 256, False), (64, 256, False), (32, 256, True),
                                             (256, 128, False), (256, 128, True)])
def test_module_bf16_sequences_autograd(F, H, batch_first):
    """FastGRNNCUDA fed bf16 frames: bf16 hidden states out, bf16 d_input and fp32 parameter gradients
    back; agrees with the same module run in fp32 on the rounded frames to bf16 rounding.  (H = 256, round 3: the
    dense H = 256 scans and their GEMMs take bf16 sequences; batch_first there runs on transposed copies.)"""
    T, B = 25, 40
    torch.manual_seed(5)
    m = FastGRNNCUDA(F, H, batch_first=batch_first, device=DEV)
    x = torch.randn(T, B, F).to(torch.bfloat16)
    G = torch.randn(T, B, H).to(torch.bfloat16)
    if batch_first:
        x, G = x.transpose(0, 1).contiguous(), G.transpose(0, 1).contiguous()
    else:
        assert fastgrnn_cuda.kernel_path(T, B, F, H, dtype=torch.bfloat16, direction=1, flags=S.FLAG_SAVE_PREACT) == 2
    xb = x.to(DEV).requires_grad_(True)
    hb = m(xb)
    assert hb.dtype == torch.bfloat16
    hb.backward(G.to(DEV))
    gb = {n: p_.grad.clone() for n, p_ in m.named_parameters()}
    dxb = xb.grad.clone()
    assert dxb.dtype == torch.bfloat16 and all(v.dtype == torch.float32 for v in gb.values())
    for p_ in m.parameters():
        p_.grad = None
    xf = x.float().to(DEV).requires_grad_(True)
    hf = m(xf)
    hf.backward(G.float().to(DEV))
    assert ((hb.float() - hf).abs() / hf.abs().clamp(min=1.0)).max() <= 2.0 ** -8 + 1e-5
    assert ((dxb.float() - xf.grad).abs() / xf.grad.abs().clamp(min=1.0)).max() <= 2.0 ** -7
    for n, p_ in m.named_parameters():
        scale = max(1.0, float(p_.grad.abs().max()))
        # h_prev enters dU / d_zeta through its bf16-rounded copy: relative 2^-9 per term, random sign
        assert (gb[n] - p_.grad).abs().max() / scale <= 1e-2, n


def test_grad_bucket_on_rccl_single_rank():
    """The data-parallel exchange on the real backend (RCCL), one rank: the bucket's pack -> all-reduce ->
    unpack leaves the gradients unchanged, on the compute stream, and ReduceOp.AVG -- which the N>1 path
    uses to take the mean inside the collective -- is accepted by this RCCL build (else the bucket's
    SUM + scale fallback is what will run)."""
    import os
    import torch.distributed as dist
    from kws_amd.dp import GradBucket
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29581")
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        torch.manual_seed(2)
        m = FastGRNNCUDA(32, 128, device=DEV)
        x = torch.randn(9, 32, 32, device=DEV)
        m(x).sum().backward()
        before = [p_.grad.clone() for p_ in m.parameters()]
        bucket = GradBucket(list(m.parameters()))
        assert bucket.total == 128 * 32 + 128 * 128 + 2 * 128 + 2          # 20 738 floats
        # the operator's gradient outputs are views of one flat buffer and autograd adopts them as .grad:
        # the bucket all-reduces that buffer in place (no pack / unpack kernels)
        assert bucket.shared_flat_() is not None
        bucket.all_reduce_()
        torch.cuda.synchronize()
        for a, p_ in zip(before, m.parameters()):
            assert torch.equal(a, p_.grad)
        t = torch.ones(4, device=DEV)
        try:
            dist.all_reduce(t, op=dist.ReduceOp.AVG)
            torch.cuda.synchronize()
            assert torch.equal(t, torch.ones(4, device=DEV))
        except RuntimeError:
            pass                                  # GradBucket falls back to SUM + scale
    finally:
        if own_group:
            dist.destroy_process_group()


@pytest.mark.parametrize("gate", ["quantTanh", "quantSigm", "quantSigm4"])
def test_quantised_gates_on_the_matrix_pipe(gate):
    """the CPU cell's quantised gate nonlinearities (rnn.py:53-60) on the 8-wave split-precision
    kernels (one-saved-tensor contract).  Piecewise-linear gates have derivative jumps, so -- as for relu --
    the backward is compared with the oracle evaluated on the kernel's own gate values (same mask)."""
    T, B, F, H = 12, 37, 32, 128
    SAVE_PREACT = S.FLAG_SAVE_PREACT
    code = S.NONLINEARITY[gate]
    rng = np.random.default_rng(code)
    p = O.make_params(F, H, dtype=np.float32, seed=31, randomize_scalars=True)
    p["bias_gate"] = (0.3 * p["bias_gate"]).astype(np.float32)   # pre-activations on both sides of the clamps
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    P = S.cell_tensors(p)
    xt, ht, Gt = S.to_dev(x), S.to_dev(h0), S.to_dev(G)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, direction=0, flags=SAVE_PREACT) == 2
    assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, direction=1, flags=SAVE_PREACT) == 2
    assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, direction=1) != 2     # reference contract: generic scan
    (hs, pre), outs = S.fwd_bwd(xt, ht, Gt, P, gate, flags=SAVE_PREACT, biases=True)
    hs_o, zs_o, cs_o = S.oracle64_forward(x, p, h0, gate)
    assert (np.abs(hs.cpu().numpy() - hs_o) / np.maximum(1.0, np.abs(hs_o))).max() <= 1e-5
    # a fair share of the gate values is strictly inside (0,1) / (-1,1): the test exercises both branches
    inside = (zs_o > (-1 if gate == "quantTanh" else 0)) & (zs_o < 1)
    assert 0.2 < inside.mean() < 0.999, inside.mean()
    pre_k = pre.cpu().numpy()
    a = pre_k + p["bias_gate"]
    zk = {"quantTanh": np.clip(a, -1, 1), "quantSigm": np.clip((a + 1) / 2, 0, 1),
          "quantSigm4": np.clip((a + 2) / 4, 0, 1)}[gate].astype(np.float32)
    ck = np.tanh(pre_k + p["bias_update"]).astype(np.float32)
    g_o = O.unroll_backward(G, x, hs.cpu().numpy(), zk, ck, p, h0, gate=gate)
    S.check_grads(outs, g_o, tol=5e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=gate)


@pytest.mark.parametrize("gate,B", [("sigmoid", 64), ("quantSigm", 37), ("sigmoid", 4096)])
def test_quant_tanh_update_on_the_matrix_pipe(gate, B):
    """The CPU cell's quantTanh UPDATE nonlinearity (rnn.py:57-58,292-293; golden g7 pins the oracle for it) on the
    8-wave split-precision kernels: c = clip(pre + b_h, -1, 1), dc/da = 1 inside (-1,1), 0 outside.  Forward against
    the fp64 oracle; backward against the oracle on the kernel's own z, c (the clamp's derivative jumps)."""
    T, F, H = (12, 32, 128) if B < 4096 else (99, 32, 128)
    SAVE_PREACT, QT = S.FLAG_SAVE_PREACT, S.NONLINEARITY["quantTanh"]
    code = S.NONLINEARITY[gate]
    rng = np.random.default_rng(B)
    p = O.make_params(F, H, dtype=np.float32, seed=17, randomize_scalars=True)
    p["w"] = (3.0 * p["w"]).astype(np.float32)                  # update pre-activations on both sides of the clamp
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    P = S.cell_tensors(p)
    xt, ht, Gt = S.to_dev(x), S.to_dev(h0), S.to_dev(G)
    for direction, flags in ((0, 0), (0, SAVE_PREACT), (1, SAVE_PREACT)):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, update_nl=QT, direction=direction, flags=flags) == 2
    assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, update_nl=QT, direction=1) != 2   # reference contract
    hs, pre = S.forward_unroll(xt, ht, P, gate, update="quantTanh", flags=SAVE_PREACT)
    hs_only = S.forward_unroll(xt, ht, P, gate, update="quantTanh", want_gates=False)[0]
    assert torch.equal(hs, hs_only)
    outs = S.backward_of((hs, pre), Gt, xt, ht, P, gate, update="quantTanh", flags=SAVE_PREACT, biases=True)
    hs_o, zs_o, cs_o = S.oracle64_forward(x, p, h0, gate, "quantTanh")
    assert (np.abs(hs.cpu().numpy() - hs_o) / np.maximum(1.0, np.abs(hs_o))).max() <= 1e-5
    inside = (cs_o > -1) & (cs_o < 1)
    assert 0.2 < inside.mean() < 0.98, inside.mean()
    pre_k = pre.cpu().numpy()
    a = pre_k + p["bias_gate"]
    zk = (1.0 / (1.0 + np.exp(-a.astype(np.float64))) if gate == "sigmoid" else np.clip((a + 1) / 2, 0, 1)).astype(np.float32)
    ck = np.clip(pre_k + p["bias_update"], -1, 1).astype(np.float32)
    g_o = O.unroll_backward(G, x, hs.cpu().numpy(), zk, ck, p, h0, gate=gate, update="quantTanh")
    S.check_grads(outs, g_o, tol=5e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag=gate + "/quantTanh")


@pytest.mark.parametrize("B,hs_batch_major,H", [(37, False, 128), (64, False, 128), (48, True, 128),
                                                 (37, False, 256), (64, False, 256)])
def test_trainer_bft_input_layout_in_place(B, hs_batch_major, H):
    """FLAG_X_BFT: x / d_x in the data loader's [B,F,T] (trainClassifier.py:204 permutes it into
    a [T,B,F] view and the reference then copies it).  Same arithmetic: every output equals the time-major
    run bit for bit.  H=128 (in place) and the reference's first layer H=256 (trainingConfig.py:12-15), which
    transposes the frames into its workspace in both calls."""
    T, F = 23, 32
    SAVE_PREACT, BATCH_MAJOR, X_BFT = S.FLAG_SAVE_PREACT, S.FLAG_BATCH_MAJOR, S.FLAG_X_BFT
    p = O.make_params(F, H, seed=6, randomize_scalars=True)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(T, B, F, generator=g).to(DEV)
    G = torch.randn(T, B, H, generator=g).to(DEV)
    h0 = (0.3 * torch.randn(B, H, generator=g)).to(DEV)

    def run(xi, Gi, flags):
        outs, gr = S.fwd_bwd(xi, h0, Gi, P, "sigmoid", flags=flags, biases=True)
        return list(outs), list(gr)

    o_t, g_t = run(x, G, SAVE_PREACT)
    x_bft = x.permute(1, 2, 0).contiguous()                       # [B,F,T]
    lay = (lambda t: t.transpose(0, 1).contiguous()) if hs_batch_major else (lambda t: t)
    unlay = (lambda t: t.transpose(0, 1)) if hs_batch_major else (lambda t: t)
    fl = SAVE_PREACT | X_BFT | (BATCH_MAJOR if hs_batch_major else 0)
    o_b, g_b = run(x_bft, lay(G), fl)
    for a, b in zip(o_t, o_b):
        assert torch.equal(a, unlay(b))
    assert g_b[0].shape == (B, F, T) and torch.equal(g_t[0], g_b[0].permute(2, 0, 1))
    for a, b in zip(g_t[1:8], g_b[1:8]):
        assert torch.equal(a, b)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=fl) == 2
    if H == 128:                                                   # not offered off the 8-wave dense kernels
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=X_BFT) != 2


@pytest.mark.parametrize("H", [128, 256])
def test_module_takes_the_trainers_permuted_view(H):
    """FastGRNNCUDA fed `audio.permute(2, 0, 1)` exactly as trainClassifier.py:204 does: same results and the
    same gradient on the loader's [B,F,T] tensor as with a contiguous copy, without making one."""
    T, B, F = 29, 40, 32
    torch.manual_seed(8)
    m = FastGRNNCUDA(F, H, device=DEV)
    audio = torch.randn(B, F, T, device=DEV)
    G = torch.randn(T, B, H, device=DEV)
    a1 = audio.clone().requires_grad_(True)
    hs1 = m(a1.permute(2, 0, 1))                                  # the trainer's view
    hs1.backward(G)
    g1 = {n: p_.grad.clone() for n, p_ in m.named_parameters()}
    for p_ in m.parameters():
        p_.grad = None
    a2 = audio.clone().requires_grad_(True)
    hs2 = m(a2.permute(2, 0, 1).contiguous())                     # what the reference's .contiguous() makes
    hs2.backward(G)
    assert torch.equal(hs1, hs2) and torch.equal(a1.grad, a2.grad)
    for n, p_ in m.named_parameters():
        assert torch.equal(g1[n], p_.grad), n


@pytest.mark.parametrize("B", [48, 37])
def test_ab_kernel_variants_agree_with_the_default(B):
    """The A/B flags select an older kernel shape / operand format of the same arithmetic: 4-wave forward (8),
    three-bf16-plane forward state product (64).  They must agree with the default kernels to fp32 rounding
    (they differ in summation order and, for 64, in the operand split)."""
    T, F, H = 40, 32, 128
    SAVE_PREACT, FWD_4WAVE, FWD_BF16X3 = S.FLAG_SAVE_PREACT, S.FLAG_FWD_4WAVE, S.FLAG_FWD_BF16X3
    p = O.make_params(F, H, seed=12, randomize_scalars=True)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(T, B, F, generator=g).to(DEV)
    G = torch.randn(T, B, H, generator=g).to(DEV)
    h0 = (0.3 * torch.randn(B, H, generator=g)).to(DEV)

    def run(flags):
        outs, gr = S.fwd_bwd(x, h0, G, P, "sigmoid", flags=flags, biases=True)
        return list(outs) + list(gr[:8])

    ref = run(SAVE_PREACT)
    for extra in (FWD_4WAVE, FWD_BF16X3, FWD_4WAVE | FWD_BF16X3):
        got = run(SAVE_PREACT | extra)
        for k, (a, b) in enumerate(zip(ref, got)):
            scale = max(1.0, float(a.abs().max()))
            tol = 4e-5 if k in (5, 6) else 2e-5           # d_zeta, d_nu: two valid summation orders, each within 2e-5
            assert float((a - b).abs().max()) / scale <= tol, (extra, k)


# ---- the classifier's view of the last layer (model.py:227 reads hs[T-1] alone) ---------------
GRAD_LAST, HS_LAST = S.FLAG_GRAD_LAST, S.FLAG_HS_LAST


@pytest.mark.parametrize("B,preact,bf16,batch_major", [(64, True, False, False), (37, True, False, False),
                                                       (48, False, False, False), (37, True, True, False),
                                                       (64, True, False, True)])
def test_grad_last_equals_the_dense_zero_padded_gradient(B, preact, bf16, batch_major):
    """FLAG_GRAD_LAST: grad_hs is the [B,H] gradient of the last state.  Adding the zero gradient of every
    other step is exact, so all twelve outputs equal the dense run's bit for bit."""
    T, F, H = 21, 32, 128
    p = O.make_params(F, H, seed=31, randomize_scalars=True)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(32)
    dt = torch.bfloat16 if bf16 else torch.float32
    lead = (B, T) if batch_major else (T, B)
    x = torch.randn(*lead, F, generator=g).to(DEV).to(dt)
    gl = torch.randn(B, H, generator=g).to(DEV).to(dt)
    h0 = (0.3 * torch.randn(B, H, generator=g)).to(DEV)
    flags = (S.FLAG_SAVE_PREACT if preact else 0) | (S.FLAG_BATCH_MAJOR if batch_major else 0)
    outs = S.forward_unroll(x, h0, P, "sigmoid", flags=flags)
    dense = torch.zeros(*lead, H, device=DEV, dtype=dt)
    (dense[:, -1] if batch_major else dense[-1]).copy_(gl)
    ref = S.backward_of(outs, dense, x, h0, P, "sigmoid", flags=flags, biases=preact)
    got = S.backward_of(outs, gl, x, h0, P, "sigmoid", flags=flags | GRAD_LAST, biases=preact)
    for k, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape and torch.equal(a, b), k
    # and against the oracle (fp32, time-major case only)
    if not bf16 and not batch_major:
        hs_o, zs_o, cs_o = O.unroll_forward(x.cpu().numpy(), p, h0.cpu().numpy())
        G = np.zeros((T, B, H), np.float32); G[-1] = gl.cpu().numpy()
        ref_o = O.unroll_backward(G, x.cpu().numpy(), hs_o, zs_o, cs_o, p, h0.cpu().numpy())
        S.check_grads(got, ref_o, tol=1e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag="grad_last")


@pytest.mark.parametrize("B,bf16,batch_major", [(64, False, False), (37, False, False), (48, True, False), (37, False, True)])
def test_hs_last_forward_writes_only_the_final_state(B, bf16, batch_major):
    """FLAG_HS_LAST (inference): hs is [B,H] = h_T, equal to the last row of the full forward to fp32 rounding; with
    saved tensors requested the combination is refused."""
    T, F, H = 17, 32, 128
    p = O.make_params(F, H, seed=33, randomize_scalars=True)
    P = S.cell_tensors(p)
    g = torch.Generator().manual_seed(34)
    dt = torch.bfloat16 if bf16 else torch.float32
    lead = (B, T) if batch_major else (T, B)
    x = torch.randn(*lead, F, generator=g).to(DEV).to(dt)
    h0 = (0.3 * torch.randn(B, H, generator=g)).to(DEV)
    flags = S.FLAG_BATCH_MAJOR if batch_major else 0
    fwd = lambda **kw: S.forward_unroll(x, h0, P, "sigmoid", **kw)
    full = fwd(want_gates=False, flags=flags)[0]
    last = fwd(want_gates=False, flags=flags | HS_LAST)[0]
    assert last.shape == (B, H)
    # a separately compiled variant of the same arithmetic (fma contraction may differ): fp32 rounding, not bits
    want = (full[:, -1] if batch_major else full[-1]).float()
    assert float((last.float() - want).abs().max()) <= (2.0 ** -7 if bf16 else 2e-6) * max(1.0, float(want.abs().max()))
    with pytest.raises(RuntimeError):
        fwd(want_gates=True, flags=flags | HS_LAST)
    with pytest.raises(RuntimeError):                 # generic path: unsupported, loudly
        fwd(want_gates=False, flags=flags | HS_LAST | S.FLAG_FORCE_GENERIC)


@pytest.mark.parametrize("kind", ["dense", "dense_batch_first", "lowrank", "dense_bf16"])
def test_module_last_state_matches_indexing_the_sequence(kind):
    """FastGRNNCUDA(..., last_state=True) == FastGRNNCUDA(...)[-1] with the same parameter and input gradients
    (dense H=128/F=32: FLAG_GRAD_LAST; other shapes: the dense form on the same kernels); under no_grad the
    sequence is not written (FLAG_HS_LAST)."""
    from kws_amd.rnn import FastGRNNCUDA
    T, B, F = 19, 40, 32
    H, r = (256, 16) if kind == "lowrank" else (128, None)
    bf = kind == "dense_batch_first"
    torch.manual_seed(5)
    m = FastGRNNCUDA(F, H, wRank=r, uRank=r, batch_first=bf, device=DEV)
    x = torch.randn((B, T, F) if bf else (T, B, F), device=DEV)
    if kind == "dense_bf16":
        x = x.to(torch.bfloat16)
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    gl = torch.randn(B, H, device=DEV).to(x.dtype)
    full = m(x1)
    (full[:, -1] if bf else full[-1]).backward(gl)
    g1 = {n: p_.grad.clone() for n, p_ in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    last = m(x2, last_state=True)
    assert last.shape == (B, H) and torch.equal(last, (full[:, -1] if bf else full[-1]).detach())
    last.backward(gl)
    for n, p_ in m.named_parameters():
        assert torch.equal(g1[n], p_.grad), n
    assert torch.equal(x1.grad, x2.grad)
    with torch.no_grad():
        inf = m(x, last_state=True)                 # FLAG_HS_LAST where available: its own kernel variant
        tol = (2.0 ** -7 if x.dtype == torch.bfloat16 else 2e-6) * max(1.0, float(last.detach().float().abs().max()))
        assert inf.shape == last.shape and float((inf.float() - last.detach().float()).abs().max()) <= tol


@pytest.mark.parametrize("B,H,Cn", [(64, 128, 12), (37, 128, 12), (4096, 128, 12), (50, 256, 35), (1, 64, 2), (130, 20, 64),
                                    (33, 256, 64)])      # the last one needs 86 KB of dynamic LDS (opt-in attribute)
def test_classifier_head_loss_and_gradients_vs_torch_cpu(B, H, Cn):
    """fastgrnn_hip_head_xent == NLLLoss()(log_softmax(Linear(h)), y) and its autograd gradients, computed by
    torch on the CPU in float64 (model.py:226-230, trainClassifier.py:154,236) and by the numpy oracle
    (oracle.head_loss_and_grads).  fp32 tolerance 1e-5 relative to the largest element of each tensor."""
    from kws_amd import head
    g = torch.Generator().manual_seed(41)
    h = torch.randn(B, H, generator=g)
    w = 0.3 * torch.randn(Cn, H, generator=g)
    b = 0.1 * torch.randn(Cn, generator=g)
    y = torch.randint(0, Cn, (B,), generator=g)
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    logp_ref = torch.log_softmax(h64 @ w64.t() + b64, dim=1)
    loss_ref = torch.nn.NLLLoss()(logp_ref, y)
    loss_ref.backward()
    loss, logp, d_h, d_w, d_b = head.head_xent(h.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV), want_log_probs=True)

    def close(a, ref, what):
        ref = ref.detach().float()
        scale = max(1e-30, float(ref.abs().max()))
        assert float((a.cpu() - ref).abs().max()) / scale <= 1e-5, what

    close(loss, loss_ref.reshape(1), "loss")
    close(logp, logp_ref, "log_probs")
    close(d_h, h64.grad, "d_h")
    close(d_w, w64.grad, "d_w")
    close(d_b, b64.grad, "d_b")
    o = O.head_loss_and_grads(h.double().numpy(), w.double().numpy(), b.double().numpy(), y.numpy())
    for a, ref, what in zip((loss, logp, d_h, d_w, d_b), o, ("loss", "log_probs", "d_h", "d_w", "d_b")):
        close(a, torch.from_numpy(np.atleast_1d(np.asarray(ref))), "oracle " + what)
    # twice the same bits (fixed-order reduction)
    again = head.head_xent(h.to(DEV), w.to(DEV), b.to(DEV), y.to(DEV), want_log_probs=True)
    for a, c in zip((loss, logp, d_h, d_w, d_b), again):
        assert torch.equal(a, c)


def test_model_tail_last_state_plus_head_matches_the_reference_chain():
    """The tail of RNNClassifierModel.forward + the training loss (model.py:226-230, trainClassifier.py:236) two
    ways on the GPU: hs = rnn(x); NLLLoss(log_softmax(Linear(hs[-1]))) with torch modules, against
    rnn(x, last_state=True) -> KeywordHead.loss.  Same loss and same gradients for every parameter and the input."""
    from kws_amd.rnn import FastGRNNCUDA
    from kws_amd.head import KeywordHead
    T, B, F, H, Cn = 25, 96, 32, 128, 12
    torch.manual_seed(6)
    rnn = FastGRNNCUDA(F, H, device=DEV)
    head = KeywordHead(H, Cn, device=DEV)
    x = torch.randn(T, B, F, device=DEV)
    y = torch.randint(0, Cn, (B,), device=DEV)
    x1 = x.clone().requires_grad_(True)
    loss_ref = torch.nn.NLLLoss()(head(rnn(x1)[-1]), y)
    loss_ref.backward()
    params = list(rnn.named_parameters()) + list(head.named_parameters())
    g_ref = {n: p_.grad.clone() for n, p_ in params}
    for _, p_ in params:
        p_.grad = None
    x2 = x.clone().requires_grad_(True)
    loss = head.loss(rnn(x2, last_state=True), y)
    loss.backward()
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * max(1.0, abs(float(loss_ref)))
    for n, p_ in params:
        scale = max(1e-12, float(g_ref[n].abs().max()))
        assert float((p_.grad - g_ref[n]).abs().max()) / scale <= 2e-5, n
    assert float((x2.grad - x1.grad).abs().max()) / max(1e-12, float(x1.grad.abs().max())) <= 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("F,H,r", [(32, 128, None), (32, 256, None), (64, 256, None), (256, 128, None), (32, 256, 16), (32, 256, 32)])
@pytest.mark.parametrize("batch_first", [False, True])
def test_module_forward_without_grad_saves_nothing_and_matches_the_training_forward(batch_first, F, H, r):
    """Under torch.no_grad() the module runs the hs-only forward (no pre-activation written); same bits as the
    training forward, also after a call under inference_mode (the cached default state must not be an inference tensor).
    Every kernel family: dense H=128 (fused and wide input), dense H=256 (F=32 and the frame-GEMM form), low-rank,
    multiplied-out factors."""
    torch.manual_seed(3)
    T, B = 17, 40
    m = FastGRNNCUDA(F, H, wRank=r, uRank=r, batch_first=batch_first, device=DEV)
    x = torch.randn((B, T, F) if batch_first else (T, B, F), device=DEV)
    with torch.inference_mode():
        hs_i = m(x).clone()
    with torch.no_grad():
        hs_n = m(x)
    xg = x.clone().requires_grad_(True)
    hs_t = m(xg)
    assert hs_t.requires_grad and not hs_n.requires_grad
    assert torch.equal(hs_i, hs_n)
    if r == 16:
        # the register-resident low-rank forward's hs-only and pre-activation-saving instantiations are compiled
        # separately and do not round their gate arithmetic identically (multiply-add contraction around the value
        # that one of them stores and the other does not): the same value to fp32 rounding, not the same bits
        assert float((hs_n - hs_t.detach()).abs().max()) <= 2e-6 * max(1.0, float(hs_t.detach().abs().max()))
    else:
        assert torch.equal(hs_n, hs_t.detach())
    hs_t.square().sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
