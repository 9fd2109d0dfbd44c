"""Case bodies and input draws that more than one GPU test file runs: the bf16-sequence layer against the fp64 oracle
(test_hip_parity.py at the suite's sizes, test_hip_partition_seams.py where the weight-gradient GEMMs cut long chunks)
and the [B,F,T]-against-time-major comparison (test_hip_bft_wide.py, test_hip_partition_seams.py).  Each states its
own bounds; the helpers are those of tests/support.py."""
import functools

import numpy as np
import pytest
import torch

from kws_amd import fastgrnn_cuda
from oracle import fastgrnn_oracle as O
from tests import support as S
from tests.support import DEV


@functools.lru_cache(maxsize=None)
def plain_cell(H, F, gate):
    """A dense cell as tests/test_hip_parity.py draws them (relu: scaled so that the state stays in range), computed
    once and left unchanged: the numpy dict and its operand tensors."""
    p = O.make_params(F, H, dtype=np.float32, seed=11, randomize_scalars=True)
    if gate == "relu":
        for k in ("w", "u"):
            p[k] = (0.3 * p[k]).astype(np.float32)
        p["bias_gate"] = (0.3 * p["bias_gate"] - 0.1).astype(np.float32)
    return p, S.cell_tensors(p)


def layer_fwd_bwd(x, h0, G, p, gate=0, flags=0, preact=False):
    """forward_unroll + backward_unroll of the cell dict ``p`` on device tensors, under the one-saved-tensor contract
    (``preact``) or the reference's pair, the biases named to the backward under either; the forward's outputs and the
    twelve gradients"""
    return S.fwd_bwd(x, h0, G, S.cell_tensors(p), gate, flags=flags | (S.FLAG_SAVE_PREACT if preact else 0),
                     biases=True)


def bf16_master_grads_case(T, B, batch_major, F, H):
    """BASELINE config "fwd+bwd training step, bf16 with fp32 master grads" at any (T, B): x, hs, grad_hs, d_x are bf16
    in HBM; state, parameters, the saved pre-activation and every parameter gradient are fp32.  Against the fp64
    oracle run on the SAME rounded tensors: hs and d_x to bf16 rounding (2^-8 relative), the fp32 outputs to the fp32
    tolerances of the other tests."""
    SAVE_PREACT, BATCH_MAJOR = S.FLAG_SAVE_PREACT, S.FLAG_BATCH_MAJOR
    rng = np.random.default_rng(77 + B)
    p = O.make_params(F, H, dtype=np.float32, seed=23, randomize_scalars=True)
    P = S.cell_tensors(p)
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16)
    x_bf = bf(rng.standard_normal((T, B, F)).astype(np.float32))
    G_bf = bf(rng.standard_normal((T, B, H)).astype(np.float32))
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    flags = SAVE_PREACT | (BATCH_MAJOR if batch_major else 0)
    lay = (lambda t: t.transpose(0, 1).contiguous()) if batch_major else (lambda t: t)
    unlay = (lambda t: t.transpose(0, 1)) if batch_major else (lambda t: t)
    xt, Gt, ht = lay(x_bf).to(DEV), lay(G_bf).to(DEV), S.to_dev(h0)
    bwd_fast = not (H == 256 and batch_major)   # (the H = 256 backward takes bf16 sequences time-major only; the module transposes)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, dtype=torch.bfloat16, direction=0, flags=flags) == 2
    assert (fastgrnn_cuda.kernel_path(T, B, F, H, dtype=torch.bfloat16, direction=1, flags=flags) == 2) == bwd_fast
    hs, pre = S.forward_unroll(xt, ht, P, "sigmoid", flags=flags)
    assert hs.dtype == torch.bfloat16 and pre.dtype == torch.float32, (hs.dtype, pre.dtype)
    if bwd_fast:
        outs = S.backward_of((hs, pre), Gt, xt, ht, P, "sigmoid", flags=flags, biases=True)
        assert outs[0].dtype == torch.bfloat16 and outs[6].dtype == torch.float32, (outs[0].dtype, outs[6].dtype)
    # ---- forward against the oracle on the rounded x: fp32 state inside, bf16 only when stored
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    x64 = x_bf.to(torch.float64).numpy(); G64 = G_bf.to(torch.float64).numpy(); h64 = h0.astype(np.float64)
    hs_o, zs_o, cs_o = O.unroll_forward(x64, p64, h64)
    hs_k = unlay(hs).to(torch.float64).cpu().numpy()
    e_hs = (np.abs(hs_k - hs_o) / np.maximum(1.0, np.abs(hs_o))).max()
    assert e_hs <= 2.0 ** -8 + 1e-5, ("hs", e_hs)   # one bf16 rounding (RNE: 2^-9 relative)
    e_pre = np.abs(unlay(pre).cpu().numpy() - S.dense_preactivation64(x64, p, h0, hs_o)).max()
    assert e_pre <= 1e-5, ("pre-activation", e_pre)
    if not bwd_fast:
        return
    # ---- backward: the kernel sees the ROUNDED hs as h_prev (what autograd with bf16 activations does):
    #      oracle on the same tensors, gates from the exact pre-activation
    hs_r = hs_k.copy()
    pre_k = unlay(pre).cpu().numpy().astype(np.float64)
    z_k = 1.0 / (1.0 + np.exp(-(pre_k + p64["bias_gate"]))); c_k = np.tanh(pre_k + p64["bias_update"])
    g_o = O.unroll_backward(G64, x64, hs_r, z_k, c_k, p64, h64, diagnostics=True)
    g = dict(zip(S.GRAD_NAMES[:8], outs[:8]))
    dx = unlay(g.pop("d_x")).to(torch.float64).cpu().numpy()
    ref = g_o.pop("d_x")
    e_dx = (np.abs(dx - ref) / np.maximum(1.0, np.abs(ref))).max()
    assert e_dx <= 2.0 ** -8 + 2e-5, ("d_x", e_dx)
    S.check_grads(g, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag="bf16-io")
    # the reference's (z_s, h_prime_s) contract is not offered for bf16 sequences
    with pytest.raises(RuntimeError):
        S.forward_unroll(xt, ht, P, "sigmoid", flags=flags & ~SAVE_PREACT)


# ---- FASTGRNN_FLAG_X_BFT: the loader's [B,F,T] frames against the time-major copy ------------------------------------

def bft_params(F, H, seed, gate="sigmoid", w_rank=None, u_rank=None):
    p = O.make_params(F, H, w_rank, u_rank, np.float32, seed=seed, randomize_scalars=True)
    if gate == "relu":                          # an unbounded gate: keep z = relu(.) small so that h stays finite
        p["bias_gate"] = (p["bias_gate"] - 1.5).astype(np.float32)
        for k in ("u", "u1"):
            if k in p:
                p[k] = (0.1 * p[k]).astype(np.float32)
    return S.cell_tensors(p)


def bft_data(T, B, F, H, seed=5):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, B, F, generator=gen).to(DEV)                 # time-major
    xb = x.permute(1, 2, 0).contiguous()                            # the loader's [B,F,T]
    h0 = (0.5 * torch.randn(B, H, generator=gen)).to(DEV)
    G = torch.randn(T, B, H, generator=gen).to(DEV)
    return x, xb, h0, G


def named_backward(G, x, outs, h0, P, gate, flags, need_dx=True, update="tanh"):
    """the twelve gradients by name, of a backward on the forward's ``outs`` that names the biases and says whether it
    wants d_x"""
    return dict(zip(S.GRAD_NAMES, S.backward_of(outs, G, x, h0, P, gate, update=update, flags=flags, biases=True,
                                                need_dx=need_dx)))


def compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, gate, flags, tag, dx_optional=True):
    """all eight gradients, d_x given ([B,F,T], equal to the time-major d_x permuted) and d_x == NULL (the dense
    cells: the operator module always asks a factorised cell for d_x)"""
    ref = named_backward(G, x, o_tm, h0, P, gate, flags)
    for need_dx in ((True, False) if dx_optional else (True,)):
        got = named_backward(G, xb, o_bft, h0, P, gate, flags | S.FLAG_X_BFT, need_dx=need_dx)
        torch.cuda.synchronize()
        if need_dx:
            assert got["d_x"].shape == xb.shape, (tag, got["d_x"].shape, xb.shape)
            S.assert_same_bits(got["d_x"], ref["d_x"].permute(1, 2, 0), tag + " d_x")
        else:
            assert got["d_x"].numel() == 0, (tag, got["d_x"].shape)
        for k in S.GRAD_NAMES[1:]:
            if ref[k].numel():
                S.assert_same_bits(got[k], ref[k], "%s %s need_dx=%s" % (tag, k, need_dx))
    for k in ("d_w", "d_u", "d_w1", "d_u1", "d_h0", "d_zeta"):
        assert torch.isfinite(ref[k]).all(), (tag, k)
