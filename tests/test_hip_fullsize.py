"""BASELINE.json configurations at their FULL size (B = 4096, T = 99) against the fp64 numpy oracle -- every output
of forward and backward, not samples or HIP-vs-HIP identities.  The fp64 oracle takes a few seconds per case.

Why at full size: d_zeta / d_nu sum T*B*H = 5e7 (H = 128) or 1e8 (H = 256) terms; a one-signed rounding bias
of 1e-8 per term is invisible at B = 64 and a 3e-4 relative error here (that is how the truncating plane split and
the in-MFMA chopping were found).  Tolerances are north_star's: hidden states 1e-5 absolute,
gradients 2e-5 of max(1, max|ref|) -- the two scalars included.
"""
import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import _lib, fastgrnn_cuda
T, B, F = 99, 4096, 32


def _inputs(H, seed, rw=None, ru=None):
    rng = np.random.default_rng(seed)
    p = O.make_params(F, H, rw, ru, np.float32, seed=seed + 1, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    return p, x, G


@pytest.mark.parametrize("contract", ["preact", "reference"])
def test_config2_dense_f32_full_batch_every_output_vs_fp64_oracle(contract):
    """BASELINE configs 1/2 and the metric shape: dense H=128, fp32, B=4096, both saved-tensor contracts."""
    H = 128
    p, x, G = _inputs(H, 100)
    P = S.cell_tensors(p)
    xt, Gt = S.to_dev(x), S.to_dev(G)
    h0 = torch.zeros(B, H, device=DEV)
    flags = _lib.FLAG_SAVE_PREACT if contract == "preact" else 0
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=flags) == 2
    outs, gr = S.fwd_bwd(xt, h0, Gt, P, "sigmoid", flags=flags, biases=True)
    torch.cuda.synchronize()
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, None)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    if contract == "reference":
        assert np.abs(outs[1].cpu().numpy() - zs_o).max() <= 1e-5 and np.abs(outs[2].cpu().numpy() - cs_o).max() <= 1e-5
    errs = S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0, tag="config2/" + contract)
    print("config2/%s full-size errors: %s" % (contract, {k: "%.2e" % v for k, v in errs.items()}))


def test_config3_bf16_sequences_full_batch_every_output_vs_fp64_oracle():
    """BASELINE config 3: bf16 x / hs / grad_hs / d_x, fp32 state, parameters and master gradients, B=4096.
    The oracle runs in fp64 on the SAME rounded inputs; hs and d_x are compared to one bf16 rounding of the
    oracle's values (relative 2^-8 of the element), every fp32 output to 2e-5."""
    H = 128
    p, x, G = _inputs(H, 200)
    P = S.cell_tensors(p)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    Gb = torch.from_numpy(G).to(torch.bfloat16)
    xt, Gt = xb.to(DEV), Gb.to(DEV)
    h0 = torch.zeros(B, H, device=DEV)
    flags = _lib.FLAG_SAVE_PREACT
    assert fastgrnn_cuda.kernel_path(T, B, F, H, dtype=torch.bfloat16, direction=1, flags=flags) == 2
    (hs, pre), gr = S.fwd_bwd(xt, h0, Gt, P, "sigmoid", flags=flags, biases=True)
    torch.cuda.synchronize()
    xr, Gr = xb.float().numpy(), Gb.float().numpy()
    # forward: the kernel carries the state in fp32 and rounds only the stored copy
    hs_o, zs_o, cs_o = S.oracle64_forward(xr, p, None)
    hs_k = hs.float().cpu().numpy()
    assert (np.abs(hs_k - hs_o) <= 2.0 ** -8 * np.abs(hs_o) + 1e-5).all()
    # the saved pre-activation comes from the fp32 state trajectory: check it against the oracle's unrounded one
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    hprev_o = np.concatenate([np.zeros((1, B, H)), hs_o[:-1]], 0)
    pre_o = xr.astype(np.float64) @ p64["w"].T + hprev_o @ p64["u"].T
    pre_k = pre.cpu().numpy().astype(np.float64)
    assert np.abs(pre_k - pre_o).max() <= 1e-5
    # backward: the kernel reads the ROUNDED hidden states it stored (h_prev) and recomputes the gates from its
    # saved pre-activation; the oracle is given exactly those tensors
    hs_r = hs_k.astype(np.float64)
    z_r = O.nonlinearity(pre_k + p64["bias_gate"], "sigmoid")
    c_r = np.tanh(pre_k + p64["bias_update"])
    g_o = O.unroll_backward(Gr.astype(np.float64), xr.astype(np.float64), hs_r, z_r, c_r, p64)
    dx = gr[0].float().cpu().numpy()
    assert (np.abs(dx - g_o["d_x"]) <= 2.0 ** -8 * np.abs(g_o["d_x"]) + 2e-5 * max(1.0, np.abs(g_o["d_x"]).max())).all()
    del g_o["d_x"]                                   # (held to bf16 rounding above)
    errs = S.check_grads(dict(zip(S.GRAD_NAMES[1:], gr[1:])), g_o, tol=2e-5, scalar_term_tol=0.0, tag="config3")
    print("config3 full-size errors: %s" % {k: "%.2e" % v for k, v in errs.items()})


def test_config4_lowrank_full_batch_every_output_vs_fp64_oracle():
    """BASELINE config 4: H=256, wRank=uRank=16, B=4096, one-saved-tensor contract (scan + TN GEMMs)."""
    H, r = 256, 16
    p, x, G = _inputs(H, 300, r, r)
    P = S.cell_tensors(p)
    xt, Gt = S.to_dev(x), S.to_dev(G)
    h0 = torch.zeros(B, H, device=DEV)
    flags = _lib.FLAG_SAVE_PREACT
    assert fastgrnn_cuda.kernel_path(T, B, F, H, r, r, direction=1, flags=flags) == 2
    (hs, pre, m), gr = S.fwd_bwd(xt, h0, Gt, P, "sigmoid", flags=flags, biases=True)
    torch.cuda.synchronize()
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, None)
    assert np.abs(hs.cpu().numpy() - hs_o).max() <= 1e-5
    errs = S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0, tag="config4")
    print("config4 full-size errors: %s" % {k: "%.2e" % v for k, v in errs.items()})
