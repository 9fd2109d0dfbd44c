"""The F = 32 / H = 128 backward scan (bwd_scan_split_w8) at the sizes where its step order changes code path.

Which wave contracts a step pair's weight gradients is a compile-time fact of each unrolled copy of the scan's
iteration (the peeled odd iteration in front of the loop is the one without a pair), and the replacement of the
gradient by zeros -- last-state gradient, lanes beyond a ragged batch -- happens where the gradient is used, an
iteration behind its request ("Backward, 8 waves").  Both are per-instantiation code, so every contract
the operator module can reach is run here: one saved tensor and the reference's pair, bf16 sequences, the tanh gate
(one column tile per weight-gradient batch), the quantTanh update, the last state's gradient alone, [B,F,T] frames,
and the wide-input route at F = 64 (d_pre leaves the scan, no x planes).  Each with and without d_x.

T is the smallest value that reaches each piece of the loop: 1 (the last iteration only), 2 (the peeled odd
iteration in front of the loop, the one odd iteration without weight gradients), 3 (the virtual zero step pairs
with step 2), 4 and 5 (the first steady-state pair, behind a peeled iteration and without one), 9 (the ring of four
plane images is overwritten twice).  B = 1, 16, 17, 33: a ragged tile, a full one, and more than one workgroup.

Per case: the fp64 oracle at the bounds tests/test_hip_parity.py applies to the same outputs of the same contract;
two calls equal bit for bit; and every output the call without d_x shares with the full call equal bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import fastgrnn_cuda
SP, BFT, GL = S.FLAG_SAVE_PREACT, S.FLAG_X_BFT, S.FLAG_GRAD_LAST
NAMES = S.GRAD_NAMES[:8]

#            F   gate       update       preact bf16   grad_last  [B,F,T]
CONTRACTS = {
    "pre":  (32, "sigmoid", "tanh",      True,  False, False, False),
    "pair": (32, "sigmoid", "tanh",      False, False, False, False),
    "bf16": (32, "sigmoid", "tanh",      True,  True,  False, False),
    "tanh": (32, "tanh",    "tanh",      True,  False, False, False),
    "uq":   (32, "sigmoid", "quantTanh", True,  False, False, False),
    "gl":   (32, "sigmoid", "tanh",      True,  False, True,  False),
    "bft":  (32, "sigmoid", "tanh",      True,  False, False, True),
    "wide": (64, "sigmoid", "tanh",      True,  False, False, False),
}
TS = [1, 2, 3, 4, 5, 9]
BS = [1, 16, 17, 33]
H = 128


@functools.lru_cache(maxsize=None)
def _inputs(name, T, B):
    """numpy inputs of one case (time-major), drawn once"""
    F, gate, update, preact, bf, gl, bft = CONTRACTS[name]
    rng = np.random.default_rng(1000 * T + B)
    p = O.make_params(F, H, dtype=np.float32, seed=19, randomize_scalars=True)
    if update == "quantTanh":
        p["w"] = (3.0 * p["w"]).astype(np.float32)          # update pre-activations on both sides of the clamp
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    if bf:                                                   # the values the kernel sees
        rnd = lambda a: torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
        x, G = rnd(x), rnd(G)
    if gl:
        G[:-1] = 0.0
    return p, x, G, h0


def _run(name, T, B):
    """forward once; the full backward twice and the backward without d_x once"""
    F, gate, update, preact, bf, gl, bft = CONTRACTS[name]
    p, x, G, h0 = _inputs(name, T, B)
    P = S.cell_tensors(p)
    dt = torch.bfloat16 if bf else torch.float32
    flags = (SP if preact else 0) | (BFT if bft else 0)
    xt = torch.from_numpy(x).to(DEV).to(dt)
    if bft:
        xt = xt.permute(1, 2, 0).contiguous()
    Gt = torch.from_numpy(G[-1] if gl else G).to(DEV).to(dt).contiguous()
    ht = torch.from_numpy(h0).to(DEV)
    code, ucode = S.NONLINEARITY[gate], S.NONLINEARITY[update]
    assert fastgrnn_cuda.kernel_path(T, B, F, H, 0, 0, code, ucode, dt, 1, flags | (GL if gl else 0)) == 2
    outs = S.forward_unroll(xt, ht, P, gate, update=update, flags=flags)

    def bwd(need_dx):
        g = S.backward_of(outs, Gt, xt, ht, P, gate, update=update, flags=flags | (GL if gl else 0), biases=True,
                          need_dx=need_dx)
        return dict(zip(NAMES, g[:8]))

    full, again, nodx = bwd(True), bwd(True), bwd(False)
    torch.cuda.synchronize()
    return outs[0], outs[1], full, again, nodx


def _oracle(name, T, B, hs, pre):
    """the fp64 reference of the contract, as tests/test_hip_parity.py builds it, and its bound"""
    F, gate, update, preact, bf, gl, bft = CONTRACTS[name]
    p, x, G, h0 = _inputs(name, T, B)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    x64, G64, h64 = x.astype(np.float64), G.astype(np.float64), h0.astype(np.float64)
    if bf:
        # the kernel sees the ROUNDED hs as h_prev and the exact pre-activation (bf16_master_grads_case)
        hs_k = hs.to(torch.float64).cpu().numpy()
        pre_k = pre.cpu().numpy().astype(np.float64)
        z_k = 1.0 / (1.0 + np.exp(-(pre_k + p64["bias_gate"])))
        c_k = np.tanh(pre_k + p64["bias_update"])
        return O.unroll_backward(G64, x64, hs_k, z_k, c_k, p64, h64, diagnostics=True), 2e-5
    if update == "quantTanh":
        # the clamp's derivative jumps: the oracle on the kernel's own z, c (test_quant_tanh_update_on_the_matrix_pipe)
        pre_k = pre.cpu().numpy()
        zk = (1.0 / (1.0 + np.exp(-(pre_k + p["bias_gate"]).astype(np.float64)))).astype(np.float32)
        ck = np.clip(pre_k + p["bias_update"], -1, 1).astype(np.float32)
        return O.unroll_backward(G, x, hs.cpu().numpy(), zk, ck, p, h0, gate=gate, update="quantTanh"), 5e-5
    hs_o, zs_o, cs_o = O.unroll_forward(x64, p64, h64, gate=gate)
    if gl:                                                   # test_grad_last_equals_the_dense_zero_padded_gradient
        return O.unroll_backward(G64, x64, hs_o, zs_o, cs_o, p64, h64, gate=gate), 1e-5
    return O.unroll_backward(G64, x64, hs_o, zs_o, cs_o, p64, h64, gate=gate, diagnostics=True), 2e-5


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", list(CONTRACTS))
def test_backward_scan_contracts_at_the_step_order_seams(name, T, B):
    F, gate, update, preact, bf, gl, bft = CONTRACTS[name]
    hs, pre, full, again, nodx = _run(name, T, B)
    # two calls, bit for bit; the call without d_x shares everything but d_x
    assert nodx["d_x"].numel() == 0
    for k in NAMES:
        S.assert_same_bits(again[k], full[k], "second call: " + k)
        if k != "d_x":
            S.assert_same_bits(nodx[k], full[k], "without d_x: " + k)
    # the oracle
    ref, tol = _oracle(name, T, B, hs, pre)
    g = dict(full)
    dx = g.pop("d_x")
    if bft:
        dx = dx.permute(2, 0, 1)
    dx_ref = ref.pop("d_x")
    if bf:
        dx = dx.to(torch.float64).cpu().numpy()
        assert (np.abs(dx - dx_ref) / np.maximum(1.0, np.abs(dx_ref))).max() <= 2.0 ** -8 + 2e-5
    else:
        S.check_grads({"d_x": dx}, {"d_x": dx_ref}, tol=tol, scalar_term_tol=S.SCALAR_TERM_TOL, tag=(name, T, B))
    S.check_grads(g, ref, tol=tol, scalar_term_tol=S.SCALAR_TERM_TOL, tag=(name, T, B))
