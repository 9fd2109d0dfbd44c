"""FASTGRNN_FLAG_NO_INPUT_GRAD on the GPU: the dense H=128 / F=32 backward without the input's gradient.

With the flag, backward_unroll accepts d_x = NULL on this shape and runs a scan variant without the d_x product
(bwd_scan_split_w8<..., NODX = true>).  That variant does the same arithmetic in the same order for everything else,
so every other output must equal the call without the flag bit for bit:

1. The ABI through fastgrnn_cuda.backward_unroll(need_dx=False) for every gate, both saved-tensor contracts,
   quantTanh, fp32 and bf16 sequences, ragged and full batches, time-major / batch-major / [B,F,T] frames and the
   last-state gradient; the flag with d_x given changes nothing at all.
2. The zero-extended route at (F, H) = (32, 100): the plan reports dx_optional, the padded call skips d_x.
3. The modules: FastGRNNCUDA with x.requires_grad False and True, graph replay, repeatability.
"""
import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import layer_cases as LC
from tests import support as S
from tests.support import DEV, GRAD_NAMES as NAMES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNCUDA, GraphedStep, fastgrnn_cuda
SP, BM, BFT, GL, ZE, NIG = (S.FLAG_SAVE_PREACT, S.FLAG_BATCH_MAJOR, S.FLAG_X_BFT, S.FLAG_GRAD_LAST, S.FLAG_ZERO_EXTEND,
                            S.FLAG_NO_INPUT_GRAD)


def _cases():
    """(gate, update, preact, bf16, layout, grad_last, B): the kernel-path-2 backward configurations of H=128 / F=32"""
    out = []
    for gate in ("sigmoid", "relu", "tanh", "quantSigm", "quantSigm4"):
        for update in ("tanh", "quantTanh"):
            if update == "quantTanh" and gate not in ("sigmoid", "quantSigm4"):
                continue
            for preact in (True, False):
                if not preact and (gate.startswith("quant") or update == "quantTanh"):
                    continue                    # quantised cells: the one-saved-tensor contract only
                for bf in (False, True):
                    if bf and (not preact or update == "quantTanh"):
                        continue
                    for layout in ("tm", "bm", "bft"):
                        if layout == "bft" and (not preact or update == "quantTanh"):
                            continue
                        for gl in (False, True):
                            for B in (37, 4096):
                                out.append((gate, update, preact, bf, layout, gl, B))
    return out


CASES = _cases()


def _id(c):
    gate, update, preact, bf, layout, gl, B = c
    return "%s-%s-%s-%s-%s%s-B%d" % (gate, update, "pre" if preact else "pair", "bf16" if bf else "f32", layout,
                                     "-gl" if gl else "", B)


def _params(F, H, seed, relu=False):
    p = O.make_params(F, H, dtype=np.float32, seed=seed, randomize_scalars=True)
    if relu:                                    # an unbounded gate: z = relu(U h + ...) ~ |h| would square h per step
        p["bias_gate"] = (p["bias_gate"] - 1.5).astype(np.float32)
        p["u"] = (0.1 * p["u"]).astype(np.float32)
    return S.cell_tensors(p)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_no_input_grad_leaves_every_other_output_bitwise(case):
    gate, update, preact, bf, layout, gl, B = case
    T, F, H = 13, 32, 128                       # odd T: the scan's virtual step T is in play
    flags = (SP if preact else 0) | (BM if layout == "bm" else 0) | (BFT if layout == "bft" else 0) | (GL if gl else 0)
    dt = torch.bfloat16 if bf else torch.float32
    for direction in (0, 1):
        for f in (flags, flags | NIG):
            assert fastgrnn_cuda.kernel_path(T, B, F, H, 0, 0, S.NONLINEARITY[gate], S.NONLINEARITY[update], dt, direction,
                                             f) == 2
    P = _params(F, H, seed=11 + B % 7, relu=gate == "relu")
    gen = torch.Generator(device="cpu").manual_seed(5)
    xshape = {"tm": (T, B, F), "bm": (B, T, F), "bft": (B, F, T)}[layout]
    x = torch.randn(xshape, generator=gen).to(DEV).to(dt)
    h0 = (0.5 * torch.randn(B, H, generator=gen)).to(DEV)
    gshape = (B, H) if gl else ((B, T, H) if layout == "bm" else (T, B, H))
    G = torch.randn(gshape, generator=gen).to(DEV).to(dt)
    outs = S.forward_unroll(x, h0, P, gate, update=update, flags=flags)
    bwd = lambda fl, need_dx: LC.named_backward(G, x, outs, h0, P, gate, fl, need_dx=need_dx, update=update)
    ref = bwd(flags, True)
    nodx = bwd(flags, False)                    # the shim adds NIG, d_x = NULL
    given = bwd(flags | NIG, True)              # the flag with d_x given
    torch.cuda.synchronize()
    assert nodx["d_x"].numel() == 0 and ref["d_x"].shape == x.shape
    for k in NAMES:
        if ref[k].numel():
            S.assert_same_bits(given[k], ref[k], "flag with d_x given: " + k)
            if k != "d_x":
                S.assert_same_bits(nodx[k], ref[k], k)
    for k in ("d_u", "d_w", "d_h0", "d_zeta"):
        assert torch.isfinite(ref[k]).all(), k


def test_no_input_grad_is_repeatable_at_the_headline_shape():
    T, B, F, H = 99, 4096, 32, 128
    P = _params(F, H, seed=3)
    gen = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(T, B, F, generator=gen).to(DEV)
    h0 = torch.zeros(B, H, device=DEV)
    G = torch.randn(T, B, H, generator=gen).to(DEV)
    outs = S.forward_unroll(x, h0, P, "sigmoid", flags=SP)
    ref = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP, need_dx=True)
    runs = [LC.named_backward(G, x, outs, h0, P, "sigmoid", SP, need_dx=False) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs:
        for k in NAMES[1:8]:
            S.assert_same_bits(r[k], ref[k], k)


def test_zero_extended_route_skips_the_input_gradient():
    T, B, F, H = 11, 37, 32, 100
    assert fastgrnn_cuda.zero_extend_plan(T, B, F, H, flags=SP)["dx_optional"] == 0
    plan = fastgrnn_cuda.zero_extend_plan(T, B, F, H, flags=SP | NIG)
    assert plan["dx_optional"] == 1 and (plan["Hp"], plan["Fp"]) == (128, 32)
    P = _params(F, H, seed=4)
    gen = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(T, B, F, generator=gen).to(DEV)
    h0 = (0.5 * torch.randn(B, H, generator=gen)).to(DEV)
    G = torch.randn(T, B, H, generator=gen).to(DEV)
    outs = S.forward_unroll(x, h0, P, "sigmoid", flags=SP | ZE)
    ref = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP | ZE, need_dx=True)
    nodx = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP | ZE, need_dx=False)
    torch.cuda.synchronize()
    assert nodx["d_x"].numel() == 0
    for k in NAMES[1:8]:
        S.assert_same_bits(nodx[k], ref[k], k)


def _module_grads(m, x, G, requires_grad):
    for q in m.parameters():
        q.grad = None
    xi = x.clone().requires_grad_(requires_grad)
    hs = m(xi)
    hs.backward(G)
    torch.cuda.synchronize()
    return hs.detach().clone(), [q.grad.clone() for q in m.parameters()], xi.grad


@pytest.mark.parametrize("H,batch_first,B", [(128, False, 4096), (128, True, 37), (100, False, 37)],
                         ids=["h128-tm-B4096", "h128-bm-B37", "h100-zext-B37"])
def test_module_parameter_gradients_do_not_depend_on_requires_grad(H, batch_first, B):
    T, F = 23, 32
    torch.manual_seed(6)
    m = FastGRNNCUDA(F, H, batch_first=batch_first, device=DEV)
    x = torch.randn((B, T, F) if batch_first else (T, B, F), device=DEV)
    G = torch.randn((B, T, H) if batch_first else (T, B, H), device=DEV)
    hs1, g1, dx1 = _module_grads(m, x, G, True)
    hs0, g0, dx0 = _module_grads(m, x, G, False)
    assert dx1 is not None and dx0 is None
    S.assert_same_bits(hs0, hs1, "hs")
    for (name, _), a, b in zip(m.named_parameters(), g0, g1):
        S.assert_same_bits(a, b, name)


def test_graph_replay_without_the_input_gradient_matches_eager():
    T, B, F, H = 21, 37, 32, 128
    torch.manual_seed(3)
    m = FastGRNNCUDA(F, H, device=DEV)
    params = list(m.parameters())
    x = torch.randn(T, B, F, device=DEV)           # no requires_grad: the NODX scan
    G = torch.randn(T, B, H, device=DEV)

    def step():
        for q in params:
            q.grad = None
        hs = m(x)
        hs.backward(G)
        return hs

    hs_e = step().detach().clone()
    torch.cuda.synchronize()
    ge = [q.grad.clone() for q in params]
    gs = GraphedStep(step)
    for _ in range(2):
        hs_g = gs()
        torch.cuda.synchronize()
        S.assert_same_bits(hs_g, hs_e, "graph hs")
        for q, v in zip(params, ge):
            S.assert_same_bits(q.grad, v, "graph grad")
