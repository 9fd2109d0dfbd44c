"""The 12-wave backward of dense H=128 / F=32 without the input's gradient (bwd_scan_split_w12).

Waves 0-7 are the 8-wave scan's recurrence without its weight-gradient phase; waves 8-11, one per SIMD, contract dW and
dU beside them -- the same batches per iteration, the same addends per accumulator in the same order.  So every output
of the default route must have the bits of the 8-wave kernel's, which FASTGRNN_FLAG_BWD_8WAVE still selects:

1. Bit equality of all twelve outputs between the two routes, for every arm the kernel is built for (sigmoid / relu /
   tanh gate, both saved-tensor contracts, fp32 sequences) and three arms that stay on 8 waves, at T in
   {1, 2, 3, 4, 5, 8} -- odd and even T, the peeled iteration, the virtual step, the tail pair (1, 0) alone, every image
   buffer -- and B in {1, 16, 17, 33} -- a lone ragged tile, a full one, full + ragged, two full + ragged; h0 is
   nonzero throughout.  FLAG_GRAD_LAST and FLAG_X_BFT on one case each.
2. The fp64 oracle at T = 5, B = 33 for every arm the kernel is built for, at the bound of tests/test_hip_parity.py
   (2e-5, the scalar-term rule for d_zeta / d_nu; relu with its gates off the kink, as there).
3. The same call twice in one process gives the same bits.
"""
import numpy as np
import pytest
import torch

from kws_amd import _lib
from oracle import fastgrnn_oracle as O
from tests import layer_cases as LC
from tests import support as S
from tests.support import DEV, GRAD_NAMES as NAMES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import fastgrnn_cuda

SP, BFT, GL, W8 = S.FLAG_SAVE_PREACT, S.FLAG_X_BFT, S.FLAG_GRAD_LAST, _lib.AB_BWD_8WAVE
F, H = 32, 128
TS = (1, 2, 3, 4, 5, 8)
BS = (1, 16, 17, 33)


# (gate, update, preact, bf16).  The kernel is built for the first six (bwd_w12_built in kernels_split.hip: the
# reference's gates, tanh update, fp32 sequences, both saved-tensor contracts); the last three -- bf16 sequences, the
# quantTanh update, a quantised gate -- stay on 8 waves, where the flag must change nothing.
ARMS = [(gate, "tanh", preact, False) for gate in ("sigmoid", "relu", "tanh") for preact in (True, False)] + [
    ("sigmoid", "tanh", True, True), ("sigmoid", "quantTanh", True, False), ("quantSigm4", "tanh", True, False)]
HEADLINE = ARMS[0]


def _arm_id(a):
    gate, update, preact, bf = a
    return "%s-%s-%s-%s" % (gate, update, "pre" if preact else "pair", "bf16" if bf else "f32")


def _params(seed, relu=False):
    p = O.make_params(F, H, dtype=np.float32, seed=seed, randomize_scalars=True)
    if relu:                                    # an unbounded gate: z = relu(U h + ...) ~ |h| would square h per step
        p["bias_gate"] = (p["bias_gate"] - 1.5).astype(np.float32)
        p["u"] = (0.1 * p["u"]).astype(np.float32)
    return p


def _both_routes(arm, T, B, extra=0, bft=False):
    """The twelve outputs of the default route and of FASTGRNN_FLAG_BWD_8WAVE on one forward's saved tensors."""
    gate, update, preact, bf = arm
    flags = (SP if preact else 0) | extra | (BFT if bft else 0)
    dt = torch.bfloat16 if bf else torch.float32
    assert fastgrnn_cuda.kernel_path(T, B, F, H, 0, 0, S.NONLINEARITY[gate], S.NONLINEARITY[update], dt, 1,
                                     flags | S.FLAG_NO_INPUT_GRAD) == 2
    P = S.cell_tensors(_params(11 + B % 7, relu=gate == "relu"))
    gen = torch.Generator(device="cpu").manual_seed(100 * T + B)
    x = torch.randn((B, F, T) if bft else (T, B, F), generator=gen).to(DEV).to(dt)
    h0 = (0.5 * torch.randn(B, H, generator=gen)).to(DEV)
    G = torch.randn((B, H) if extra & GL else (T, B, H), generator=gen).to(DEV).to(dt)
    outs = S.forward_unroll(x, h0, P, gate, update=update, flags=flags)
    new = LC.named_backward(G, x, outs, h0, P, gate, flags, need_dx=False, update=update)
    old = LC.named_backward(G, x, outs, h0, P, gate, flags | W8, need_dx=False, update=update)
    torch.cuda.synchronize()
    return new, old


def _assert_routes_agree(new, old, tag):
    assert new["d_x"].numel() == 0 and old["d_x"].numel() == 0, tag
    for k in NAMES:
        S.assert_same_bits(new[k], old[k], "%s %s" % (tag, k))
    for k in ("d_u", "d_w", "d_h0", "d_bias_gate", "d_bias_update", "d_zeta", "d_nu"):
        assert new[k].numel() and torch.isfinite(new[k]).all(), (tag, k)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("arm", ARMS, ids=_arm_id)
def test_helper_waves_give_the_8wave_kernels_bits(arm, T):
    for B in BS:
        new, old = _both_routes(arm, T, B)
        _assert_routes_agree(new, old, "%s T%d B%d" % (_arm_id(arm), T, B))


def test_last_state_gradient_alone():
    new, old = _both_routes(HEADLINE, 5, 33, extra=GL)
    _assert_routes_agree(new, old, "grad_last")


def test_frames_in_the_loaders_layout():
    new, old = _both_routes(HEADLINE, 5, 33, bft=True)
    _assert_routes_agree(new, old, "x_bft")


@pytest.fixture(scope="module")
def oracle_case():
    """T = 5, B = 33: one set of inputs per gate and its fp64 gradients, shared by both saved-tensor contracts."""
    T, B = 5, 33
    made = {}

    def get(gate):
        if gate not in made:
            rng = np.random.default_rng(7)
            p = _params(13, relu=gate == "relu")
            x = rng.standard_normal((T, B, F)).astype(np.float32)
            h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
            G = rng.standard_normal((T, B, H)).astype(np.float32)
            if gate == "relu":
                p = S.keep_relu_gates_off_the_kink(p, x, h0)
            g_o = dict(S.oracle64(x, G, p, h0, gate)[3])
            del g_o["d_x"]                      # not computed on this route
            made[gate] = (p, x, h0, G, g_o)
        return made[gate]
    return get


@pytest.mark.parametrize("preact", [True, False], ids=["pre", "pair"])
@pytest.mark.parametrize("gate", ["sigmoid", "tanh", "relu"])
def test_against_the_fp64_oracle(oracle_case, gate, preact):
    p, x, h0, G, g_o = oracle_case(gate)
    flags = SP if preact else 0
    P, xt, ht, Gt = S.cell_tensors(p), S.to_dev(x), S.to_dev(h0), S.to_dev(G)
    outs = S.forward_unroll(xt, ht, P, gate, flags=flags)
    got = LC.named_backward(Gt, xt, outs, ht, P, gate, flags, need_dx=False)
    torch.cuda.synchronize()
    assert got["d_x"].numel() == 0
    S.check_grads(got, g_o, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag="%s preact=%s" % (gate, preact))


@pytest.mark.parametrize("B", [33, 4096])
def test_the_same_call_twice_gives_the_same_bits(B):
    T = 99 if B == 4096 else 5                  # the headline shape (one workgroup per CU) and the small one
    P = S.cell_tensors(_params(3))
    gen = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(T, B, F, generator=gen).to(DEV)
    h0 = (0.5 * torch.randn(B, H, generator=gen)).to(DEV)
    G = torch.randn(T, B, H, generator=gen).to(DEV)
    outs = S.forward_unroll(x, h0, P, "sigmoid", flags=SP)
    a = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP, need_dx=False)
    b = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP, need_dx=False)
    old = LC.named_backward(G, x, outs, h0, P, "sigmoid", SP | W8, need_dx=False)
    torch.cuda.synchronize()
    for k in NAMES:
        S.assert_same_bits(a[k], b[k], "twice: " + k)
        S.assert_same_bits(a[k], old[k], "8-wave: " + k)
