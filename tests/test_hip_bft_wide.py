"""FASTGRNN_FLAG_X_BFT on the GPU for the layers whose frame product is a GEMM of its own: dense H=256 with F=64/128
and dense H=128 with F=64/128/256 (the reference's default features, 32 MFCCs + 32 deltas, into 256 units).

The frame GEMM reads the loader's [B,F,T] frames in place and forms every row's sum as on time-major rows, and the
backward runs on a time-major workspace copy, so EVERY comparison here is exact (bit for bit) between a call fed
[B,F,T] with the flag and the same call fed the time-major copy without it.  The time-major calls are held to the fp64
oracle at full size by tests/test_hip_stack.py.  One comparison is against the reference itself: layer 1 of the delta
model against tests/golden/g13_delta64_l1_f32.npz, under the bounds of test_hip_parity.test_golden_vectors.
"""
import numpy as np
import pytest
import torch

from tests import layer_cases as LC
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNBatchNorm, FastGRNNCUDA, RNNClassifierModel, _lib, fastgrnn_cuda  # noqa: F401
SP, BM, BFT, GL, LAST = S.FLAG_SAVE_PREACT, S.FLAG_BATCH_MAJOR, S.FLAG_X_BFT, S.FLAG_GRAD_LAST, S.FLAG_HS_LAST
SHAPES = [(256, 64), (256, 128), (128, 64), (128, 128), (128, 256)]          # (H, F)
# ragged and full batches; T below, at and across a 32-row stage of the frame GEMM; stages that straddle utterances
SIZES = [(23, 37), (33, 64), (99, 16), (1, 5)]


@pytest.mark.parametrize("T,B", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("H,F", SHAPES, ids=lambda v: str(v))
def test_operator_bitwise_equal_to_the_time_major_call(H, F, T, B):
    x, xb, h0, G = LC.bft_data(T, B, F, H)
    P = LC.bft_params(F, H, seed=11 + B % 7)
    for direction, fl in ((0, BFT), (0, BFT | SP), (0, BFT | LAST), (0, BFT | BM), (1, BFT | SP), (1, BFT | SP | GL), (1, BFT)):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=direction, flags=fl) == 2, (direction, fl)
    # hs alone
    hs_only = lambda xi, fl: S.forward_unroll(xi, h0, P, "sigmoid", flags=fl, want_gates=False)[0]
    S.assert_same_bits(hs_only(xb, BFT), hs_only(x, 0), "hs alone")
    # the one-saved-tensor contract: hs, the pre-activation, every gradient
    o_tm, o_bft = S.forward_unroll(x, h0, P, "sigmoid", flags=SP), S.forward_unroll(xb, h0, P, "sigmoid", flags=SP | BFT)
    assert len(o_tm) == len(o_bft) == 2
    S.assert_same_bits(o_bft[0], o_tm[0], "preact hs"); S.assert_same_bits(o_bft[1], o_tm[1], "preact z")
    LC.compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, "sigmoid", SP, "preact")
    # ... with the gradient of the last state alone
    LC.compare_bft_backward(G[-1].contiguous(), x, xb, o_tm, o_bft, h0, P, "sigmoid", SP | GL, "grad_last")
    # the reference's (z_s, h_prime_s) pair
    o_tm, o_bft = S.forward_unroll(x, h0, P, "sigmoid"), S.forward_unroll(xb, h0, P, "sigmoid", flags=BFT)
    for a, b, n in zip(o_bft, o_tm, ("hs", "z_s", "h_prime_s")):
        S.assert_same_bits(a, b, "pair " + n)
    LC.compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, "sigmoid", 0, "pair")
    # h_T alone
    S.assert_same_bits(hs_only(xb, BFT | LAST), hs_only(x, LAST), "hs_last")
    # batch-major sequences from [B,F,T] frames: hs alone and with the saved pre-activation
    xbm = x.transpose(0, 1).contiguous()
    S.assert_same_bits(hs_only(xb, BFT | BM), hs_only(xbm, BM), "bm hs")
    o_tm = S.forward_unroll(xbm, h0, P, "sigmoid", flags=BM | SP)
    o_bft = S.forward_unroll(xb, h0, P, "sigmoid", flags=BFT | BM | SP)
    S.assert_same_bits(o_bft[0], o_tm[0], "bm preact hs"); S.assert_same_bits(o_bft[1], o_tm[1], "bm preact z")


@pytest.mark.parametrize("gate", ["relu", "tanh", "quantSigm"])
@pytest.mark.parametrize("H,F", SHAPES, ids=lambda v: str(v))
def test_operator_other_gates(H, F, gate):
    T, B = (6, 37) if gate == "relu" else (12, 37)           # gates that do not bound h: short sequences
    x, xb, h0, G = LC.bft_data(T, B, F, H, seed=8)
    P = LC.bft_params(F, H, seed=4, gate=gate)
    o_tm, o_bft = S.forward_unroll(x, h0, P, gate, flags=SP), S.forward_unroll(xb, h0, P, gate, flags=SP | BFT)
    S.assert_same_bits(o_bft[0], o_tm[0], "hs"); S.assert_same_bits(o_bft[1], o_tm[1], "z")
    LC.compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, gate, SP, gate)
    S.assert_same_bits(S.forward_unroll(xb, h0, P, gate, flags=BFT, want_gates=False)[0],
                       S.forward_unroll(x, h0, P, gate, want_gates=False)[0], "hs alone")


@pytest.mark.parametrize("H,F", SHAPES, ids=lambda v: str(v))
def test_scaled_forward_bitwise(H, F):
    """fastgrnn_hip_forward_unroll_affine (an eval-mode BatchNorm cell, folded) from [B,F,T] frames"""
    T, B = 33, 37
    x, xb, h0, _ = LC.bft_data(T, B, F, H, seed=2)
    P = LC.bft_params(F, H, seed=6)
    gen = torch.Generator(device="cpu").manual_seed(1)
    sg = (1.0 + 0.3 * torch.randn(H, generator=gen)).to(DEV)
    sc = (1.0 + 0.3 * torch.randn(H, generator=gen)).to(DEV)
    run = lambda inp, fl: fastgrnn_cuda.forward_unroll_affine(inp, P["w"], P["u"], P["bias_gate"], P["bias_update"],
                                                              P["zeta"], P["nu"], sg, sc, h0, 0, 2, fl)
    for fl in (0, LAST):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, flags=fl | BFT | _lib.FLAG_PREACT_AFFINE) == 2
        S.assert_same_bits(run(xb, fl | BFT), run(x, fl), "affine flags=%d" % fl)
        S.assert_same_bits(run(xb, fl | BFT | BM), run(x.transpose(0, 1).contiguous(), fl | BM), "affine bm flags=%d" % fl)


@pytest.mark.parametrize("H,F,w_rank,u_rank", [(128, 64, 8, None), (256, 64, 40, 40)], ids=["h128-w8", "h256-r40"])
def test_multiplied_out_factorised_cells_inherit_the_flag(H, F, w_rank, u_rank):
    T, B = 23, 37
    assert fastgrnn_cuda.kernel_path(T, B, F, H, w_rank or 0, u_rank or 0, direction=1, flags=SP | BFT) == 2
    x, xb, h0, G = LC.bft_data(T, B, F, H, seed=3)
    P = LC.bft_params(F, H, seed=9, w_rank=w_rank, u_rank=u_rank)
    o_tm, o_bft = S.forward_unroll(x, h0, P, "sigmoid", flags=SP), S.forward_unroll(xb, h0, P, "sigmoid", flags=SP | BFT)
    S.assert_same_bits(o_bft[0], o_tm[0], "hs"); S.assert_same_bits(o_bft[1], o_tm[1], "z")
    LC.compare_bft_backward(G, x, xb, o_tm, o_bft, h0, P, "sigmoid", SP, "densified", dx_optional=False)


def test_full_size_first_layer():
    T, B, F, H = 99, 4096, 64, 256
    x, xb, h0, G = LC.bft_data(T, B, F, H, seed=1)
    P = LC.bft_params(F, H, seed=2)
    o_tm, o_bft = S.forward_unroll(x, h0, P, "sigmoid", flags=SP), S.forward_unroll(xb, h0, P, "sigmoid", flags=SP | BFT)
    S.assert_same_bits(o_bft[0], o_tm[0], "hs"); S.assert_same_bits(o_bft[1], o_tm[1], "z")
    ref = LC.named_backward(G, x, o_tm, h0, P, "sigmoid", SP, need_dx=False)
    got = LC.named_backward(G, xb, o_bft, h0, P, "sigmoid", SP | BFT, need_dx=False)
    torch.cuda.synchronize()
    assert got["d_x"].numel() == 0
    for k in S.GRAD_NAMES[1:8]:
        S.assert_same_bits(got[k], ref[k], k)


def test_same_bits_after_cu_state_is_poisoned():
    """The new staging code reads no LDS it did not write: NaNs left in every CU's LDS and registers change nothing."""
    T, B, F, H = 33, 37, 64, 256
    x, xb, h0, G = LC.bft_data(T, B, F, H, seed=7)
    P = LC.bft_params(F, H, seed=3)
    o_tm = S.forward_unroll(x, h0, P, "sigmoid", flags=SP)
    ref = LC.named_backward(G, x, o_tm, h0, P, "sigmoid", SP)
    torch.cuda.synchronize()
    assert _lib.load().fastgrnn_hip_debug_poison_cu_state(0x7fc00000, None) == 0
    o_bft = S.forward_unroll(xb, h0, P, "sigmoid", flags=SP | BFT)
    assert _lib.load().fastgrnn_hip_debug_poison_cu_state(0x7fc00000, None) == 0
    got = LC.named_backward(G, xb, o_bft, h0, P, "sigmoid", SP | BFT)
    torch.cuda.synchronize()
    S.assert_same_bits(o_bft[0], o_tm[0], "hs"); S.assert_same_bits(o_bft[1], o_tm[1], "z")
    S.assert_same_bits(got["d_x"], ref["d_x"].permute(1, 2, 0), "d_x")
    for k in S.GRAD_NAMES[1:8]:
        S.assert_same_bits(got[k], ref[k], k)


# ---- modules ------------------------------------------------------------------------------------------------
class _Spy:
    """Records (input, flags) of every call of a fastgrnn_cuda entry point and passes it on."""

    def __init__(self, monkeypatch, name, flags_pos=None):
        self.calls, self._orig, self._pos = [], getattr(fastgrnn_cuda, name), flags_pos
        monkeypatch.setattr(fastgrnn_cuda, name, self)

    def __call__(self, *a, **k):
        flags = a[self._pos] if self._pos is not None else k.get("flags", 0)
        self.calls.append((a[0], int(flags)))
        return self._orig(*a, **k)


def _module_run(m, audio, G, copy):
    for q in m.parameters():
        q.grad = None
    a = audio.clone().requires_grad_(True)
    view = a.permute(2, 0, 1)                                  # what the trainer hands over (trainClassifier.py:204)
    hs = m(view.contiguous() if copy else view)
    hs.backward(G)
    torch.cuda.synchronize()
    return a, hs.detach().clone(), [q.grad.clone() for q in m.parameters()], a.grad.clone()


@pytest.mark.parametrize("F,H", [(64, 256), (64, 128)])
def test_module_takes_the_trainers_view_without_a_copy(F, H, monkeypatch):
    T, B = 23, 37
    torch.manual_seed(4)
    m = FastGRNNCUDA(F, H, device=DEV)
    audio = torch.randn(B, F, T, device=DEV)
    G = torch.randn(T, B, H, device=DEV)
    _, hs_c, g_c, dx_c = _module_run(m, audio, G, copy=True)
    spy = _Spy(monkeypatch, "forward_unroll")
    a, hs_v, g_v, dx_v = _module_run(m, audio, G, copy=False)
    (inp, flags), = spy.calls
    assert flags & BFT and flags & SP
    assert inp.data_ptr() == a.data_ptr() and tuple(inp.shape) == (B, F, T) and inp.is_contiguous()
    S.assert_same_bits(hs_v, hs_c, "hs"); S.assert_same_bits(dx_v, dx_c, "audio.grad")
    for (name, _), u, v in zip(m.named_parameters(), g_v, g_c):
        S.assert_same_bits(u, v, name)


@pytest.mark.parametrize("F,H", [(64, 256), (32, 128)])
@pytest.mark.parametrize("last_state", [False, True])
def test_module_inference_takes_the_view_and_saves_nothing(F, H, last_state, monkeypatch):
    T, B = 23, 37
    torch.manual_seed(5)
    m = FastGRNNCUDA(F, H, device=DEV)
    audio = torch.randn(B, F, T, device=DEV)
    view = audio.permute(2, 0, 1)
    with torch.no_grad():
        ref = m(view.contiguous(), last_state=last_state)
        spy = _Spy(monkeypatch, "forward_unroll")
        out = m(view, last_state=last_state)
    torch.cuda.synchronize()
    (inp, flags), = spy.calls
    assert flags & BFT and not flags & SP and bool(flags & LAST) == last_state
    assert inp.data_ptr() == audio.data_ptr() and tuple(inp.shape) == (B, F, T)
    assert tuple(out.shape) == ((B, H) if last_state else (T, B, H))
    S.assert_same_bits(out, ref, "no_grad output")


def test_delta_model_training_step_from_the_view():
    T, B, C = 23, 37, 12
    torch.manual_seed(6)
    model = RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None, None], [None, None], [1.0, 1.0], [1.0, 1.0],
                               "sigmoid", "tanh", num_classes=C, device=DEV)
    audio = torch.randn(B, 64, T, device=DEV)
    y = torch.randint(0, C, (B,), device=DEV)

    def step(xin):
        for q in model.parameters():
            q.grad = None
        model.init_hidden()
        loss = model.loss(xin, y)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [q.grad.clone() for q in model.parameters()]

    l_c, g_c = step(audio.permute(2, 0, 1).contiguous())
    l_v, g_v = step(audio.permute(2, 0, 1))
    S.assert_same_bits(l_v.reshape(1), l_c.reshape(1), "loss")
    for (name, _), u, v in zip(model.named_parameters(), g_v, g_c):
        S.assert_same_bits(u, v, name)


def test_delta_layer1_against_the_reference_cell():
    """tests/golden/g13_delta64_l1_f32.npz (T=99, B=4, F=64, H=256, written from the reference's own cell), fed as
    [B,F,T] with the flag, under the bounds tests/test_hip_parity.py::test_golden_vectors holds every golden to."""
    from tests.conftest import load_golden
    g = load_golden("g13_delta64_l1_f32")
    T, B, F = g["x"].shape
    H = g["h0"].shape[-1]
    assert (T, B, F, H) == (99, 4, 64, 256) and g["dtype"] != "f64"
    P = S.cell_tensors(g["params"])
    xb = S.to_dev(g["x"]).permute(1, 2, 0).contiguous()
    h0, G = S.to_dev(g["h0"]), S.to_dev(g["G"])
    for direction in (0, 1):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=S.NONLINEARITY[g["gate"]], direction=direction, flags=BFT) == 2
    outs = S.forward_unroll(xb, h0, P, g["gate"], flags=BFT)
    grads = LC.named_backward(G, xb, outs, h0, P, g["gate"], BFT)
    torch.cuda.synchronize()
    err = float(np.abs(outs[0].cpu().numpy() - g["hs"]).max())
    print("g13 [B,F,T]: max|hs - reference| %.3g (bound 1e-5)" % err)
    assert err <= 1e-5
    got = {k: v.cpu().numpy() for k, v in grads.items() if v.numel()}
    got["d_x"] = grads["d_x"].permute(2, 0, 1).contiguous().cpu().numpy()
    ref = dict(g["dparams"]); ref["d_x"] = g["dx"]; ref["d_h0"] = g["dh0"]
    g_o = S.oracle64(g["x"], g["G"], g["params"], g["h0"], g["gate"], g["update"])[3]
    ref["_abs_zeta"], ref["_abs_nu"] = g_o["_abs_zeta"], g_o["_abs_nu"]
    S.check_grads(got, ref, tol=2e-5, scalar_term_tol=S.SCALAR_TERM_TOL, tag="g13 [B,F,T]")


def test_trained_batchnorm_model_takes_the_view_on_layer_1(monkeypatch):
    from tests import batchnorm_golden as BG
    d, full = BG.trained_state_dict()
    m = BG.build_model(DEV)
    m.load_state_dict(full, strict=True)
    m.eval()
    x = torch.from_numpy(d["x"]).to(DEV)                       # [T,B,64]
    audio = x.permute(1, 2, 0).contiguous()
    m.init_hidden()
    ref = m(audio.permute(2, 0, 1).contiguous()).detach().clone()
    ref_states = [h.clone() for h in m.hidden_states]
    spy = _Spy(monkeypatch, "forward_unroll_affine", flags_pos=12)
    m.init_hidden()
    out = m(audio.permute(2, 0, 1)).detach()
    torch.cuda.synchronize()
    assert len(spy.calls) == 3
    (i1, f1), (_, f2), (_, f3) = spy.calls
    assert f1 & BFT and not f2 & BFT and not f3 & BFT
    assert i1.data_ptr() == audio.data_ptr() and tuple(i1.shape) == tuple(audio.shape)
    S.assert_same_bits(out, ref, "log-probs")
    for l, (a, b) in enumerate(zip(m.hidden_states, ref_states)):
        S.assert_same_bits(a, b, "layer %d state" % l)
