"""GPU tests for the reference's default stack (trainingConfig.py:12-15: dense 32 -> 256 -> 128, model.py:196-203):
the wide-input layer (H=128, F=256 and its siblings F=64/128: recurrence-only scans + batched split-precision GEMMs),
the H=256 layer, and the layers chained through ``kws_amd.RNNClassifierModel`` against the fixture made from the
reference's own cells (tests/golden/g12_stack2_f64.npz) and the fp64 oracle.  All through the C ABI."""
import numpy as np
import pytest
import torch

from oracle import fastgrnn_oracle as O
from tests import layer_cases as LC
from tests import support as S
from tests.support import DEV

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNCUDA, RNNClassifierModel, _lib, fastgrnn_cuda


WIDE = [  # T, B, F, H, preact
    (99, 64, 256, 128, True), (99, 50, 256, 128, True), (23, 37, 256, 128, False), (12, 16, 128, 128, True),
    (7, 33, 64, 128, True), (1, 5, 256, 128, True), (2, 1, 256, 128, False), (6, 130, 128, 128, False),
    (99, 32, 32, 256, True), (24, 37, 32, 256, True), (9, 16, 32, 256, False), (1, 3, 32, 256, True), (2, 50, 32, 256, False),
    # the reference's default feature width: 32 MFCCs + 32 deltas (trainingConfig.py:36) into 256 units, and 128 inputs
    (99, 64, 64, 256, True), (24, 37, 64, 256, True), (9, 16, 64, 256, False), (1, 3, 64, 256, True), (17, 50, 128, 256, True),
    (5, 20, 128, 256, False),
]


@pytest.mark.parametrize("case", WIDE, ids=lambda c: "T%dB%dF%dH%d%s" % (c[0], c[1], c[2], c[3], "p" if c[4] else "r"))
def test_stack_layer_shapes_on_the_matrix_pipe_vs_oracle(case):
    T, B, F, H, preact = case
    flags = _lib.FLAG_SAVE_PREACT if preact else 0
    for direction in (0, 1):
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=direction, flags=flags) == 2, (case, direction)
    rng = np.random.default_rng(1000 + T * 7 + B + F)
    p = O.make_params(F, H, dtype=np.float32, seed=31, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=preact)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    if preact:
        assert np.abs(outs[1].cpu().numpy() - S.dense_preactivation64(x, p, h0, hs_o)).max() <= 1e-5
    else:
        assert np.abs(outs[1].cpu().numpy() - zs_o).max() <= 1e-5 and np.abs(outs[2].cpu().numpy() - cs_o).max() <= 1e-5
    S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0, tag=case)


@pytest.mark.parametrize("F,H", [(256, 128), (32, 256), (64, 256)])
@pytest.mark.parametrize("gate", ["tanh", "relu", "quantSigm"])
def test_stack_layer_shapes_other_gates(F, H, gate):
    T, B = 8, 37
    code = O.GATE_CODES[gate]
    rng = np.random.default_rng(5)
    p = O.make_params(F, H, dtype=np.float32, seed=33, randomize_scalars=True)
    for k in ("w", "u"):
        p[k] = (0.3 * p[k]).astype(np.float32)
    p["bias_gate"] = (0.3 * p["bias_gate"] - 0.1).astype(np.float32)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=code, direction=1, flags=_lib.FLAG_SAVE_PREACT) == 2
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, gate=code, preact=True)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0, gate=gate)
    assert (np.abs(outs[0].cpu().numpy() - hs_o) / np.maximum(1.0, np.abs(hs_o))).max() <= 1e-5
    if gate != "tanh":     # piecewise-linear gates: same mask as the kernel (the oracle in fp32 on the kernel's own states)
        pre = outs[1].cpu().numpy()
        zk = O.nonlinearity(pre + p["bias_gate"], gate).astype(np.float32)
        ck = np.tanh(pre + p["bias_update"]).astype(np.float32)
        g_o = O.unroll_backward(G, x, outs[0].cpu().numpy(), zk, ck, p, h0, gate=gate)
        S.check_grads(gr, g_o, tol=5e-5, scalar_term_tol=0.0, tag=gate)
    else:
        S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0, tag=gate)


@pytest.mark.parametrize("F,H", [(256, 128), (32, 256), (64, 256)])
def test_stack_layer_batch_major_and_last_state_contracts(F, H):
    """FLAG_BATCH_MAJOR is bit-equal to the time-major run; FLAG_GRAD_LAST equals the dense zero-padded gradient;
    FLAG_HS_LAST returns the last row of the full forward."""
    T, B = 21, 37
    rng = np.random.default_rng(9)
    p = O.make_params(F, H, dtype=np.float32, seed=35, randomize_scalars=True)
    P = S.cell_tensors(p)
    x = S.to_dev(rng.standard_normal((T, B, F)).astype(np.float32))
    h0 = S.to_dev((0.5 * rng.standard_normal((B, H))).astype(np.float32))
    G = S.to_dev(rng.standard_normal((T, B, H)).astype(np.float32))
    outs, gr = LC.layer_fwd_bwd(x, h0, G, p, preact=True)
    # (round 3: the H = 256 scans index [B,T,.] in place too -- two-stride rows, the d_pre workspace in the sequences'
    # row order, and a dU GEMM that takes every T-th row of H_prev from h0)
    xb, Gb = x.transpose(0, 1).contiguous(), G.transpose(0, 1).contiguous()
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=0, flags=_lib.FLAG_SAVE_PREACT | _lib.FLAG_BATCH_MAJOR) == 2
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=_lib.FLAG_SAVE_PREACT | _lib.FLAG_BATCH_MAJOR) == 2
    outs_b, gr_b = LC.layer_fwd_bwd(xb, h0, Gb, p, flags=_lib.FLAG_BATCH_MAJOR, preact=True)
    assert torch.equal(outs_b[0].transpose(0, 1), outs[0]) and torch.equal(outs_b[1].transpose(0, 1), outs[1])
    assert torch.equal(gr_b[0].transpose(0, 1), gr[0])
    for k, (a, b) in enumerate(zip(gr[1:8], gr_b[1:8])):
        if k == 5 or (k == 6 and H == 256):   # d_w (d_u): the TN GEMM sums the rows in memory order, which differs between the layouts
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max())), k
        else:
            assert torch.equal(a, b), k
    if H == 256:
        # the reference operator's own contract (z_s and h_prime_s saved) in place as well, and the last-state pair
        outs_z, gr_z = LC.layer_fwd_bwd(x, h0, G, p)
        outs_zb, gr_zb = LC.layer_fwd_bwd(xb, h0, Gb, p, flags=_lib.FLAG_BATCH_MAJOR)
        for a, b in zip(outs_z, outs_zb):
            assert torch.equal(b.transpose(0, 1), a)
        assert torch.equal(gr_zb[0].transpose(0, 1), gr_z[0]) and torch.equal(gr_zb[5], gr_z[5])
        for k in (6, 7):
            assert float((gr_zb[k] - gr_z[k]).abs().max()) <= 2e-6 * max(1.0, float(gr_z[k].abs().max())), k
        fb = _lib.FLAG_SAVE_PREACT | _lib.FLAG_BATCH_MAJOR | _lib.FLAG_GRAD_LAST
        assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=fb) == 2
        got = S.backward_of(outs_b, G[-1].contiguous(), xb, h0, P, "sigmoid", flags=fb, biases=True)
        Gl0 = torch.zeros_like(G); Gl0[-1] = G[-1]
        want = S.backward_of(outs, Gl0, x, h0, P, "sigmoid", flags=_lib.FLAG_SAVE_PREACT, biases=True)
        assert torch.equal(got[0].transpose(0, 1), want[0]) and torch.equal(got[5], want[5])
        for k in (6, 7):
            assert float((got[k] - want[k]).abs().max()) <= 2e-6 * max(1.0, float(want[k].abs().max())), k
    # last-state gradient
    Gl = torch.zeros_like(G); Gl[-1] = G[-1]
    fl = _lib.FLAG_SAVE_PREACT
    ref = S.backward_of(outs, Gl, x, h0, P, "sigmoid", flags=fl, biases=True)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=fl | _lib.FLAG_GRAD_LAST) == 2
    got = S.backward_of(outs, G[-1].contiguous(), x, h0, P, "sigmoid", flags=fl | _lib.FLAG_GRAD_LAST, biases=True)
    for a, b in zip(ref[:8], got[:8]):
        assert torch.equal(a, b)
    # inference: h_T only
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=0, flags=_lib.FLAG_HS_LAST) == 2
    hT = S.forward_unroll(x, h0, P, "sigmoid", want_gates=False, flags=_lib.FLAG_HS_LAST)[0]
    assert hT.shape == (B, H) and float((hT - outs[0][-1]).abs().max()) <= 2e-6


@pytest.mark.parametrize("F,H", [(256, 128), (32, 256), (64, 256)])
def test_stack_layer_full_batch_every_output_vs_fp64_oracle(F, H):
    """B = 4096, T = 99 for each layer of the default stack: every output against the fp64 oracle."""
    T, B = 99, 4096
    rng = np.random.default_rng(77 + F)
    p = O.make_params(F, H, dtype=np.float32, seed=37, randomize_scalars=True)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    h0 = np.zeros((B, H), np.float32)
    assert fastgrnn_cuda.kernel_path(T, B, F, H, direction=1, flags=_lib.FLAG_SAVE_PREACT) == 2
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=True)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    # (the stack's first layer, F = 32 / H = 256: plain 2e-5; layers with a wide input: the conditioning-aware bound too)
    errs = S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0 if (F, H) == (32, 256) else S.SCALAR_TERM_TOL,
                         tag=(F, H))
    print("stack layer F=%d H=%d full-size errors: %s" % (F, H, {k: "%.2e" % v for k, v in errs.items()}))


def _build_model(g, dtype=torch.float32):
    hidden = g["hidden"]
    m = RNNClassifierModel("FastGRNNCUDA", g["x"].shape[2], len(hidden), hidden, [None] * len(hidden), [None] * len(hidden),
                           [1.0] * len(hidden), [1.0] * len(hidden), "sigmoid", "tanh", num_classes=g["fc_w"].shape[0],
                           device=DEV)
    with torch.no_grad():
        for rnn, (p, _) in zip(m.rnn_list, g["layers"]):
            S.copy_cell_params(rnn, {k: v.astype(np.float32) for k, v in p.items()})
        m.hidden2keyword.weight.copy_(S.to_dev(g["fc_w"].astype(np.float32)))
        m.hidden2keyword.bias.copy_(S.to_dev(g["fc_b"].astype(np.float32)))
    return m


@pytest.mark.parametrize("fused_head", [False, True])
def test_two_layer_model_matches_the_reference_cells_chained(stack_golden, fused_head):
    """kws_amd.RNNClassifierModel (32 -> 256 -> 128 -> Linear -> log_softmax -> NLLLoss) in fp32 against the fp64
    fixture produced by chaining the reference's own cells: scores, loss and every gradient."""
    g = stack_golden
    m = _build_model(g)
    for l, rnn in enumerate(m.rnn_list):
        F_l = g["x"].shape[2] if l == 0 else g["hidden"][l - 1]
        assert fastgrnn_cuda.kernel_path(g["x"].shape[0], g["x"].shape[1], F_l, g["hidden"][l], direction=1,
                                         flags=_lib.FLAG_SAVE_PREACT) == 2
    x = S.to_dev(g["x"].astype(np.float32)).requires_grad_(True)
    y = S.to_dev(g["labels"])
    m.init_hidden()
    if fused_head:
        loss = m.loss(x, y)
    else:
        scores = m(x)
        assert np.abs(scores.detach().cpu().numpy() - g["scores"]).max() <= 1e-5
        loss = torch.nn.NLLLoss()(scores, y)
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) <= 1e-5
    rel = lambda a, ref: float(np.abs(a.detach().cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    assert rel(x.grad, g["dx"]) <= 2e-5
    assert rel(m.hidden2keyword.weight.grad, g["dfc_w"]) <= 2e-5 and rel(m.hidden2keyword.bias.grad, g["dfc_b"]) <= 2e-5
    for rnn, (_, dp) in zip(m.rnn_list, g["layers"]):
        for name, par in (("d_w", rnn.W), ("d_u", rnn.U), ("d_bias_gate", rnn.bias_gate), ("d_bias_update", rnn.bias_update),
                          ("d_zeta", rnn.zeta), ("d_nu", rnn.nu)):
            assert rel(par.grad, dp[name]) <= 2e-5, name


def test_two_layer_model_full_batch_vs_fp64_oracle_and_inference_path():
    """B = 4096: loss, d_x and every parameter gradient of the 2-layer model against the fp64 oracle of the stack;
    under no_grad the same scores come out of the inference path (top layer without its hidden-state sequence)."""
    T, B, F, C = 99, 4096, 32, 12
    hidden = [256, 128]
    rng = np.random.default_rng(123)
    layers = [O.make_params(F, 256, dtype=np.float32, seed=41, randomize_scalars=True),
              O.make_params(256, 128, dtype=np.float32, seed=42, randomize_scalars=True)]
    fc_w = (0.2 * rng.standard_normal((C, 128))).astype(np.float32)
    fc_b = (0.1 * rng.standard_normal((C,))).astype(np.float32)
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    y = rng.integers(0, C, (B,))
    g = {"hidden": hidden, "x": x, "fc_w": fc_w, "fc_b": fc_b, "layers": [(p, None) for p in layers]}
    m = _build_model(g)
    xt = S.to_dev(x).requires_grad_(True)
    loss = m.loss(xt, S.to_dev(y))
    loss.backward()
    torch.cuda.synchronize()
    l64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in layers]
    loss_o, scores_o, h_last_o, dx_o, grads_o, dw_o, db_o = O.stack_forward_backward(
        x.astype(np.float64), l64, fc_w.astype(np.float64), fc_b.astype(np.float64), y)
    assert abs(float(loss) - float(loss_o)) <= 1e-5
    rel = lambda a, ref: float(np.abs(a.detach().cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max()) / max(1e-3, float(np.abs(ref).max()))
    # the loss is a MEAN over 4096 utterances: gradients are ~1e-4 in size, so they are compared relative to their
    # own largest element (floor 1e-3), at the 2e-5 the single layers meet
    assert rel(xt.grad, dx_o) <= 2e-5
    assert rel(m.hidden2keyword.weight.grad, dw_o) <= 2e-5 and rel(m.hidden2keyword.bias.grad, db_o) <= 2e-5
    for rnn, go in zip(m.rnn_list, grads_o):
        for name, par in (("d_w", rnn.W), ("d_u", rnn.U), ("d_bias_gate", rnn.bias_gate), ("d_bias_update", rnn.bias_update),
                          ("d_zeta", rnn.zeta), ("d_nu", rnn.nu)):
            assert rel(par.grad, go[name]) <= 2e-5, (name, rel(par.grad, go[name]))
    with torch.no_grad():
        m.init_hidden()
        scores = m(S.to_dev(x))
    assert (np.abs(scores.cpu().numpy() - scores_o) / np.maximum(1.0, np.abs(scores_o))).max() <= 1e-5


def test_two_layer_model_with_bf16_sequences(stack_golden):
    """BASELINE config 3 ("bf16 with fp32 master grads") for the default stack: bf16 frames in, bf16 hidden-state
    sequences between the layers, fp32 state / parameters / parameter gradients; both layers on the matrix-pipe
    kernels.  Against the same model run in fp32 on the rounded frames: loss to 2e-3, gradients to 2 % of their
    largest element (each layer's hs is rounded once to bf16: 2^-9 relative per element)."""
    g = stack_golden
    T, B, F = g["x"].shape
    for F_l, H_l in ((F, g["hidden"][0]), (g["hidden"][0], g["hidden"][1])):
        for direction in (0, 1):
            assert fastgrnn_cuda.kernel_path(T, B, F_l, H_l, dtype=torch.bfloat16, direction=direction,
                                             flags=_lib.FLAG_SAVE_PREACT) == 2
    m = _build_model(g)
    y = S.to_dev(g["labels"])
    xb = S.to_dev(g["x"].astype(np.float32)).to(torch.bfloat16)
    res = []
    for x in (xb, xb.float()):
        for p_ in m.parameters():
            p_.grad = None
        m.init_hidden()
        xin = x.clone().requires_grad_(True)
        loss = m.loss(xin, y)
        loss.backward()
        assert xin.grad.dtype == x.dtype
        res.append((float(loss), xin.grad.float().clone(), {n: p_.grad.clone() for n, p_ in m.named_parameters()}))
    assert abs(res[0][0] - res[1][0]) <= 2e-3
    rel = lambda a, b: float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))
    assert rel(res[0][1], res[1][1]) <= 2e-2
    for n in res[0][2]:
        assert res[0][2][n].dtype == torch.float32 and rel(res[0][2][n], res[1][2][n]) <= 2e-2, (n, rel(res[0][2][n], res[1][2][n]))


@pytest.mark.parametrize("want_dx", [False, True])
def test_two_layer_model_reads_the_loaders_batch_in_place(stack_golden, want_dx):
    """The trainer feeds `audio.permute(2, 0, 1)` of the loader's [B,F,T] batch (trainClassifier.py:204,299); the
    reference's first layer (H=256) takes it as it is (FASTGRNN_FLAG_X_BFT, a workspace transpose): same loss and gradients, bit for bit, as
    with the contiguous copy the reference makes (rnn.py:910), with and without a gradient on the audio."""
    g = stack_golden
    T, B, F = g["x"].shape
    assert fastgrnn_cuda.kernel_path(T, B, F, g["hidden"][0], direction=1,
                                     flags=_lib.FLAG_SAVE_PREACT | _lib.FLAG_X_BFT) == 2
    m = _build_model(g)
    y = S.to_dev(g["labels"])
    audio = S.to_dev(np.ascontiguousarray(g["x"].astype(np.float32).transpose(1, 2, 0)))       # [B,F,T]
    res = []
    for view in (True, False):
        a = audio.clone().requires_grad_(want_dx)
        xin = a.permute(2, 0, 1) if view else a.permute(2, 0, 1).contiguous()
        for p_ in m.parameters():
            p_.grad = None
        m.init_hidden()
        loss = m.loss(xin, y)
        loss.backward()
        res.append((loss.detach().clone(), a.grad.clone() if want_dx else None,
                    {n: p_.grad.clone() for n, p_ in m.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and abs(float(res[0][0]) - float(g["loss"])) <= 1e-5
    if want_dx:
        assert res[0][1].shape == (B, F, T) and torch.equal(res[0][1], res[1][1])
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n


@pytest.mark.parametrize("F,H", [(32, 256), (256, 128), (64, 128), (64, 256)])
def test_input_gradient_is_optional_where_it_is_a_gemm_of_its_own(F, H):
    """fastgrnn_grads.d_x may be NULL on the H=256 and wide-input shapes (a model's first layer: its input is data):
    the d_x GEMM is skipped, every other gradient is bit-identical; elsewhere a NULL d_x stays an error."""
    T, B = 9, 37
    rng = np.random.default_rng(3)
    p = O.make_params(F, H, dtype=np.float32, seed=37, randomize_scalars=True)
    P = S.cell_tensors(p)
    x = S.to_dev(rng.standard_normal((T, B, F)).astype(np.float32))
    h0 = S.to_dev((0.5 * rng.standard_normal((B, H))).astype(np.float32))
    G = S.to_dev(rng.standard_normal((T, B, H)).astype(np.float32))
    fl = _lib.FLAG_SAVE_PREACT
    outs = S.forward_unroll(x, h0, P, "sigmoid", flags=fl)
    run = lambda need: S.backward_of(outs, G, x, h0, P, "sigmoid", flags=fl, biases=True, need_dx=need)
    full, lean = run(True), run(False)
    assert full[0].shape == x.shape and lean[0].numel() == 0
    for a, b in zip(full[1:8], lean[1:8]):
        assert torch.equal(a, b)
    # through autograd: an input that does not require grad
    m = FastGRNNCUDA(F, H, device=DEV)
    m(x).square().mean().backward()
    g1 = [q.grad.clone() for q in m.parameters()]
    for q in m.parameters():
        q.grad = None
    xr = x.clone().requires_grad_(True)
    m(xr).square().mean().backward()
    assert xr.grad is not None and all(torch.equal(a, q.grad) for a, q in zip(g1, m.parameters()))


@pytest.mark.parametrize("B,preact", [(37, True), (16, False)])
def test_h256_with_column_blocks_of_U_in_different_binades(B, preact):
    """The H=256 backward scales each wave's 32-column block of U by its own power of two: blocks whose largest
    elements sit in different binades (any trained matrix; not the 0.1 * randn of the other tests) must come out
    right too.  (The first build un-scaled with the PRODUCER wave's factor: wrong by powers of two here.)"""
    T, F, H = 9, 32, 256
    rng = np.random.default_rng(11)
    p = O.make_params(F, H, dtype=np.float32, seed=43, randomize_scalars=True)
    blk = np.repeat(np.array([1.0, 0.3, 2.2, 0.55, 0.13, 1.7, 0.9, 0.06], np.float32), 32)
    p["u"] = (p["u"] * blk[None, :] * 0.5).astype(np.float32)        # columns k = 32w .. 32w+31 share a factor
    x = rng.standard_normal((T, B, F)).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((B, H))).astype(np.float32)
    G = rng.standard_normal((T, B, H)).astype(np.float32)
    outs, gr = LC.layer_fwd_bwd(S.to_dev(x), S.to_dev(h0), S.to_dev(G), p, preact=preact)
    hs_o, zs_o, cs_o, g_o = S.oracle64(x, G, p, h0)
    assert np.abs(outs[0].cpu().numpy() - hs_o).max() <= 1e-5
    S.check_grads(gr, g_o, tol=2e-5, scalar_term_tol=0.0, tag=(B, preact))
