"""FastGRNNBatchNorm eval-mode inference on the GPU: the reference's trained keyword spotter against its fp64
evaluation, the full-size batch, random BatchNorm statistics on every kernel-path-2 shape, the generic scan in fp64,
hidden-state carry and the refused backward."""
import pytest
import torch

from kws_amd import FastGRNNBatchNorm, _lib, fastgrnn_cuda
from tests import batchnorm_golden as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A, BM, LAST = _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_HS_LAST


def _trained(batch_first):
    d, full = G.trained_state_dict()
    m = G.build_model(DEV, batch_first=batch_first)
    m.load_state_dict(full, strict=True)
    return d, full, m.eval()


def _layer_states(m):
    return [h.detach().double().cpu() for h in m.hidden_states]


@pytest.mark.parametrize("batch_first", [False, True])
def test_trained_model_against_fp64(batch_first):
    d, full, m = _trained(batch_first)
    x = torch.from_numpy(d["x"]).to(DEV)
    if batch_first:
        x = x.transpose(0, 1).contiguous()
    T, B, F = d["x"].shape
    for l, (f, h) in enumerate(zip([64, 256, 128], G.HIDDEN)):
        fl = A | (BM if batch_first else 0) | (LAST if l == 2 else 0)
        assert fastgrnn_cuda.kernel_path(T, B, f, h, flags=fl) == 2, l
    m.init_hidden()
    logp = m(x).detach().double().cpu()
    for l, h in enumerate(_layer_states(m)):
        err = float((h - torch.from_numpy(d["f64_h%d" % l])).abs().max())
        bound = 2 * float(d["err_h%d" % l]) + 1e-6
        print("layer %d: max|gpu-fp64| %.3g, bound %.3g, ratio %.3f" % (l, err, bound, err / bound))
        assert err <= bound, (l, err, bound)
    ref = torch.from_numpy(d["f64_logp"])
    err = float((logp - ref).abs().max())
    bound = 2 * float(d["err_logp"]) + 1e-6
    print("log-probs: max|gpu-fp64| %.3g, bound %.3g, ratio %.3f" % (err, bound, err / bound))
    assert err <= bound
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(logp.argmax(1)[sure], ref.argmax(1)[sure])


def test_trained_model_full_size():
    d, full, m = _trained(True)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(4096, 99, 64, device=DEV, generator=g)
    m.init_hidden()
    logp = m(x).detach().double()
    sd = {k: v.to(DEV) for k, v in full.items()}
    hT, ref = G.model_oracle(sd, x.transpose(0, 1))
    for l, h in enumerate(m.hidden_states):
        err = float((h.double() - hT[l]).abs().max())
        bound = 10 * float(d["err_h%d" % l]) + 1e-6
        print("full size layer %d: max|gpu-fp64| %.3g, bound %.3g, ratio %.3f" % (l, err, bound, err / bound))
        assert err <= bound, (l, err, bound)
    err = float((logp - ref).abs().max())
    bound = 10 * float(d["err_logp"]) + 1e-6
    print("full size log-probs: max|gpu-fp64| %.3g, bound %.3g, ratio %.3f" % (err, bound, err / bound))
    assert err <= bound
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(logp.argmax(1)[sure], ref.argmax(1)[sure])


SHAPES = [(128, 32), (128, 64), (128, 128), (128, 256), (256, 32), (256, 64), (256, 128)]


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("gate", ["sigmoid", "relu", "tanh"])
def test_stress_path2(H, F, gate):
    m = G.random_bn(F, H, gate, seed=H + F + len(gate))
    worst = 0.0
    for B in (17, 4097):
        T = 12 if (B > 1000 or gate == "relu") else 30
        g = torch.Generator(device=DEV).manual_seed(B)
        x = torch.randn(T, B, F, device=DEV, generator=g)
        h0 = 0.5 * torch.randn(B, H, device=DEV, generator=g)
        ref = G.fp64_scan(m, x, h0)
        assert bool(torch.isfinite(ref).all())
        e32 = float((G.fp32_scan(m, x, h0).double() - ref).abs().max())
        bound = 4 * e32 + 1e-5 * max(1.0, float(ref.abs().max()))
        for bf in (False, True):
            m.batch_first = bf
            xi = x.transpose(0, 1).contiguous() if bf else x
            assert fastgrnn_cuda.kernel_path(T, B, F, H, gate_nl=_lib.NONLINEARITY[gate], flags=A | (BM if bf else 0)) == 2
            with torch.no_grad():
                hs = m(xi, h0, training=False)
                last = m(xi, h0, training=False, last_state=True)
            hs_tm = hs.transpose(0, 1) if bf else hs
            err = float((hs_tm.double() - ref).abs().max())
            worst = max(worst, err / bound)
            assert err <= bound, (B, bf, err, bound, e32)
            assert torch.allclose(last, hs_tm[-1], rtol=0, atol=1e-6 * max(1.0, float(hs_tm[-1].abs().max()))), (B, bf)
    m.batch_first = False
    print("stress H=%d F=%d %s: worst error / bound %.3f" % (H, F, gate, worst))


def test_generic_fp64_h100():
    d, sd = G.load("random_h100_f64")
    m = FastGRNNBatchNorm(24, 100, device=DEV).double().eval()
    m.cell.load_state_dict(sd, strict=True)
    assert fastgrnn_cuda.kernel_path(20, 5, 24, 100, dtype=torch.float64, flags=A) == 0
    with torch.no_grad():
        hs = m(torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["h0"]).to(DEV), training=False)
    assert float((hs.cpu() - torch.from_numpy(d["hs"])).abs().max()) <= 1e-12


def test_hidden_state_carry():
    d, full, m = _trained(True)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(33, 70, 64, device=DEV, generator=g)
    m.init_hidden()
    whole = m(x).detach()
    states = [h.clone() for h in m.hidden_states]
    m.init_hidden()
    m(x[:, :40].contiguous())
    parts = m(x[:, 40:].contiguous()).detach()
    # (equal to fp32 rounding: the frame GEMMs of the wide layers tile T*B rows differently for the shorter calls)
    assert float((parts - whole).abs().max()) <= 1e-5
    for l, (a, b) in enumerate(zip(states, m.hidden_states)):
        diff = float((a - b).abs().max())
        print("carry layer %d: max|two calls - one call| %.3g (max|h| %.3g)" % (l, diff, float(a.abs().max())))
        assert diff <= 2e-5 * max(1.0, float(a.abs().max())), l


def test_backward_raises():
    d, full, m = _trained(False)
    x = torch.randn(10, 4, 64, device=DEV)
    m.init_hidden()
    out = m(x)
    assert out.requires_grad
    with pytest.raises(NotImplementedError, match="no backward"):
        out.sum().backward()
