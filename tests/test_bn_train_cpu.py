"""FastGRNNBatchNormCUDA without a GPU: the torch-op training formula against the reference's own fixture, strict
loading of the reference checkpoint, the C entry points' argument checks (no launch), the old entry points'
refusal of FASTGRNN_FLAG_BN_TRAIN, the supported-shape table, and the static scans of the new kernel source."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import FastGRNNBatchNorm, FastGRNNBatchNormCUDA, RNNClassifierModel, _lib
from tests import batchnorm_golden as BG
from tests import bn_train_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_bn_train.hip")


@pytest.mark.parametrize("case", G.CASES)
def test_torch_op_formula_matches_reference_fixture(case):
    d = G.load_case(case)
    m = G.build_layer(d, "cpu")
    x, h0, Gt = (torch.from_numpy(d[k]) for k in ("x", "h0", "G"))
    hs, dx, dh0, grads, run = G.step(m, x, h0, Gt, torch_ops=True)
    ehs, edx, edh0, eg, er = G.fixture_expect(d)
    assert np.abs(hs.numpy() - ehs).max() <= 1e-12
    assert np.abs(dx.numpy() - edx).max() <= 1e-12 * max(1.0, np.abs(edx).max())
    assert np.abs(dh0.numpy() - edh0).max() <= 1e-12 * max(1.0, np.abs(edh0).max())
    for k, v in eg.items():
        assert np.abs(grads[k].numpy().reshape(v.shape) - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), k
    for k, v in er.items():
        assert np.abs(run[k].numpy() - v).max() <= 1e-12, k


def test_zero_gradients_are_zero_up_to_rounding():
    d = G.load_case("h128_in32")
    eg = G.fixture_expect(d)[3]
    for k in G.ZERO_GRADS:
        assert np.abs(eg[k]).max() <= 1e-9, k


def test_is_a_fastgrnn_batchnorm_with_the_same_keys():
    a = FastGRNNBatchNormCUDA(64, 256, device="cpu")
    b = FastGRNNBatchNorm(64, 256, device="cpu")
    assert isinstance(a, FastGRNNBatchNorm)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    b.load_state_dict(a.state_dict(), strict=True)


def test_reference_checkpoint_loads_strictly_into_the_training_model():
    d, full = BG.trained_state_dict()
    m = RNNClassifierModel("FastGRNNBatchNormCUDA", 64, 3, BG.HIDDEN, [None] * 3, [None] * 3, [1.0] * 3, [1.0] * 3,
                           "sigmoid", "tanh", num_classes=BG.CLASSES, device="cpu")
    assert all(isinstance(r, FastGRNNBatchNormCUDA) for r in m.rnn_list)
    assert list(m.state_dict().keys()) == [str(k) for k in d["keys"]]
    m.load_state_dict(full, strict=True)
    assert torch.equal(m.rnn_list[0].cell.bn_gate.running_mean, full["rnn_list.0.cell.bn_gate.running_mean"])
    m.eval()
    assert not any(r.training for r in m.rnn_list)
    m.train()
    assert all(r.cell.bn_u.training for r in m.rnn_list)


def test_model_name_is_new():
    with pytest.raises(ValueError):
        RNNClassifierModel("FastGRNNBatchNormCUDAx", 64, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                           num_classes=3, device="cpu")


# ---- C ABI (no launch: every call below fails validation first, or is a pure query) --------------------------------
def _desc(T=4, B=8, F=32, H=128, gate=0, update=2, dtype=_lib.F32, flags=_lib.FLAG_BN_TRAIN, wr=0, ur=0):
    return _lib.Desc(T, B, F, H, wr, ur, gate, update, dtype, flags)


def _fake(n=8):
    return [C.c_void_p(0x10000 + 0x1000 * i) for i in range(n)]


def _bn(null=None):
    a = _fake(5)
    layers = []
    for q in range(4):
        layers.append(_lib.BnLayer(a[0], a[1], a[2], a[3], a[4], 1e-5, 0.1))
    p = _lib.BnParams(*layers)
    if null:
        setattr(getattr(p, null[0]), null[1], None)
    return p


def _params(null=None, factored=False):
    v = _fake(10)
    p = _lib.Params(v[0], v[1], *(v[2:6] if factored else (None,) * 4), v[6], v[7], v[8], v[9])
    if null:
        setattr(p, null, None)
    return p


def _fwd(desc, params=None, bn=None, ptrs=None, ws=None, nbytes=0):
    lib = _lib.load()
    x, h0, hs, sv, st = ptrs if ptrs is not None else _fake(5)
    return lib.fastgrnn_hip_bn_train_forward(C.byref(desc), C.byref(params or _params()), C.byref(bn or _bn()),
                                             x, h0, hs, sv, st, ws, nbytes, None)


def _bwd(desc, params=None, bn=None, g=None, bg=None):
    lib = _lib.load()
    v = _fake(7)
    g = g or _lib.Grads(*_fake(12))
    bg = bg or _lib.BnGrads(*_fake(8))
    return lib.fastgrnn_hip_bn_train_backward(C.byref(desc), C.byref(params or _params()), C.byref(bn or _bn()),
                                              v[0], v[1], v[2], v[3], v[4], v[5], C.byref(g), C.byref(bg), None, 0,
                                              None)


def test_entry_points_validate_without_launching():
    ok = _desc()
    # nothing valid reaches the launch: a NULL workspace for a nonzero requirement fails last
    assert _fwd(ok) == 5 and _bwd(ok) == 5
    assert _fwd(ok, params=_params("w")) == 1 and _bwd(ok, params=_params("u")) == 1
    assert _fwd(ok, params=_params("zeta")) == 1
    assert _fwd(ok, bn=_bn(("gate", "gamma"))) == 1 and _bwd(ok, bn=_bn(("update", "beta"))) == 1
    assert _fwd(ok, bn=_bn(("u", "running_var"))) == 1
    assert _fwd(ok, ptrs=[None] + _fake(4)) == 1 and _fwd(ok, ptrs=_fake(4) + [None]) == 1
    # momentum=None needs num_batches_tracked in the forward
    bn = _bn(("w", "num_batches_tracked"))
    assert _fwd(ok, bn=bn) == 5
    bn.w.momentum = -1.0
    assert _fwd(ok, bn=bn) == 1
    g = _lib.Grads(*_fake(12))
    g.d_u = None
    assert _bwd(ok, g=g) == 1
    bg = _lib.BnGrads(*_fake(8))
    bg.d_beta_gate = None
    assert _bwd(ok, bg=bg) == 1
    g = _lib.Grads(*_fake(12))
    g.d_x = None                                  # the input's gradient is optional
    assert _bwd(ok, g=g) == 5
    # bf16 sequences, fp64, factorised operands, B = 1, the flag missing, other flags
    assert _fwd(_desc(dtype=_lib.BF16_IO)) == 7 and _bwd(_desc(dtype=_lib.BF16_IO)) == 7
    assert _fwd(_desc(dtype=_lib.F64)) == 7
    assert _fwd(_desc(wr=8), params=_params(factored=True)) == 7
    assert _bwd(_desc(ur=8), params=_params(factored=True)) == 7
    assert _fwd(_desc(B=1)) == 2 and _bwd(_desc(B=1)) == 2
    assert _fwd(_desc(flags=0)) == 7 and _bwd(_desc(flags=_lib.FLAG_BATCH_MAJOR)) == 7
    assert _fwd(_desc(flags=_lib.FLAG_BN_TRAIN | _lib.FLAG_HS_LAST)) == 7
    assert _fwd(_desc(gate=3)) == 7 and _fwd(_desc(update=0)) == 7
    assert _fwd(_desc(H=100)) == 7


def test_old_entry_points_refuse_the_flag():
    lib = _lib.load()
    for flags in (_lib.FLAG_BN_TRAIN, _lib.FLAG_BN_TRAIN | _lib.FLAG_PREACT_AFFINE):
        d = _desc(flags=flags)
        v = _fake(8)
        assert lib.fastgrnn_hip_kernel_path(C.byref(d), 0) == -1
        assert lib.fastgrnn_hip_kernel_path(C.byref(d), 1) == -1
        assert lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)) == 0
        assert lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)) == 0
        p = _params()
        assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(p), v[0], v[1], v[2], v[3], v[4], v[5], 1 << 30,
                                               None) == 7
        assert lib.fastgrnn_hip_forward_unroll_affine(C.byref(d), C.byref(p), v[0], v[1], v[2], v[3], v[4], v[5],
                                                      1 << 30, None) == 7
        g = _lib.Grads(*_fake(12))
        assert lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(p), v[0], v[1], v[2], v[3], v[4], v[5],
                                                C.byref(g), v[6], 1 << 30, None) == 7
        d1 = _desc(T=1, flags=flags)
        assert lib.fastgrnn_hip_forward(C.byref(d1), C.byref(p), v[0], v[1], v[2], v[3], v[4], v[5], 1 << 30,
                                        None) == 7
        assert lib.fastgrnn_hip_backward(C.byref(d1), C.byref(p), v[0], v[1], v[2], v[3], v[4], C.byref(g), v[5],
                                         1 << 30, None) == 7


TABLE = [(128, 32), (128, 64), (128, 128), (128, 256), (256, 32), (256, 64), (256, 128)]


@pytest.mark.parametrize("H,F", TABLE)
def test_supported_shape_table(H, F):
    lib = _lib.load()
    for gate in (0, 1, 2):
        for flags in (_lib.FLAG_BN_TRAIN, _lib.FLAG_BN_TRAIN | _lib.FLAG_BATCH_MAJOR):
            for T, B in ((1, 2), (99, 4096), (12, 17)):
                d = _desc(T=T, B=B, F=F, H=H, gate=gate, flags=flags)
                assert lib.fastgrnn_hip_bn_train_supported(C.byref(d)) == 1
                assert lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(d)) > 0
                assert lib.fastgrnn_hip_bn_train_backward_workspace_bytes(C.byref(d)) > 0
    for bad in (_desc(F=F, H=H, B=1), _desc(F=F, H=H, gate=3), _desc(F=F, H=H, dtype=_lib.F64),
                _desc(F=F, H=H, flags=0), _desc(F=F, H=H, flags=_lib.FLAG_BN_TRAIN | _lib.FLAG_X_BFT)):
        assert lib.fastgrnn_hip_bn_train_supported(C.byref(bad)) == 0
        assert lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(bad)) == 0


def test_shapes_off_the_table():
    lib = _lib.load()
    for H, F in ((256, 256), (100, 24), (128, 48), (64, 32)):
        assert lib.fastgrnn_hip_bn_train_supported(C.byref(_desc(F=F, H=H))) == 0


# ---- static scans of the new kernel source (the existing scanner tests list their sources by name) ----------------
@pytest.fixture(scope="module")
def bn_train_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_bn_train.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC))
    return out


def test_war_scan_clean(bn_train_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), bn_train_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) >= 2 and parts[0].startswith("_Z") and parts[1].isdigit():
            assert int(parts[1]) == 0, line


def test_lds_branch_scan_strict_clean(bn_train_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), bn_train_asm,
                        "--strict"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
