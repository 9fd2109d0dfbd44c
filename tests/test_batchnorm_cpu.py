"""FastGRNNBatchNorm without a GPU: the reference checkpoint's key set, the fold against the unfolded BatchNorm
formula in fp64, the argument checks of the module and of fastgrnn_hip_forward_unroll_affine."""
import ctypes as C

import numpy as np
import pytest
import torch

from kws_amd import FastGRNNBatchNorm, RNNClassifierModel, _lib, fastgrnn_cuda, fold_batchnorm
from tests import batchnorm_golden as G


def test_trained_state_dict_loads_strictly():
    d, full = G.trained_state_dict()
    m = G.build_model("cpu")
    mine = m.state_dict()
    assert list(mine.keys()) == [str(k) for k in d["keys"]]
    for k, v in full.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    m.load_state_dict(full, strict=True)
    assert torch.equal(m.rnn_list[2].unrollRNN.RNNCell.bn_u.running_var, full["rnn_list.2.cell.bn_u.running_var"])


def test_unfolded_oracle_matches_golden_fp64():
    d, full = G.trained_state_dict()
    hT, logp = G.model_oracle(full, d["x"])
    for l in range(3):
        assert np.abs(hT[l].numpy() - d["f64_h%d" % l]).max() <= 1e-12, l
    assert np.abs(logp.numpy() - d["f64_logp"]).max() <= 1e-12


def test_fold_with_fp64_scan_matches_golden():
    d, full = G.trained_state_dict()
    m = G.build_model("cpu")
    m.load_state_dict(full, strict=True)
    m.double().eval()
    rin = torch.from_numpy(d["x"]).double()
    for l, H in enumerate(G.HIDDEN):
        cell = m.rnn_list[l].cell
        w, u, bg, bu, sg, sc = fold_batchnorm(cell)
        assert w.shape == (H, rin.shape[-1]) and u.shape == (H, H)
        hs = G.folded_scan(w, u, bg, bu, sg, sc, cell.zeta.reshape(()), cell.nu.reshape(()), rin,
                           torch.zeros(rin.shape[1], H, dtype=torch.float64))
        assert np.abs(hs[-1].numpy() - d["f64_h%d" % l]).max() <= 1e-12, l
        rin = hs


def test_fold_random_h100_fp64():
    d, sd = G.load("random_h100_f64")
    m = FastGRNNBatchNorm(24, 100, device="cpu").double()
    m.cell.load_state_dict(sd, strict=True)
    w, u, bg, bu, sg, sc = fold_batchnorm(m.cell)
    hs = G.folded_scan(w, u, bg, bu, sg, sc, m.cell.zeta.reshape(()), m.cell.nu.reshape(()),
                       torch.from_numpy(d["x"]), torch.from_numpy(d["h0"]))
    assert np.abs(hs.numpy() - d["hs"]).max() <= 1e-12
    hs_u = G.unfolded_scan({k: v.double() for k, v in sd.items()}, torch.from_numpy(d["x"]), torch.from_numpy(d["h0"]))
    assert np.abs(hs_u.numpy() - d["hs"]).max() <= 1e-12


def test_fold_cache_follows_in_place_updates():
    m = FastGRNNBatchNorm(8, 16, device="cpu")
    a = m.cell._folded()
    assert m.cell._folded() is a
    with torch.no_grad():
        m.cell.bn_gate.running_var.mul_(4.0)
    b = m.cell._folded()
    assert b is not a and torch.allclose(b[4], a[4] / 2.0)


def test_module_errors():
    with pytest.raises(ValueError):
        FastGRNNBatchNorm(32, 64, wRank=8, device="cpu")
    with pytest.raises(ValueError):
        FastGRNNBatchNorm(32, 64, uRank=8, device="cpu")
    with pytest.raises(ValueError):
        RNNClassifierModel("FastGRNNBatchNorm", 32, 1, [64], [8], [None], [1.0], [1.0], "sigmoid", "tanh",
                           num_classes=4, device="cpu")
    m = FastGRNNBatchNorm(8, 16, device="cpu")
    with pytest.raises(NotImplementedError, match="grid-wide"):
        m(torch.zeros(3, 2, 8))                                   # training=True is the reference default
    model = RNNClassifierModel("FastGRNNBatchNorm", 8, 1, [16], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=4, device="cpu")
    with pytest.raises(NotImplementedError):
        model(torch.zeros(3, 2, 8))                               # a fresh model is in training mode
    model.eval()
    assert not model.rnn_list[0].training and not model.rnn_list[0].cell.bn_w.training
    model.train()
    assert model.rnn_list[0].training
    with pytest.raises(NotImplementedError):
        model.loss(torch.zeros(3, 2, 8), torch.zeros(2, dtype=torch.long))


def _desc(T, B, F, H, gate=0, update=2, dtype=_lib.F32, flags=_lib.FLAG_PREACT_AFFINE):
    return _lib.Desc(T, B, F, H, 0, 0, gate, update, dtype, flags)


def test_library_argument_checks():
    lib = _lib.load()
    fake = C.c_void_p(0x10000)                 # never dereferenced: every call below is refused before a launch
    prm = _lib.Params(fake, fake, None, None, None, None, fake, fake, fake, fake)
    d = _desc(10, 4, 32, 128)
    call = lib.fastgrnn_hip_forward_unroll_affine
    assert call(C.byref(d), C.byref(prm), None, fake, fake, fake, fake, None, 0, None) == 1      # ERR_NULL_POINTER
    assert call(C.byref(d), C.byref(prm), fake, None, fake, fake, fake, None, 0, None) == 1
    db = _desc(10, 4, 32, 128, dtype=_lib.BF16_IO)
    assert call(C.byref(db), C.byref(prm), fake, fake, fake, fake, fake, None, 0, None) == 7      # UNSUPPORTED
    for fl in (_lib.FLAG_X_BFT, _lib.FLAG_SAVE_PREACT):
        dx = _desc(10, 4, 32, 128, flags=_lib.FLAG_PREACT_AFFINE | fl)
        assert call(C.byref(dx), C.byref(prm), fake, fake, fake, fake, fake, None, 0, None) == 7
    dn = _desc(10, 4, 32, 128, flags=0)                                                          # flag missing
    assert call(C.byref(dn), C.byref(prm), fake, fake, fake, fake, fake, None, 0, None) == 7
    # batch-major / last-state off kernel path 2
    dbm = _desc(10, 4, 32, 100, flags=_lib.FLAG_PREACT_AFFINE | _lib.FLAG_BATCH_MAJOR)
    assert call(C.byref(dbm), C.byref(prm), fake, fake, fake, fake, fake, None, 0, None) == 7
    # the new flag on the existing entry points
    assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(prm), fake, fake, fake, None, None, None, 0,
                                           None) == 7
    assert lib.fastgrnn_hip_forward(C.byref(_desc(1, 4, 32, 128)), C.byref(prm), fake, fake, fake, None, None,
                                    None, 0, None) == 7
    g = _lib.Grads(*([fake] * 12))
    assert lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(prm), fake, fake, fake, fake, fake, fake,
                                            C.byref(g), None, 0, None) == 7


PATH2 = [(128, 32), (128, 64), (128, 128), (128, 256), (256, 32), (256, 64), (256, 128)]


@pytest.mark.parametrize("H,F", PATH2)
def test_kernel_path_table(H, F):
    A, BM, LAST = _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_HS_LAST
    kp = lambda **k: fastgrnn_cuda.kernel_path(99, 4096, F, H, **k)
    for gate in (0, 1, 2):
        for fl in (A, A | BM, A | LAST, A | BM | LAST):
            assert kp(gate_nl=gate, flags=fl) == 2, (gate, fl)
    assert kp(gate_nl=3, flags=A) == 0                         # quantised codes: generic scan
    assert kp(gate_nl=0, update_nl=3, flags=A) == 0
    assert kp(dtype=torch.float64, flags=A) == 0
    assert kp(flags=A | _lib.FLAG_FORCE_GENERIC) == 0
    assert kp(flags=A, direction=1) == -1                       # no backward
    lib = _lib.load()
    d = _desc(99, 4096, F, H)
    assert lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)) == 0


def test_kernel_path_other_shapes():
    A = _lib.FLAG_PREACT_AFFINE
    for F, H in ((32, 100), (64, 64), (32, 512), (48, 128)):
        assert fastgrnn_cuda.kernel_path(99, 64, F, H, flags=A) == 0, (F, H)
    lib = _lib.load()
    # path 0 packs biases and scales into its workspace: 4 H more than the plain generic forward
    d0 = _desc(5, 3, 24, 100, dtype=_lib.F64, flags=A)
    d1 = _desc(5, 3, 24, 100, dtype=_lib.F64, flags=0)
    assert lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d0)) == \
        lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d1)) + (4 * 100 * 8 + 255) // 256 * 256
