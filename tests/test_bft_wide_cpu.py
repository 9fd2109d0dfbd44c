"""FASTGRNN_FLAG_X_BFT on the layers whose frame product is a GEMM of its own (dense H=256 with F=64/128, dense H=128
with F=64/128/256): the path table, the workspace sizes and the argument checks, all host-side (no kernel is launched).

The forward reads the loader's [B,F,T] frames in place (no workspace copy: the forward's bytes do not change with the
flag); the backward takes one time-major copy of x for the weight-gradient GEMM (align256(T*B*F*4) more)."""
import ctypes as C

import pytest
import torch

from kws_amd import _lib, fastgrnn_cuda

X, SP, LAST, GL, BM = _lib.FLAG_X_BFT, _lib.FLAG_SAVE_PREACT, _lib.FLAG_HS_LAST, _lib.FLAG_GRAD_LAST, _lib.FLAG_BATCH_MAJOR
A, BN = _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BN_TRAIN
SHAPES = [(256, 64), (256, 128), (128, 64), (128, 128), (128, 256)]          # (H, F)
T, B = 99, 4096


def _align256(n):
    return (n + 255) // 256 * 256


def _desc(F, H, flags, T=T, B=B, gate=0, dtype=_lib.F32, w_rank=0, u_rank=0):
    return _lib.Desc(T, B, F, H, w_rank, u_rank, gate, 2, dtype, flags)


@pytest.mark.parametrize("H,F", SHAPES)
def test_kernel_path_table(H, F):
    kp = lambda **k: fastgrnn_cuda.kernel_path(T, B, F, H, **k)
    for gate in (0, 1, 2):
        for fl in (X, X | SP, X | LAST, X | BM):
            assert kp(gate_nl=gate, flags=fl) == 2, (gate, fl)
        for fl in (X | SP, X | SP | GL):
            assert kp(gate_nl=gate, flags=fl, direction=1) == 2, (gate, fl)
        for fl in (A | X, A | X | BM, A | X | LAST):
            assert kp(gate_nl=gate, flags=fl) == 2, (gate, fl)
            assert kp(gate_nl=gate, flags=fl, direction=1) == -1, (gate, fl)
    # quantised gates: the forward, and the backward under the one-saved-tensor contract, as without the flag
    for gate in (3, 4, 5):
        assert kp(gate_nl=gate, flags=X) == 2 and kp(gate_nl=gate, flags=X | SP, direction=1) == 2
        assert kp(gate_nl=gate, flags=X, direction=1) != 2
    # the backward with both layout flags stays off path 2 (its time-major copy of x would not match [B,T] rows)
    assert kp(flags=X | SP | BM, direction=1) != 2
    assert kp(flags=X | SP | LAST) != 2                       # HS_LAST saves nothing, with the flag as without


@pytest.mark.parametrize("H,F", SHAPES)
def test_still_unsupported_beside_the_flag(H, F):
    kp = lambda **k: fastgrnn_cuda.kernel_path(T, B, F, H, **k)
    for fl in (X, X | SP, X | LAST, X | BM):                  # bf16 sequences
        assert kp(dtype=torch.bfloat16, flags=fl) != 2, fl
    assert kp(dtype=torch.bfloat16, flags=X | SP, direction=1) != 2
    lib = _lib.load()
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(_desc(F, H, BN | X))) == 0
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(_desc(32, 128, BN | X))) == 0


def test_affine_with_the_flag_stays_refused_on_32_feature_cells():
    lib = _lib.load()
    fake = C.c_void_p(0x10000)                                # never dereferenced: refused before a launch
    prm = _lib.Params(fake, fake, None, None, None, None, fake, fake, fake, fake)
    for H in (128, 256):
        d = _desc(32, H, A | X, T=10, B=4)
        assert lib.fastgrnn_hip_forward_unroll_affine(C.byref(d), C.byref(prm), fake, fake, fake, fake, fake, None, 0,
                                                      None) == 7
        assert fastgrnn_cuda.kernel_path(10, 4, 32, H, flags=A | X) != 2


@pytest.mark.parametrize("H,F", SHAPES)
def test_workspace_sizes(H, F):
    lib = _lib.load()
    fw, bw = lib.fastgrnn_hip_forward_workspace_bytes, lib.fastgrnn_hip_backward_workspace_bytes
    for t, b in ((T, B), (23, 37), (1, 5)):
        for fl in (0, SP, LAST, BM):
            assert fw(C.byref(_desc(F, H, fl | X, T=t, B=b))) == fw(C.byref(_desc(F, H, fl, T=t, B=b))), (t, b, fl)
        assert fw(C.byref(_desc(F, H, A | X, T=t, B=b))) == fw(C.byref(_desc(F, H, A, T=t, B=b)))
        for fl in (SP, SP | GL):
            with_flag, without = bw(C.byref(_desc(F, H, fl | X, T=t, B=b))), bw(C.byref(_desc(F, H, fl, T=t, B=b)))
            assert with_flag == without + _align256(t * b * F * 4), (t, b, fl)
    # factorised cells multiplied out onto these shapes inherit the flag, their layouts the backward's copy of x
    for w_rank, u_rank in ((8, 0), (0, 8), (40, 40)):
        kw = dict(w_rank=w_rank, u_rank=u_rank)
        assert fastgrnn_cuda.kernel_path(T, B, F, H, w_rank, u_rank, flags=X | SP) == 2
        assert fastgrnn_cuda.kernel_path(T, B, F, H, w_rank, u_rank, direction=1, flags=X | SP) == 2
        assert fw(C.byref(_desc(F, H, SP | X, **kw))) == fw(C.byref(_desc(F, H, SP, **kw)))
        assert bw(C.byref(_desc(F, H, SP | X, **kw))) == bw(C.byref(_desc(F, H, SP, **kw))) + _align256(T * B * F * 4)


@pytest.mark.parametrize("H,F", SHAPES)
def test_missing_workspace_is_refused_before_any_launch(H, F):
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)
    pf = _lib.Params(*([one] * 10))
    d = _desc(F, H, X, T=3, B=4)
    assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(pf), one, one, one, null, null, null, 0, null) == 5
    d = _desc(F, H, A | X, T=3, B=4)
    assert lib.fastgrnn_hip_forward_unroll_affine(C.byref(d), C.byref(pf), one, one, one, one, one, null, 0, null) == 5
    g = _lib.Grads(*([one] * 12))
    gx = _lib.Grads(*([null] + [one] * 11))                   # d_x == NULL: a first layer
    d = _desc(F, H, X | SP, T=3, B=4)
    for grads in (g, gx):
        assert lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(pf), one, one, one, one, one, one, C.byref(grads),
                                                null, 0, null) == 5


def test_flag_does_not_combine_with_zero_extension():
    """A view on a zero-extended shape keeps the copy: the flag's answer does not depend on FLAG_ZERO_EXTEND."""
    ZE = _lib.FLAG_ZERO_EXTEND
    for F, H in ((64, 200), (64, 100), (100, 256)):
        for direction in (0, 1):
            a = fastgrnn_cuda.kernel_path(T, B, F, H, direction=direction, flags=X | SP)
            assert a == fastgrnn_cuda.kernel_path(T, B, F, H, direction=direction, flags=X | SP | ZE) and a != 2
