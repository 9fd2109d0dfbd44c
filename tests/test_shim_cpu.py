"""The shared pieces of the Python operator shim (kws_amd/fastgrnn_cuda.py) without a GPU: the output-shape rule, the
flat parameter-gradient buffer, the per-family cache of the library's answers against direct calls of the C queries, and
the two device checks of forward / backward on stand-in operands."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from kws_amd import _lib, batchnorm_train, fastgrnn_cuda as fc

BM = _lib.FLAG_BATCH_MAJOR
T, B, R = 7, 37, 61
SHAPES = [(128, 32), (256, 32), (256, 64)]                 # (H, F)
CUDA0, CUDA1 = torch.device("cuda:0"), torch.device("cuda:1")


def test_seq_shape_table():
    assert fc._seq_shape(3, 5, 7, False, False) == (3, 5, 7)
    assert fc._seq_shape(3, 5, 7, True, False) == (5, 3, 7)
    assert fc._seq_shape(3, 5, 7, False, True) == (5, 7)
    assert fc._seq_shape(3, 5, 7, True, True) == (5, 7)


@pytest.mark.parametrize("rw,ru", [(0, 0), (2, 1), (2, 0), (0, 1)], ids=["dense", "lowrank", "w_lowrank", "u_lowrank"])
def test_flat_gradient_buffer(rw, ru):
    H, F = 4, 3
    shapes = ([(rw, F), (H, rw)] if rw else [(H, F)]) + ([(ru, H), (H, ru)] if ru else [(H, H)]) + \
        [(1, H), (1, H), (1, 1), (1, 1)]
    sizes = [a * b for a, b in shapes]
    views, slots = fc._flat_grads(bool(rw), bool(ru), shapes, sizes, torch.float64, torch.device("cpu"))
    assert [tuple(v.shape) for v in views] == shapes
    assert all(v.dtype == torch.float64 and v.is_contiguous() for v in views)
    base = views[0].untyped_storage().data_ptr()
    assert all(v.untyped_storage().data_ptr() == base for v in views)           # one allocation
    assert views[0].untyped_storage().nbytes() == 8 * sum(sizes)                # and nothing else in it
    assert [v.storage_offset() for v in views] == [sum(sizes[:i]) for i in range(len(sizes))]   # registration order
    d_w, d_u, d_w1, d_w2, d_u1, d_u2 = slots
    nw = 2 if rw else 1
    want_w = (None, views[0], views[1]) if rw else (views[0], None, None)
    want_u = (None, views[nw], views[nw + 1]) if ru else (views[nw], None, None)
    for got, want in zip((d_w, d_w1, d_w2, d_u, d_u1, d_u2), want_w + want_u):
        if want is None:
            assert got is fc._NONE and got.numel() == 0
        else:
            assert got is want
    assert len(views) == nw + (2 if ru else 1) + 4


def _key(H, F, flags, B=B, dtype=_lib.F32):
    return (T, B, F, H, 0, 0, 0, 2, dtype, flags)


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("flags", [0, BM], ids=["time_major", "batch_major"])
def test_pool_plan_equals_the_library_on_supported_shapes(H, F, flags):
    lib = _lib.load()
    d = _lib.Desc(*_key(H, F, flags))
    w = fc._pool_plan(_key(H, F, flags), "windows", R)
    assert lib.fastgrnn_hip_windows_supported(C.byref(d)) == 1 and w.supported is True
    assert w.ws_forward == lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R) and w.ws_backward == 0
    t = fc._pool_plan(_key(H, F, flags), "train_windows", R)
    assert lib.fastgrnn_hip_train_windows_supported(C.byref(d)) == 1 and t.supported is True
    assert t.ws_forward == lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(d), R)
    assert t.ws_backward == lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), R) > 0
    for p in (w, t):
        assert [getattr(p.desc, n) for n, _ in _lib.Desc._fields_] == list(_key(H, F, flags))
    assert fc.windows_supported(T, B, F, H, flags=flags) and fc.train_windows_supported(T, B, F, H, flags=flags)


@pytest.mark.parametrize("family", ["windows", "train_windows"])
def test_pool_plan_of_unsupported_shapes_is_all_zero(family):
    for key in (_key(128, 64, 0), _key(128, 32, 0, dtype=_lib.F64)):
        p = fc._pool_plan(key, family, R)
        assert (p.supported, p.ws_forward, p.ws_backward) == (False, 0, 0)
    assert not fc.windows_supported(T, B, 64, 128) and not fc.train_windows_supported(T, B, 64, 128)
    assert not fc.windows_supported(T, B, 32, 128, dtype=torch.float64)
    assert fc.windows_supported(T, B, 32, 128, dtype=torch.float16) is False    # outside _DTYPES: no query at all
    assert fc.train_windows_supported(T, B, 32, 128, dtype=torch.float16) is False


@pytest.mark.parametrize("H,F", [(128, 32), (256, 64)])
@pytest.mark.parametrize("batch_major", [False, True])
def test_pool_plan_of_batchnorm_training(H, F, batch_major):
    lib = _lib.load()
    flags = _lib.FLAG_BN_TRAIN | (BM if batch_major else 0)
    d = _lib.Desc(*_key(H, F, flags, B=2))
    p = batchnorm_train._plan(T, 2, F, H, 0, batch_major)
    assert p is fc._pool_plan(_key(H, F, flags, B=2), "bn_train")               # the shared cache, one entry
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(d)) == 1 and p.supported is True
    assert p.ws_forward == lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(d)) > 0
    assert p.ws_backward == lib.fastgrnn_hip_bn_train_backward_workspace_bytes(C.byref(d)) > 0
    assert batchnorm_train.bn_train_supported(T, 2, F, H, batch_major=batch_major) is True
    one = batchnorm_train._plan(T, 1, F, H, 0, batch_major)
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(_lib.Desc(*_key(H, F, flags, B=1)))) == 0
    assert (one.supported, one.ws_forward, one.ws_backward) == (False, 0, 0)
    assert batchnorm_train.bn_train_supported(T, 1, F, H, batch_major=batch_major) is False
    assert batchnorm_train.bn_train_supported(T, 2, F, H, dtype=torch.float64) is False


def _operand(device=CUDA0, numel=6, contiguous=True):
    """What the device checks look at, without a GPU."""
    return SimpleNamespace(device=device, numel=lambda: numel, is_contiguous=lambda: contiguous)


def test_fast_path_predicate():
    a, b = _operand(), _operand()
    assert fc._all_dense_on(CUDA0, a, b, _operand()) is True
    assert fc._all_dense_on(CUDA0, a, _operand(device=CUDA1), b) is False
    assert fc._all_dense_on(CUDA0, a, _operand(device=CUDA1, numel=0), b) is True     # (an operand that does not apply)
    assert fc._all_dense_on(CUDA0, a, _operand(contiguous=False), b) is False
    assert fc._all_dense_on(CUDA0, a, _operand(device=torch.device("cpu")), b) is False
    assert fc._all_dense_on(CUDA1, a) is False


def test_slow_path_device_check():
    ok = [(_operand(), "w"), (None, "w1"), (_operand(device=CUDA1, numel=0), "u1"), (_operand(), "nu")]
    fc._check_devices(CUDA0, ok)
    with pytest.raises(RuntimeError) as e:
        fc._check_devices(CUDA0, ok + [(_operand(device=CUDA1), "zeta")])
    assert "zeta" in str(e.value) and "cuda:1" in str(e.value) and "cuda:0" in str(e.value)
    meta = [(_operand(device=torch.device("meta")), "h_prime")]
    fc._check_devices(CUDA0, meta, meta_ok=True)                # FLAG_SAVE_PREACT's unused operand may be a meta tensor
    with pytest.raises(RuntimeError, match="h_prime"):
        fc._check_devices(CUDA0, meta)
