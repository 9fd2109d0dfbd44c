"""fastgrnn_hip_forward_windows without a GPU: the three symbols, which descriptors the windowed scans hold, the
argument errors (every call below is refused before a launch), the workspace answer, and the Python side's checks that
need no device."""
import ctypes as C

import pytest
import torch

from kws_amd import RNNClassifierModel, _lib, fastgrnn_cuda
from kws_amd.rnn import gather_windows

A, BM, LAST = _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BATCH_MAJOR, _lib.FLAG_HS_LAST
OK, NULL_POINTER, BAD_SHAPE, WORKSPACE, UNSUPPORTED = 0, 1, 2, 5, 7
SHAPES = [(128, 32), (256, 32), (256, 64)]                # (H, F): what the issue requires and the header lists
T, B, R = 7, 37, 61
fake_ws = C.c_void_p(0x10000)                 # never dereferenced: every call that gets it is refused before a launch


def _desc(H, F, T=T, B=B, gate=0, update=2, dtype=_lib.F32, flags=0, rw=0, ru=0):
    return _lib.Desc(T, B, F, H, rw, ru, gate, update, dtype, flags)


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("fastgrnn_hip_windows_supported", "fastgrnn_hip_forward_windows_workspace_bytes",
                 "fastgrnn_hip_forward_windows"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert lib.fastgrnn_hip_abi_version() == 1


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("affine", [0, A], ids=["plain", "affine"])
@pytest.mark.parametrize("layout", [0, BM, LAST], ids=["time_major", "batch_major", "last_state"])
@pytest.mark.parametrize("gate", [0, 1, 2], ids=["sigmoid", "relu", "tanh"])
def test_supported_shapes(H, F, affine, layout, gate):
    lib = _lib.load()
    for b in (16, B, 4096):
        d = _desc(H, F, B=b, gate=gate, flags=affine | layout)
        assert lib.fastgrnn_hip_windows_supported(C.byref(d)) == 1
    assert fastgrnn_cuda.windows_supported(T, B, F, H, gate_nl=gate, flags=affine | layout)


@pytest.mark.parametrize("H,F", SHAPES)
def test_unsupported_descriptors(H, F):
    lib = _lib.load()
    no = lambda d: lib.fastgrnn_hip_windows_supported(C.byref(d)) == 0 and \
        lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R) == 0            # noqa: E731
    assert no(_desc(H, F, dtype=_lib.BF16_IO))
    assert no(_desc(H, F, dtype=_lib.F64))
    assert no(_desc(H, F, rw=8, ru=8))                                       # low-rank
    assert no(_desc(H, F, rw=8)) and no(_desc(H, F, ru=8))
    assert no(_desc(H, F, gate=_lib.NONLINEARITY["quantSigm"]))
    assert no(_desc(H, F, update=_lib.NONLINEARITY["quantTanh"]))
    for fl in (_lib.FLAG_SAVE_PREACT, _lib.FLAG_X_BFT, _lib.FLAG_BN_TRAIN, _lib.FLAG_ZERO_EXTEND,
               _lib.FLAG_FORCE_GENERIC, _lib.FLAG_FORCE_F32_MFMA, _lib.FLAG_GRAD_LAST, _lib.FLAG_FWD_4WAVE,
               _lib.FLAG_FWD_BF16X3, _lib.FLAG_NO_INPUT_GRAD):
        assert no(_desc(H, F, flags=fl)), fl
        assert no(_desc(H, F, flags=fl | A)), fl
    assert no(_desc(100, F))                                                 # H = 100
    assert no(_desc(H, 24))
    assert not fastgrnn_cuda.windows_supported(T, B, F, H, dtype=torch.bfloat16)
    assert not fastgrnn_cuda.windows_supported(T, B, F, H, w_rank=8, u_rank=8)


def test_shapes_the_header_does_not_list():
    lib = _lib.load()
    for H, F in ((128, 64), (128, 128), (128, 256), (256, 128), (64, 32)):
        for fl in (0, A):
            assert lib.fastgrnn_hip_windows_supported(C.byref(_desc(H, F, flags=fl))) == 0, (H, F)


@pytest.mark.parametrize("H,F", SHAPES)
def test_argument_errors(H, F):
    lib = _lib.load()
    fake = C.c_void_p(0x10000)                 # never dereferenced: every call below is refused before a launch
    prm = _lib.Params(fake, fake, None, None, None, None, fake, fake, fake, fake)
    call = lib.fastgrnn_hip_forward_windows
    d, da = _desc(H, F), _desc(H, F, flags=A)
    big = 1 << 40

    def run(desc, sg=None, sc=None, pool=fake, rows=R, start=fake, h0=fake, hs=fake, ws=fake_ws, nbytes=big, params=prm):
        return call(C.byref(desc), C.byref(params), sg, sc, pool, rows, start, h0, hs, ws, nbytes, None)

    assert run(d, start=None) == NULL_POINTER
    assert run(d, pool=None) == NULL_POINTER
    assert run(d, hs=None) == NULL_POINTER
    assert run(d, h0=None) == NULL_POINTER
    assert run(da, sg=fake, sc=None) == NULL_POINTER                         # exactly one scale
    assert run(da, sg=None, sc=fake) == NULL_POINTER
    assert run(d, sg=fake, sc=None) == NULL_POINTER
    assert run(da) == NULL_POINTER                                           # the flag without scales
    assert run(d, sg=fake, sc=fake) == UNSUPPORTED                           # scales without the flag
    assert run(d, params=_lib.Params(None, fake, None, None, None, None, fake, fake, fake, fake)) == NULL_POINTER
    for desc, sc in ((d, None), (da, fake)):
        assert run(desc, sg=sc, sc=sc, rows=T - 1) == BAD_SHAPE              # pool_rows < T
        assert run(desc, sg=sc, sc=sc, rows=0) == BAD_SHAPE
        assert run(desc, sg=sc, sc=sc, rows=1 << 31) == BAD_SHAPE            # starts are int32
        assert run(desc, sg=sc, sc=sc, rows=1 << 62) == BAD_SHAPE            # size overflow
    assert run(_desc(H, F, T=0)) == BAD_SHAPE
    assert run(_desc(H, F, dtype=_lib.BF16_IO)) == UNSUPPORTED
    assert run(_desc(H, F, rw=8, ru=8), params=_lib.Params(None, None, fake, fake, fake, fake, fake, fake, fake, fake)) \
        == UNSUPPORTED
    assert run(_desc(H, F, gate=4)) == UNSUPPORTED
    assert run(_desc(H, F, gate=9)) == 3                                     # BAD_NONLINEARITY, as everywhere
    for fl in (_lib.FLAG_SAVE_PREACT, _lib.FLAG_X_BFT, _lib.FLAG_ZERO_EXTEND, _lib.FLAG_BN_TRAIN,
               _lib.FLAG_FORCE_GENERIC, _lib.FLAG_FORCE_F32_MFMA):
        assert run(_desc(H, F, flags=fl)) == UNSUPPORTED, fl
    assert run(_desc(100, F)) == UNSUPPORTED
    need = lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R)
    if need:
        assert run(d, ws=None, nbytes=0) == WORKSPACE
        assert run(d, nbytes=need - 1) == WORKSPACE
        assert run(d, ws=C.c_void_p(0x10010)) == WORKSPACE                   # not 256-byte aligned
        assert run(da, sg=fake, sc=fake, nbytes=need - 1) == WORKSPACE
    else:
        assert (H, F) == (128, 32)


def test_workspace_follows_the_pool_not_the_batch():
    lib = _lib.load()
    q = lambda H, F, rows, b=B, t=T, fl=0: int(lib.fastgrnn_hip_forward_windows_workspace_bytes(   # noqa: E731
        C.byref(_desc(H, F, T=t, B=b, flags=fl)), rows))
    base = q(256, 64, 61)
    assert base >= 61 * 256 * 4
    assert q(256, 64, 4194) - base >= (4194 - 61) * 256 * 4 - 256            # P_pool[R, 256] fp32, 256-byte granules
    assert q(256, 64, 4194) - base <= (4194 - 61) * 256 * 4 + 256
    assert q(256, 64, 62) > base or q(256, 64, 125) > base                   # grows with R
    for b, t in [(b, t) for b in (1, 16, 37, 4096) for t in (1, 7, 61)] + [(100000, 7), (1 << 20, 1)]:
        for fl in (0, A, BM, LAST | A):
            assert q(256, 64, 61, b=b, t=t, fl=fl) == base, (b, t, fl)       # ... and with nothing else
    assert q(256, 32, 61) == q(256, 32, 100000) == q(256, 32, 61, b=4096)    # F = 32: no frame product to park
    assert q(256, 32, 61) < base
    assert q(128, 32, 61) == 0 and q(128, 32, 100000) == 0
    # the existing forward parks T*B rows for the same cell: the windowed call does not
    d = _desc(256, 64, T=99, B=4096)
    assert lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)) >= 99 * 4096 * 1024
    assert q(256, 64, 4096 + 98, b=4096, t=99) < 6 * 1024 * 1024


def test_existing_entry_points_do_not_know_windows():
    """No descriptor flag was added for the windowed call: the older queries answer for a descriptor exactly as on the
    parent (spot values of the header's table)."""
    lib = _lib.load()
    assert lib.fastgrnn_hip_kernel_path(C.byref(_desc(256, 64)), 0) == 2
    assert lib.fastgrnn_hip_forward_workspace_bytes(C.byref(_desc(128, 32))) == 0
    used = 0
    for name in dir(_lib):
        if name.startswith("FLAG_"):
            used |= getattr(_lib, name)
    assert used == 1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192


def test_gather_windows_and_range_check_on_the_host():
    pool = torch.arange(61 * 3, dtype=torch.float32).reshape(61, 3)
    starts = torch.tensor([0, 54, 9, 9], dtype=torch.int32)
    w = gather_windows(pool, starts, 7)
    assert w.shape == (4, 7, 3)
    for b, s in enumerate(starts.tolist()):
        assert torch.equal(w[b], pool[s:s + 7])
    with pytest.raises(ValueError):
        gather_windows(pool, torch.tensor([55]), 7)
    with pytest.raises(ValueError):
        gather_windows(pool, torch.tensor([-1]), 7)
    with pytest.raises(ValueError):
        gather_windows(pool, torch.tensor([0]), 62)


def test_score_stream_argument_errors():
    model = RNNClassifierModel("FastGRNNCUDA", 32, 2, [256, 128], [None, None], [None, None], [1.0, 1.0], [1.0, 1.0],
                               "sigmoid", "tanh", num_classes=12, device="cpu")
    with pytest.raises(ValueError):
        model.score_stream(torch.zeros(2, 6, 32), hop=1, window=7)          # L < window
    with pytest.raises(ValueError):
        model.score_stream(torch.zeros(2, 23, 32), hop=0, window=7)
    with pytest.raises(ValueError):
        model.score_stream(torch.zeros(32), hop=1, window=7)
    assert model.hidden_states == [None, None]
