"""fastgrnn_hip_forward_windows_train / fastgrnn_hip_backward_windows without a GPU: the five symbols, which descriptors
the two calls hold, the argument errors (every call below is refused before a launch), the workspace answers, what the
older window entry points still answer, and the Python side's checks that need no device."""
import ctypes as C

import pytest
import torch

from kws_amd import FastGRNNCUDA, RNNClassifierModel, _lib, fastgrnn_cuda
from kws_amd.rnn import gather_windows

BM, GL, SP = _lib.FLAG_BATCH_MAJOR, _lib.FLAG_GRAD_LAST, _lib.FLAG_SAVE_PREACT
OK, NULL_POINTER, BAD_SHAPE, WORKSPACE, UNSUPPORTED = 0, 1, 2, 5, 7
SHAPES = [(128, 32), (256, 32), (256, 64)]                # (H, F): what the issue requires and the header lists
T, B, R = 7, 37, 61
INT32_MAX = (1 << 31) - 1
fake = C.c_void_p(0x10000)                    # never dereferenced: every call that gets it is refused before a launch
SYMBOLS = ("fastgrnn_hip_train_windows_supported", "fastgrnn_hip_train_windows_forward_workspace_bytes",
           "fastgrnn_hip_train_windows_backward_workspace_bytes", "fastgrnn_hip_forward_windows_train",
           "fastgrnn_hip_backward_windows")
ALL_FLAGS = [getattr(_lib, n) for n in dir(_lib) if n.startswith("FLAG_")]


def _desc(H, F, T=T, B=B, gate=0, update=2, dtype=_lib.F32, flags=0, rw=0, ru=0):
    return _lib.Desc(T, B, F, H, rw, ru, gate, update, dtype, flags)


def _align256(n):
    return (n + 255) // 256 * 256


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert lib.fastgrnn_hip_abi_version() == 1 and _lib.ABI_VERSION == 1


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("layout", [0, BM], ids=["time_major", "batch_major"])
@pytest.mark.parametrize("gate", [0, 1, 2], ids=["sigmoid", "relu", "tanh"])
def test_supported_shapes(H, F, layout, gate):
    lib = _lib.load()
    for b in (1, 16, B, 4096):
        for t in (1, T, 99):
            for gl in (0, GL):
                d = _desc(H, F, T=t, B=b, gate=gate, flags=layout | gl)
                assert lib.fastgrnn_hip_train_windows_supported(C.byref(d)) == 1, (b, t, gl)
    assert fastgrnn_cuda.train_windows_supported(T, B, F, H, gate_nl=gate, flags=layout)
    assert fastgrnn_cuda.train_windows_supported(T, B, F, H, gate_nl=gate, flags=layout | GL)


def _refused(d):
    lib = _lib.load()
    return (lib.fastgrnn_hip_train_windows_supported(C.byref(d)) == 0
            and lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(d), R) == 0
            and lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), R) == 0)


@pytest.mark.parametrize("H,F", SHAPES)
def test_unsupported_descriptors(H, F):
    assert _refused(_desc(H, F, dtype=_lib.BF16_IO))
    assert _refused(_desc(H, F, dtype=_lib.F64))
    assert _refused(_desc(H, F, rw=8, ru=8))                                  # factorised operands
    assert _refused(_desc(H, F, rw=8)) and _refused(_desc(H, F, ru=8))
    for code in ("quantTanh", "quantSigm", "quantSigm4"):
        assert _refused(_desc(H, F, gate=_lib.NONLINEARITY[code])), code
    assert _refused(_desc(H, F, update=_lib.NONLINEARITY["quantTanh"]))
    assert _refused(_desc(H, F, update=0))
    assert _refused(_desc(100, F))                                            # H = 100
    assert _refused(_desc(H, 24))
    for fl in ALL_FLAGS:                                                      # every flag outside the accepted ones
        if fl in (BM, GL):
            continue
        for extra in (0, BM, GL):
            assert _refused(_desc(H, F, flags=fl | extra)), (fl, extra)
    assert not fastgrnn_cuda.train_windows_supported(T, B, F, H, dtype=torch.bfloat16)
    assert not fastgrnn_cuda.train_windows_supported(T, B, F, H, dtype=torch.float64)
    assert not fastgrnn_cuda.train_windows_supported(T, B, F, H, w_rank=8, u_rank=8)
    assert not fastgrnn_cuda.train_windows_supported(T, B, F, H, flags=SP)


def test_shapes_the_header_does_not_list():
    for H, F in ((128, 64), (128, 128), (128, 256), (256, 128), (64, 32), (100, 32)):
        for fl in (0, BM, GL):
            assert _refused(_desc(H, F, flags=fl)), (H, F, fl)


def test_every_flag_is_known():
    """The accepted set is stated against the whole flag table: a new flag has to be placed on one side here."""
    used = 0
    for fl in ALL_FLAGS:
        used |= fl
    assert used == 1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512 | 1024 | 2048 | 4096 | 8192


def _params(w=fake, u=fake, bg=fake, bu=fake, zeta=fake, nu=fake):
    return _lib.Params(w, u, None, None, None, None, bg, bu, zeta, nu)


def _grads(**kw):
    g = dict(d_x=None, d_bias_gate=fake, d_bias_update=fake, d_zeta=fake, d_nu=fake, d_h0=fake, d_w=fake, d_u=fake,
             d_w1=None, d_w2=None, d_u1=None, d_u2=None)
    g.update(kw)
    return _lib.Grads(*[g[n] for n, _ in _lib.Grads._fields_])


BIG = 1 << 40


def _fwd(desc, pool=fake, rows=R, start=fake, h0=fake, hs=fake, saved=fake, ws=fake, nbytes=BIG, params=None):
    params = _params() if params is None else params
    return _lib.load().fastgrnn_hip_forward_windows_train(C.byref(desc), C.byref(params), pool, rows, start, h0, hs,
                                                          saved, ws, nbytes, None)


def _bwd(desc, ghs=fake, pool=fake, rows=R, start=fake, hs=fake, saved=fake, h0=fake, grads=None, ws=fake, nbytes=BIG,
         params=None):
    params = _params() if params is None else params
    grads = _grads() if grads is None else grads
    return _lib.load().fastgrnn_hip_backward_windows(C.byref(desc), C.byref(params), ghs, pool, rows, start, hs, saved,
                                                     h0, C.byref(grads) if grads is not False else None, ws, nbytes,
                                                     None)


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("layout", [0, BM], ids=["time_major", "batch_major"])
def test_forward_argument_errors(H, F, layout):
    lib = _lib.load()
    d = _desc(H, F, flags=layout)
    for name in ("pool", "start", "h0", "hs", "saved"):
        assert _fwd(d, **{name: None}) == NULL_POINTER, name
    for name in ("w", "u", "bg", "bu", "zeta", "nu"):
        assert _fwd(d, params=_params(**{name: None})) == NULL_POINTER, name
    assert _fwd(d, rows=T - 1) == BAD_SHAPE                                  # pool_rows < T
    assert _fwd(d, rows=0) == BAD_SHAPE
    assert _fwd(d, rows=INT32_MAX + 1) == BAD_SHAPE                          # starts are int32
    assert _fwd(d, rows=1 << 62) == BAD_SHAPE                                # size overflow
    assert _fwd(_desc(H, F, T=0)) == BAD_SHAPE
    assert _fwd(_desc(H, F, gate=9)) == 3                                    # BAD_NONLINEARITY, as everywhere
    assert _fwd(_desc(H, F, flags=layout | GL)) == UNSUPPORTED               # GRAD_LAST is the backward's
    assert _fwd(_desc(H, F, flags=layout | SP)) == UNSUPPORTED               # the contract is implied, the flag refused
    assert _fwd(_desc(H, F, flags=layout | _lib.FLAG_HS_LAST)) == UNSUPPORTED
    assert _fwd(_desc(H, F, dtype=_lib.BF16_IO)) == UNSUPPORTED
    assert _fwd(_desc(H, F, gate=4)) == UNSUPPORTED
    assert _fwd(_desc(100, F)) == UNSUPPORTED
    assert _fwd(_desc(H, F, rw=8, ru=8),
                params=_lib.Params(None, None, fake, fake, fake, fake, fake, fake, fake, fake)) == UNSUPPORTED
    need = int(lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(d), R))
    if H == 256:                                 # the scans read the pool in place: the inference call's workspace
        assert need == int(lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R))
    else:                                        # H = 128: the gathered copy of x, [T,B,F] fp32
        assert need == (d.T * d.B * d.F * 4 + 255) // 256 * 256
    assert _fwd(d, ws=None, nbytes=0) == WORKSPACE
    assert _fwd(d, nbytes=need - 1) == WORKSPACE
    assert _fwd(d, ws=C.c_void_p(0x10010)) == WORKSPACE                      # not 256-byte aligned
    assert int(lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(_desc(H, F, flags=layout | GL)), R)) == 0
    assert int(lib.fastgrnn_hip_train_windows_forward_workspace_bytes(C.byref(d), INT32_MAX + 1)) == 0


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("flags", [0, BM, GL, BM | GL], ids=["tm", "bm", "tm_last", "bm_last"])
def test_backward_argument_errors(H, F, flags):
    lib = _lib.load()
    d = _desc(H, F, flags=flags)
    for name in ("ghs", "pool", "start", "hs", "saved", "h0"):
        assert _bwd(d, **{name: None}) == NULL_POINTER, name
    assert _bwd(d, grads=False) == NULL_POINTER
    for name in ("w", "u", "bg", "bu", "zeta", "nu"):
        assert _bwd(d, params=_params(**{name: None})) == NULL_POINTER, name
    for name in ("d_bias_gate", "d_bias_update", "d_zeta", "d_nu", "d_h0", "d_w", "d_u"):
        assert _bwd(d, grads=_grads(**{name: None})) == NULL_POINTER, name
    assert _bwd(d, grads=_grads(d_x=fake)) == UNSUPPORTED                    # the scatter-add into the pool: not built
    assert _bwd(d, rows=T - 1) == BAD_SHAPE
    assert _bwd(d, rows=0) == BAD_SHAPE
    assert _bwd(d, rows=INT32_MAX + 1) == BAD_SHAPE
    assert _bwd(d, rows=1 << 62) == BAD_SHAPE
    assert _bwd(_desc(H, F, T=0, flags=flags)) == BAD_SHAPE
    assert _bwd(_desc(H, F, flags=flags | SP)) == UNSUPPORTED
    assert _bwd(_desc(H, F, flags=flags | _lib.FLAG_NO_INPUT_GRAD)) == UNSUPPORTED
    assert _bwd(_desc(H, F, flags=flags | _lib.FLAG_X_BFT)) == UNSUPPORTED
    assert _bwd(_desc(H, F, dtype=_lib.BF16_IO, flags=flags)) == UNSUPPORTED
    assert _bwd(_desc(100, F, flags=flags)) == UNSUPPORTED
    need = int(lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), R))
    assert need > 0
    assert _bwd(d, ws=None, nbytes=0) == WORKSPACE
    assert _bwd(d, nbytes=need - 1) == WORKSPACE
    assert _bwd(d, ws=C.c_void_p(0x10010)) == WORKSPACE
    assert int(lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), INT32_MAX + 1)) == 0


@pytest.mark.parametrize("flags", [0, BM, GL, BM | GL], ids=["tm", "bm", "tm_last", "bm_last"])
def test_backward_workspace_is_the_existing_one_plus_the_gathered_copy(flags):
    lib = _lib.load()
    q = lambda d, rows: int(lib.fastgrnn_hip_train_windows_backward_workspace_bytes(C.byref(d), rows))   # noqa: E731
    for F in (32, 64):
        for t, b in ((T, B), (1, 1), (99, 4096), (2, 17)):
            d = _desc(256, F, T=t, B=b, flags=flags)
            base = int(lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)))
            assert base > 0
            for rows in (max(t, R), 100000):
                assert q(d, rows) == base + _align256(t * b * F * 4), (F, t, b, rows)
    # H = 128 takes the same route (no scan reads the pool in place), whatever the pool's size
    for t, b in ((T, B), (99, 4096)):
        d = _desc(128, 32, T=t, B=b, flags=flags)
        base = int(lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)))
        for rows in (R if t <= R else 4200, (1 << 25) - 1, 1 << 25, INT32_MAX):
            assert q(d, rows) == base + _align256(t * b * 32 * 4), rows


def test_the_older_window_entry_points_still_refuse_save_preact():
    lib = _lib.load()
    prm = _params()
    for H, F in SHAPES:
        for fl in (SP, SP | BM):
            d = _desc(H, F, flags=fl)
            assert lib.fastgrnn_hip_windows_supported(C.byref(d)) == 0
            assert lib.fastgrnn_hip_forward_windows_workspace_bytes(C.byref(d), R) == 0
            st = lib.fastgrnn_hip_forward_windows(C.byref(d), C.byref(prm), None, None, fake, R, fake, fake, fake, fake,
                                                  BIG, None)
            assert st == UNSUPPORTED
        assert lib.fastgrnn_hip_windows_supported(C.byref(_desc(H, F))) == 1


def test_unroll_windows_refuses_a_pool_that_requires_grad():
    m = FastGRNNCUDA(32, 128, device="cpu")
    pool = torch.zeros(61, 32, requires_grad=True)
    with pytest.raises(ValueError, match="require grad"):
        m.unroll_windows(pool, torch.tensor([0, 3]), 7)
    model = RNNClassifierModel("FastGRNNCUDA", 32, 2, [256, 128], [None, None], [None, None], [1.0, 1.0], [1.0, 1.0],
                               "sigmoid", "tanh", num_classes=12, device="cpu")
    with pytest.raises(ValueError, match="require grad"):
        model.loss_windows(pool, torch.tensor([0, 3]), torch.tensor([1, 2]), window=7)
    assert model.hidden_states == [None, None]


def _message(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


def test_range_check_messages_match_forward_windows():
    """The host check of the training calls words its errors as forward_windows / gather_windows do."""
    pool = torch.arange(61 * 3, dtype=torch.float32).reshape(61, 3)
    for bad in (torch.tensor([55]), torch.tensor([3, -1]), torch.tensor([0, 54, 200], dtype=torch.int32)):
        assert _message(lambda: fastgrnn_cuda.check_starts_range(bad, 61, 7)) == \
            _message(lambda: gather_windows(pool, bad, 7))
    assert _message(lambda: fastgrnn_cuda.check_starts_range(torch.tensor([0]), 61, 62)) == \
        _message(lambda: gather_windows(pool, torch.tensor([0]), 62))
    fastgrnn_cuda.check_starts_range(torch.tensor([0, 54]), 61, 7)            # both ends are in range
    model = RNNClassifierModel("FastGRNNCUDA", 3, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=12, device="cpu")
    assert _message(lambda: model.loss_windows(pool, torch.tensor([55]), torch.tensor([1]), window=7)) == \
        _message(lambda: gather_windows(pool, torch.tensor([55]), 7))
    # a cell the training calls do not hold gathers and runs forward: the same check, the same words
    m = FastGRNNCUDA(3, 128, device="cpu")
    assert _message(lambda: m.unroll_windows(pool, torch.tensor([55]), 7)) == \
        _message(lambda: gather_windows(pool, torch.tensor([55]), 7))
