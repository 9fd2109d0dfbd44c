"""CPU-side checks of fastgrnn_hip_plan (include/fastgrnn_hip.h): over the descriptor grid of
tests/plan_table_cases.py, with and without FASTGRNN_FLAG_NO_INPUT_GRAD, the plan agrees field by field with the older
single-answer queries; dx_optional agrees with what backward_unroll itself accepts; forward_ws_optional and
rank_space_cols hold exactly on the descriptors listed here.  No kernel is launched: a call that passes the argument
checks stops at the workspace check (status 5)."""
import ctypes as C

import pytest

from kws_amd import _lib
from tests import plan_table_cases as PT
from tests import support as S

NIG, SP, ZE = _lib.FLAG_NO_INPUT_GRAD, _lib.FLAG_SAVE_PREACT, _lib.FLAG_ZERO_EXTEND
BM, BFT = _lib.FLAG_BATCH_MAJOR, _lib.FLAG_X_BFT
ONE = C.c_void_p(256)
NULL = C.c_void_p(None)
ZEXT_FIELDS = ("forward", "backward", "Hp", "Fp", "dx_optional", "reserved", "saved_bytes")


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def _plan(lib, d, status=0):
    p = _lib.Plan()
    assert lib.fastgrnn_hip_plan(C.byref(d), C.byref(p)) == status
    return p


def _backward(lib, d, d_x):
    """status of backward_unroll with every other pointer given and no workspace"""
    p = _lib.Params(*([ONE] * 10))
    g = _lib.Grads(*([d_x] + [ONE] * 11))
    return lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE, C.byref(g), NULL, 0,
                                            NULL)


def test_plan_agrees_with_every_older_query(lib):
    n = 0
    for d in PT.both_grids():
        what = (d.F, d.H, d.w_rank, d.gate_nl, d.update_nl, d.dtype, d.flags)
        plan = _lib.Plan()
        zx = _lib.ZextPlan()
        assert lib.fastgrnn_hip_plan(C.byref(d), C.byref(plan)) == \
            lib.fastgrnn_hip_zero_extend_plan(C.byref(d), C.byref(zx)), what
        for direction in (0, 1):
            assert plan.path[direction] == lib.fastgrnn_hip_kernel_path(C.byref(d), direction), what
        assert plan.workspace_bytes[0] == lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)), what
        assert plan.workspace_bytes[1] == lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)), what
        for f in ZEXT_FIELDS:
            assert getattr(plan.zext, f) == getattr(zx, f), (what, f)
        if plan.zext.backward:
            assert plan.dx_optional == zx.dx_optional, what
        assert plan.forward_ws_optional in (0, 1) and plan.dx_optional in (0, 1) and plan.rank_space_cols in (0, 32)
        n += 1
    assert n > 10000


def test_dx_optional_is_what_backward_unroll_accepts(lib):
    """d_x == NULL, every other pointer given, no workspace: the call reaches the workspace check (5) where the plan
    says dx_optional and stops at the pointer check (1) where it does not.  Only descriptors with a non-zero backward
    workspace are asked, so nothing is ever launched.  A descriptor whose backward is refused as unsupported (7) with
    d_x given is refused the same way without it, and its plan must not call d_x optional."""
    asked = {0: 0, 1: 0}
    for d in PT.both_grids():
        plan = _plan(lib, d)
        if plan.workspace_bytes[1] == 0:
            continue
        what = (d.B, d.F, d.H, d.w_rank, d.gate_nl, d.update_nl, d.dtype, d.flags)
        with_dx = _backward(lib, d, ONE)
        assert with_dx in (5, 7), what
        if with_dx == 7:
            assert plan.dx_optional == 0 and _backward(lib, d, NULL) == 7, what
            continue
        assert _backward(lib, d, NULL) == (5 if plan.dx_optional else 1), what
        asked[plan.dx_optional] += 1
    assert asked[0] > 500 and asked[1] > 500, asked


# forward_unroll accepts workspace == NULL when z_s is passed: dense H = 128 with a wide input on kernel path 2
WS_OPTIONAL = [dict(F=F, flags=fl, dtype=dt) for F in (64, 128, 256) for fl in (0, SP, BM, SP | BM, SP | ZE, NIG)
               for dt in (0, 2) if not (dt == 2 and fl in (0, BM, NIG))] + \
              [dict(F=F, flags=fl) for F in (64, 128, 256) for fl in (BFT, SP | BFT)] + \
              [dict(F=F, w_rank=0, u_rank=0, gate_nl=g) for F in (64, 256) for g in (1, 2)]
WS_REQUIRED = [dict(), dict(flags=SP), dict(H=256), dict(H=256, F=64, flags=SP), dict(H=256, F=128),
               dict(F=64, w_rank=8, u_rank=8, flags=SP),                 # factorised: multiplied out in the workspace
               dict(F=64, flags=_lib.FLAG_FORCE_GENERIC), dict(F=64, flags=_lib.FLAG_FORCE_F32_MFMA),
               dict(F=64, dtype=1), dict(F=64, update_nl=3),
               dict(F=64, H=100, flags=ZE), dict(F=100, H=100, flags=SP | ZE), dict(F=100, flags=SP | ZE),   # padded route
               dict(F=64, flags=_lib.FLAG_PREACT_AFFINE), dict(F=64, flags=_lib.FLAG_BN_TRAIN)]


def test_forward_ws_optional_on_the_listed_descriptors(lib):
    p = _lib.Params(*([ONE] * 10))
    for kw in WS_OPTIONAL:
        d = PT.desc(**kw)
        plan = _plan(lib, d)
        assert plan.path[0] == 2 and plan.zext.forward == 0 and plan.workspace_bytes[0] > 0, kw
        assert plan.forward_ws_optional == 1, kw
        # without z_s the workspace is required: the call stops there
        assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, NULL, NULL, NULL, 0, NULL) == 5, kw
    for kw in WS_REQUIRED:
        d = PT.desc(**kw)
        plan = _plan(lib, d)
        assert plan.forward_ws_optional == 0, kw
        if plan.workspace_bytes[0] and not d.flags & (_lib.FLAG_PREACT_AFFINE | _lib.FLAG_BN_TRAIN):
            # z_s passed (and c_s for the reference's pair), no workspace: refused, at the workspace check on path 2
            st = lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, NULL, 0, NULL)
            assert st in (5, 7) and (st == 5 or plan.path[0] != 2), (kw, st)


# a SAVE_PREACT forward writes the rank-space vector through c_s: H = 256 / F = 32, both ranks 1..16, kernel path 2
RANK_SPACE = [dict(H=256, w_rank=rw, u_rank=ru, gate_nl=g, flags=SP | fl)
              for rw, ru in ((1, 1), (1, 16), (16, 1), (16, 16), (8, 8), (5, 12)) for g in (0, 1, 2)
              for fl in (0, BM, BFT, ZE, NIG, _lib.FLAG_GRAD_LAST)] + \
             [dict(H=256, w_rank=8, u_rank=8, dtype=2, flags=SP)]
NO_RANK_SPACE = [dict(H=256, w_rank=8, u_rank=8),                          # no SAVE_PREACT
                 dict(H=256, w_rank=17, u_rank=8, flags=SP), dict(H=256, w_rank=8, u_rank=17, flags=SP),
                 dict(H=256, w_rank=8, u_rank=0, flags=SP), dict(H=256, w_rank=0, u_rank=8, flags=SP),
                 dict(H=256, flags=SP), dict(flags=SP), dict(w_rank=8, u_rank=8, flags=SP),
                 dict(H=256, F=64, w_rank=8, u_rank=8, flags=SP),
                 dict(H=256, w_rank=8, u_rank=8, gate_nl=4, flags=SP),     # quantised gate: not on path 2
                 dict(H=256, w_rank=8, u_rank=8, dtype=1, flags=SP),
                 dict(H=256, w_rank=8, u_rank=8, flags=SP | _lib.FLAG_FORCE_GENERIC),
                 dict(H=200, w_rank=8, u_rank=8, flags=SP | ZE)]           # padded route: inside the opaque z_s buffer


def test_rank_space_cols_on_the_listed_descriptors(lib):
    for kw in RANK_SPACE:
        plan = _plan(lib, PT.desc(**kw))
        assert plan.path[0] == 2 and plan.path[1] == 2 and plan.zext.forward == 0, kw
        assert plan.rank_space_cols == 32, kw
    for kw in NO_RANK_SPACE:
        assert _plan(lib, PT.desc(**kw)).rank_space_cols == 0, kw
    zx = _plan(lib, PT.desc(H=200, w_rank=8, u_rank=8, flags=SP | ZE)).zext
    assert (zx.forward, zx.backward, zx.Hp, zx.Fp) == (1, 1, 256, 32)


def test_error_convention(lib):
    p = _lib.Plan()
    assert lib.fastgrnn_hip_plan(None, C.byref(p)) == 1
    assert lib.fastgrnn_hip_plan(C.byref(PT.desc()), None) == 1
    for kw, st in ((dict(T=0, flags=ZE), 2), (dict(gate_nl=9), 3), (dict(dtype=5), 4)):
        p = _plan(lib, PT.desc(F=64, flags=SP))
        assert p.path[0] == 2 and p.forward_ws_optional == 1
        assert lib.fastgrnn_hip_plan(C.byref(PT.desc(**kw)), C.byref(p)) == st
        assert bytes(p) == bytes(C.sizeof(_lib.Plan)), kw           # out zeroed


def test_shim_plan_has_the_library_answers(lib):
    from kws_amd import fastgrnn_cuda
    a = fastgrnn_cuda._plan(99, 4096, 64, 128, 0, 0, 0, 2, _lib.F32, SP)
    p = _plan(lib, a.desc)
    assert (a.path, a.ws) == (tuple(p.path), tuple(p.workspace_bytes))
    assert (a.forward_ws_optional, a.dx_optional, a.rank_space_cols, a.zext.forward) == (True, True, 0, 0)
    b = fastgrnn_cuda._plan(99, 4096, 32, 256, 8, 8, 0, 2, _lib.F32, SP)
    assert (b.forward_ws_optional, b.dx_optional, b.rank_space_cols) == (False, False, 32)
    assert fastgrnn_cuda._plan(0, 4096, 32, 128, 0, 0, 0, 2, _lib.F32, 0).path == (-1, -1)
