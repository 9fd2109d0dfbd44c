"""CPU-side checks of FASTGRNN_FLAG_ZERO_EXTEND (include/fastgrnn_hip.h): which descriptors take the padded route, the
padded shape and saved-buffer size the plan query reports, that the flag changes nothing where it does not apply, and
that the copy kernels of kernels_zext.hip pass both static assembly scanners.  No kernel is launched here."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from kws_amd import _lib, fastgrnn_cuda
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ZE, SP = _lib.FLAG_ZERO_EXTEND, _lib.FLAG_SAVE_PREACT


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def _desc(**kw):
    base = dict(T=99, B=4096, F=32, H=128, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=0, flags=0)
    base.update(kw)
    return _lib.Desc(**base)


def _answers(lib, d):
    return (lib.fastgrnn_hip_kernel_path(C.byref(d), 0), lib.fastgrnn_hip_kernel_path(C.byref(d), 1),
            lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)), lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)))


def _plan(lib, d):
    p = _lib.ZextPlan()
    assert lib.fastgrnn_hip_zero_extend_plan(C.byref(d), C.byref(p)) == 0
    return p


def _a256(n):
    return (n + 255) // 256 * 256


def test_the_issue_shape_leaves_the_generic_scan():
    assert fastgrnn_cuda.kernel_path(99, 4096, 32, 100, flags=SP, direction=1) == 0
    assert fastgrnn_cuda.kernel_path(99, 4096, 32, 100, flags=SP | ZE, direction=1) == 2
    assert fastgrnn_cuda.kernel_path(99, 4096, 32, 100, flags=SP | ZE, direction=0) == 2


ODD = [(7, 20), (100, 100), (32, 1), (40, 129), (64, 200), (32, 255), (13, 16), (100, 33), (40, 127)]


@pytest.mark.parametrize("F,H", ODD)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_odd_shapes_go_to_path_2(F, H, dtype):
    bf = dtype == torch.bfloat16
    # (bf16 sequences: the padded H = 256 scans have no batch-major backward; last-state forwards are dense
    # H = 128 / F = 32 only -- the table of include/fastgrnn_hip.h)
    for flags in (SP, SP | _lib.FLAG_BATCH_MAJOR):
        assert fastgrnn_cuda.kernel_path(99, 4096, F, H, dtype=dtype, flags=flags, direction=1) == 0
        want = 0 if (bf and H > 128 and flags & _lib.FLAG_BATCH_MAJOR) else 2
        for direction in (0, 1):
            assert fastgrnn_cuda.kernel_path(99, 4096, F, H, dtype=dtype, flags=flags | ZE, direction=direction) == want
    # hs-only / last-state forwards (inference)
    assert fastgrnn_cuda.kernel_path(99, 37, F, H, dtype=dtype, flags=ZE, direction=0) == 2
    want = 0 if (bf and (H > 128 or F > 32)) else 2
    assert fastgrnn_cuda.kernel_path(99, 37, F, H, dtype=dtype, flags=ZE | _lib.FLAG_HS_LAST, direction=0) == want


def test_h64_f32_stays_on_path_1_in_fp32_and_pads_in_bf16():
    for flags in (0, SP, ZE, SP | ZE):
        for direction in (0, 1):
            assert fastgrnn_cuda.kernel_path(99, 4096, 32, 64, flags=flags, direction=direction) == 1
    assert fastgrnn_cuda.kernel_path(99, 4096, 32, 64, dtype=torch.bfloat16, flags=SP, direction=1) == 0
    for direction in (0, 1):
        assert fastgrnn_cuda.kernel_path(99, 4096, 32, 64, dtype=torch.bfloat16, flags=SP | ZE, direction=direction) == 2


def test_grad_last_and_factorised_cells(lib):
    # the classifier's last layer at H = 100 (GRAD_LAST carries over to the padded H = 128 scans)
    assert fastgrnn_cuda.kernel_path(99, 4096, 100, 100, flags=SP | ZE | _lib.FLAG_GRAD_LAST, direction=1) == 2
    # factorised: ranks <= 16 at H = 200, F <= 32 run on the low-rank H = 256 scans; others densified
    for F, H, rw, ru, Hp, Fp in ((20, 200, 8, 16, 256, 32), (32, 100, 5, 7, 128, 32), (40, 129, 20, 3, 256, 64),
                                 (7, 20, 4, 0, 128, 32), (32, 255, 0, 16, 256, 32)):
        d = _desc(F=F, H=H, w_rank=rw, u_rank=ru, flags=SP | ZE)
        assert _answers(lib, _desc(F=F, H=H, w_rank=rw, u_rank=ru, flags=SP))[:2] == (0, 0)
        assert _answers(lib, d)[:2] == (2, 2), (F, H, rw, ru)
        p = _plan(lib, d)
        assert (p.forward, p.backward, p.Hp, p.Fp) == (1, 1, Hp, Fp)
        TB = 99 * 4096
        lowrank = Hp == 256 and Fp == 32 and 1 <= rw <= 16 and 1 <= ru <= 16
        assert p.saved_bytes == _a256(TB * Hp * 4) + _a256(TB * Hp * 4) + (_a256(TB * 32 * 4) if lowrank else 0)


@pytest.mark.parametrize("F,H,Hp,Fp", [(32, 100, 128, 32), (7, 20, 128, 32), (100, 100, 128, 128), (32, 1, 128, 32),
                                      (40, 129, 256, 64), (64, 200, 256, 64), (32, 255, 256, 32), (40, 128, 128, 64),
                                      (257 - 1, 100, 128, 256), (128, 200, 256, 128)])
def test_plan_reports_the_padded_shape(lib, F, H, Hp, Fp):
    TB = 99 * 4096
    for dtype, esz in ((0, 4), (2, 2)):
        d = _desc(F=F, H=H, dtype=dtype, flags=SP | ZE)
        p = _plan(lib, d)
        assert (p.forward, p.backward, p.Hp, p.Fp) == (1, 1, Hp, Fp), (F, H, dtype)
        want = _a256(TB * Hp * 4) + (_a256(TB * Hp * esz) if H != Hp else 0)
        assert p.saved_bytes == want
        # without SAVE_PREACT only the hs-only forward is padded, and nothing is saved
        q = _plan(lib, _desc(F=F, H=H, dtype=dtype, flags=ZE))
        assert (q.forward, q.backward, q.Hp, q.Fp, q.saved_bytes) == (1, 0, Hp, Fp, 0)
        assert lib.fastgrnn_hip_kernel_path(C.byref(_desc(F=F, H=H, dtype=dtype, flags=ZE)), 1) == \
            lib.fastgrnn_hip_kernel_path(C.byref(_desc(F=F, H=H, dtype=dtype)), 1)
        # the workspace covers at least the padded operands and the inner path-2 workspace
        e = _desc(F=Fp, H=Hp, dtype=dtype, flags=SP)
        fw, bw = _answers(lib, d)[2:]
        assert fw >= lib.fastgrnn_hip_forward_workspace_bytes(C.byref(e)) + (Hp * Hp * 4 if H != Hp else 0)
        assert bw >= lib.fastgrnn_hip_backward_workspace_bytes(C.byref(e)) + (2 * Hp * Hp * 4 if H != Hp else 0)


NATIVE = [dict(F=32, H=128), dict(F=64, H=128), dict(F=128, H=128), dict(F=256, H=128), dict(F=32, H=256),
          dict(F=64, H=256), dict(F=128, H=256), dict(F=32, H=256, w_rank=8, u_rank=16),
          dict(F=32, H=128, w_rank=20, u_rank=20), dict(F=64, H=256, w_rank=4, u_rank=4),
          dict(F=32, H=128, gate_nl=4), dict(F=32, H=128, dtype=2), dict(F=64, H=128, dtype=2)]
NOT_APPLICABLE = [dict(F=32, H=100, dtype=1), dict(F=7, H=20, dtype=1), dict(F=32, H=300), dict(F=300, H=128),
                  dict(F=256, H=256), dict(F=200, H=200), dict(F=32, H=64),
                  dict(F=32, H=100, update_nl=0), dict(F=32, H=100, update_nl=3, dtype=2)]
FLAGS = [_lib.FLAG_X_BFT, _lib.FLAG_PREACT_AFFINE, _lib.FLAG_BN_TRAIN, _lib.FLAG_FORCE_GENERIC,
         _lib.FLAG_FORCE_F32_MFMA]


@pytest.mark.parametrize("kw", NATIVE + NOT_APPLICABLE, ids=lambda kw: "-".join("%s%s" % i for i in kw.items()))
def test_flag_changes_nothing_where_it_does_not_apply(lib, kw):
    for extra in (0, SP, SP | _lib.FLAG_BATCH_MAJOR, _lib.FLAG_HS_LAST, SP | _lib.FLAG_GRAD_LAST):
        d0, d1 = _desc(flags=extra, **kw), _desc(flags=extra | ZE, **kw)
        assert _answers(lib, d0) == _answers(lib, d1), (kw, extra)
        p = _plan(lib, d1)
        assert (p.forward, p.backward, p.Hp, p.Fp, p.saved_bytes) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("F,H", [(32, 100), (7, 20), (64, 200), (32, 128)])
def test_excluded_flags_turn_the_route_off(lib, flag, F, H):
    for extra in (0, SP):
        d0, d1 = _desc(F=F, H=H, flags=flag | extra), _desc(F=F, H=H, flags=flag | extra | ZE)
        assert _answers(lib, d0) == _answers(lib, d1), (flag, extra)
        p = _plan(lib, d1)
        assert p.forward == 0 and p.saved_bytes == 0
        assert lib.fastgrnn_hip_bn_train_supported(C.byref(d0)) == lib.fastgrnn_hip_bn_train_supported(C.byref(d1))
        for q in (lib.fastgrnn_hip_bn_train_forward_workspace_bytes, lib.fastgrnn_hip_bn_train_backward_workspace_bytes):
            assert q(C.byref(d0)) == q(C.byref(d1))


def test_bn_train_entry_points_ignore_the_flag(lib):
    d0 = _desc(F=32, H=128, flags=_lib.FLAG_BN_TRAIN)
    d1 = _desc(F=32, H=128, flags=_lib.FLAG_BN_TRAIN | ZE)
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(d0)) == 1
    assert lib.fastgrnn_hip_bn_train_supported(C.byref(d1)) == 1
    assert lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(d1)) == \
        lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(d0))


def test_plan_query_arguments(lib):
    p = _lib.ZextPlan()
    assert lib.fastgrnn_hip_zero_extend_plan(None, C.byref(p)) == 1
    assert lib.fastgrnn_hip_zero_extend_plan(C.byref(_desc()), None) == 1
    assert lib.fastgrnn_hip_zero_extend_plan(C.byref(_desc(T=0, flags=ZE)), C.byref(p)) == 2
    assert fastgrnn_cuda.zero_extend_plan(99, 4096, 32, 100, flags=SP) == dict(
        forward=1, backward=1, Hp=128, Fp=32, dx_optional=0, saved_bytes=2 * _a256(99 * 4096 * 128 * 4))
    assert fastgrnn_cuda.zero_extend_plan(99, 4096, 32, 128, flags=SP)["forward"] == 0


def test_calls_without_a_device_are_refused_for_their_arguments(lib):
    """Argument checks on the padded route come before any launch (NULL pointers, workspace)."""
    d = _desc(F=32, H=100, flags=SP | ZE)
    params = _lib.Params()
    assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(params), None, None, None, None, None, None, 0,
                                           None) == 1
    params = _lib.Params(*([C.c_void_p(256)] * 10))
    one = C.c_void_p(256)
    # z_s is required under SAVE_PREACT on the padded route
    assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(params), one, one, one, None, None, one, 1 << 40,
                                           None) == 1
    # a workspace smaller than the query's answer
    assert lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(params), one, one, one, one, None, one, 256,
                                           None) == 5


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_copy_kernels_pass_both_scanners(tmp_path):
    src = os.path.join(ROOT, "kws_amd", "csrc", "kernels_zext.hip")
    asm = tmp_path / "kernels_zext.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", str(asm),
                    src], check=True, capture_output=True, timeout=900)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), str(asm)], capture_output=True,
                       text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "total pairs: 0", r.stdout[-2000:] + r.stderr[-2000:]
    assert any(l.startswith("kernels declared 1, scanned 1") for l in lines), lines
    for mode in ("--strict", "--narrow"):
        r2 = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), str(asm), mode],
                            capture_output=True, text=True, timeout=300)
        assert r2.returncode == 0, r2.stderr[-2000:]
        assert r2.stdout.strip().splitlines()[-1] == "sites in loops: 0", r2.stdout[-2000:]
    text = asm.read_text()
    assert "scratch_" not in text and ".private_segment_fixed_size: 0" in text.replace("\t", " ").replace("  ", " ")
