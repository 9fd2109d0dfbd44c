"""CPU-side checks of FASTGRNN_FLAG_NO_INPUT_GRAD (include/fastgrnn_hip.h): where backward_unroll accepts d_x == NULL
with and without the flag, that every path choice, workspace query and support predicate answers the same with it,
that the other entry points ignore it, and that the NODX scan variants pass both static assembly scanners.  No kernel
is launched here: a call that passes the argument checks stops at the workspace check (status 5)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from kws_amd import _lib
from tests import plan_table_cases as PT
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NIG, SP, ZE = _lib.FLAG_NO_INPUT_GRAD, _lib.FLAG_SAVE_PREACT, _lib.FLAG_ZERO_EXTEND
ONE = C.c_void_p(256)
NULL = C.c_void_p(None)


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def _backward_without_dx(lib, d):
    """status of backward_unroll with every pointer given but d_x (and no workspace)"""
    p = _lib.Params(*([ONE] * 10))
    g = _lib.Grads(*([NULL] + [ONE] * 11))
    return lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE, C.byref(g), NULL, 0,
                                            NULL)


# dense H = 128 / F = 32 backward configurations on kernel path 2: (gate, update, dtype, flags)
PATH2 = [(gate, 2, 0, fl) for gate in range(3) for fl in (0, SP, _lib.FLAG_BATCH_MAJOR, SP | _lib.FLAG_X_BFT,
                                                            _lib.FLAG_GRAD_LAST, SP | _lib.FLAG_BATCH_MAJOR | _lib.FLAG_GRAD_LAST)] + \
        [(gate, 2, 0, fl) for gate in (4, 5) for fl in (SP, SP | _lib.FLAG_X_BFT, SP | _lib.FLAG_GRAD_LAST)] + \
        [(gate, 2, 2, fl) for gate in range(6) if gate != 3 for fl in (SP, SP | _lib.FLAG_BATCH_MAJOR, SP | _lib.FLAG_X_BFT)] + \
        [(gate, 3, 0, fl) for gate in (0, 1, 4) for fl in (SP, SP | _lib.FLAG_BATCH_MAJOR, SP | _lib.FLAG_GRAD_LAST)]


@pytest.mark.parametrize("gate,update,dtype,flags", PATH2)
@pytest.mark.parametrize("B", [37, 4096])
def test_null_dx_needs_the_flag_on_h128_f32(lib, gate, update, dtype, flags, B):
    d = PT.desc(B=B, gate_nl=gate, update_nl=update, dtype=dtype, flags=flags)
    assert lib.fastgrnn_hip_kernel_path(C.byref(d), 1) == 2
    assert _backward_without_dx(lib, d) == 1                    # as before: d_x is required without the flag
    dn = PT.desc(B=B, gate_nl=gate, update_nl=update, dtype=dtype, flags=flags | NIG)
    assert _backward_without_dx(lib, dn) == 5                   # accepted: the next check is the workspace


def test_the_flag_changes_nothing_where_null_dx_was_accepted_or_refused(lib):
    # already optional: dense H = 256 and dense H = 128 with F > 32 (kernel path 2)
    for kw in (dict(H=256), dict(F=64), dict(F=256)):
        for fl in (SP, SP | NIG):
            assert _backward_without_dx(lib, PT.desc(B=4, T=3, flags=fl, **kw)) == 5
    # still required: other paths and factorised cells, whatever the flag says
    for kw in (dict(flags=_lib.FLAG_FORCE_GENERIC), dict(flags=_lib.FLAG_FORCE_F32_MFMA), dict(H=64),
               dict(H=100), dict(F=20), dict(w_rank=8, u_rank=8, flags=SP), dict(dtype=_lib.F64)):
        for extra in (0, NIG):
            k = dict(kw)
            k["flags"] = k.get("flags", 0) | extra
            d = PT.desc(B=4, T=3, **k)
            if d.w_rank:
                p = _lib.Params(NULL, NULL, *([ONE] * 8))
                g = _lib.Grads(*([NULL] + [ONE] * 11))
                st = lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE, C.byref(g),
                                                      NULL, 0, NULL)
            else:
                st = _backward_without_dx(lib, d)
            assert st == 1, (kw, extra)


def test_single_step_backward_ignores_the_flag(lib):
    p = _lib.Params(*([ONE] * 10))
    g = _lib.Grads(*([NULL] + [ONE] * 11))
    for fl in (0, NIG, SP | NIG):
        d = PT.desc(T=1, B=4, flags=fl)
        assert lib.fastgrnn_hip_backward(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, C.byref(g), NULL, 0,
                                         NULL) == 1


def test_zero_extended_route_passes_null_dx_through_with_the_flag(lib):
    for fl, want in ((SP | ZE, 0), (SP | ZE | NIG, 1)):
        d = PT.desc(H=100, flags=fl)
        plan = _lib.ZextPlan()
        assert lib.fastgrnn_hip_zero_extend_plan(C.byref(d), C.byref(plan)) == 0
        assert (plan.backward, plan.Hp, plan.Fp, plan.dx_optional) == (1, 128, 32, want)
        assert _backward_without_dx(lib, d) == (5 if want else 1)
    # padded shapes that already skip d_x (H = 256; H = 128 with Fp = 128) report it either way
    for kw in (dict(H=200), dict(F=100, H=100)):
        for fl in (SP | ZE, SP | ZE | NIG):
            plan = _lib.ZextPlan()
            assert lib.fastgrnn_hip_zero_extend_plan(C.byref(PT.desc(flags=fl, **kw)), C.byref(plan)) == 0
            assert plan.dx_optional == 1, kw


def _answers(lib, d):
    plan = _lib.ZextPlan()
    st = lib.fastgrnn_hip_zero_extend_plan(C.byref(d), C.byref(plan))
    bn = (lib.fastgrnn_hip_bn_train_supported(C.byref(d)), lib.fastgrnn_hip_bn_train_forward_workspace_bytes(C.byref(d)),
          lib.fastgrnn_hip_bn_train_backward_workspace_bytes(C.byref(d)))
    full = _lib.Plan()
    st_full = lib.fastgrnn_hip_plan(C.byref(d), C.byref(full))
    zx = full.zext
    new = (st_full, tuple(full.path), tuple(full.workspace_bytes), full.forward_ws_optional, full.rank_space_cols,
           zx.forward, zx.backward, zx.Hp, zx.Fp, zx.saved_bytes)
    return (lib.fastgrnn_hip_kernel_path(C.byref(d), 0), lib.fastgrnn_hip_kernel_path(C.byref(d), 1),
            lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)), lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)),
            st, plan.forward, plan.backward, plan.Hp, plan.Fp, plan.saved_bytes) + bn + new


def test_every_query_and_predicate_answers_the_same_with_the_flag(lib):
    n = 0
    for d in PT.grid():
        dn = _lib.Desc(d.T, d.B, d.F, d.H, d.w_rank, d.u_rank, d.gate_nl, d.update_nl, d.dtype, d.flags | NIG)
        assert _answers(lib, dn) == _answers(lib, d), (d.F, d.H, d.w_rank, d.gate_nl, d.update_nl, d.dtype, d.flags)
        n += 1
    assert n > 5000


def test_forward_entry_points_ignore_the_flag(lib):
    """the same status with and without the flag, for calls that stop at an argument or workspace check"""
    p = _lib.Params(*([ONE] * 10))
    for kw in (dict(), dict(flags=SP), dict(H=100, flags=SP | ZE), dict(flags=_lib.FLAG_HS_LAST), dict(H=64),
               dict(flags=_lib.FLAG_BN_TRAIN), dict(flags=_lib.FLAG_PREACT_AFFINE)):
        for ws in (0, 256):
            res = []
            for extra in (0, NIG):
                k = dict(kw)
                k["flags"] = k.get("flags", 0) | extra
                d = PT.desc(B=4096, **k)
                res.append((lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, NULL, ONE, ws,
                                                            NULL),
                            lib.fastgrnn_hip_forward_unroll_affine(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE,
                                                                   ws, NULL)))
                d1 = PT.desc(T=1, B=4096, **k)
                res[-1] += (lib.fastgrnn_hip_forward(C.byref(d1), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE, ws, NULL),)
            assert res[0] == res[1], (kw, ws, res)
            assert all(s != 0 for s in res[0])          # nothing was launched


def test_bn_train_entry_points_ignore_the_flag(lib):
    p = _lib.Params(*([ONE] * 10))
    bn = _lib.BnParams()
    for kw in (dict(flags=_lib.FLAG_BN_TRAIN), dict(flags=_lib.FLAG_BN_TRAIN | _lib.FLAG_BATCH_MAJOR), dict()):
        res = []
        for extra in (0, NIG):
            k = dict(kw)
            k["flags"] = k.get("flags", 0) | extra
            d = PT.desc(B=4096, **k)
            res.append((lib.fastgrnn_hip_bn_train_supported(C.byref(d)),
                        lib.fastgrnn_hip_bn_train_forward(C.byref(d), C.byref(p), C.byref(bn), ONE, ONE, ONE, ONE, ONE,
                                                          NULL, 0, NULL)))
        assert res[0] == res[1], (kw, res)


def test_the_flag_is_part_of_the_cached_plan_key():
    """calls with and without the input's gradient never share a descriptor; their paths and workspaces agree"""
    from kws_amd import fastgrnn_cuda
    a = fastgrnn_cuda._plan(99, 4096, 32, 128, 0, 0, 0, 2, _lib.F32, SP)
    b = fastgrnn_cuda._plan(99, 4096, 32, 128, 0, 0, 0, 2, _lib.F32, SP | NIG)
    assert a.desc.flags == SP and b.desc.flags == SP | NIG and a.path == b.path and a.ws == b.ws
    assert fastgrnn_cuda.kernel_path(99, 4096, 32, 128, flags=SP | NIG, direction=1) == 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_nodx_scans_pass_both_scanners_without_scratch(tmp_path):
    """the NODX instantiations of bwd_scan_split_w8 are among the kernels both scanners see, with no violating pair,
    no pending-LDS-write site and no scratch"""
    src = os.path.join(ROOT, "kws_amd", "csrc", "kernels_split.hip")
    asm = tmp_path / "kernels_split.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", str(asm),
                    src], check=True, capture_output=True, timeout=1500)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), str(asm),
                        "--only=bwd_scan_split_w8"], capture_output=True, text=True, timeout=900)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "total pairs: 0", r.stdout[-2000:] + r.stderr[-2000:]
    nodx = re.compile(r"bwd_scan_split_w8ILi\dE(?:Lb[01]E){5}Lb1E")
    seen = [l for l in lines if nodx.search(l)]
    assert len(seen) == 48, seen[:4]                           # 6 gates x {quantTanh, bf16, PREACT, pair} x {ragged, full}
    for l in seen:
        assert int(l.split(" mfma ")[1].split()[0]) > 0 and int(l.split("pairs")[1].split()[0]) == 0, l
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), str(asm), "--strict"],
                        capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0 and r2.stdout.strip().splitlines()[-1] == "sites in loops: 0", r2.stdout[-2000:]
    text = asm.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)
    nk = [(name, body) for name, body in kernels if nodx.search(name)]
    assert len(nk) == 48
    for name, body in nk:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
    for name, _ in nk:
        start = text.index("\n" + name + ":")
        end = text.index(".Lfunc_end", start)
        assert "scratch_" not in text[start:end], name
