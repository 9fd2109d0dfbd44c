"""CPU-side checks of tests/generic_cases.py, the cases of the generic scans (kernel path 0):

  * the two references of the 72 nonlinearity-pair cases -- the numpy oracle's hand-written backward and torch autograd
    through the torch CPU port -- agree to 1e-12, so the GPU tests may hold the kernel to either;
  * no argument of a piecewise-linear nonlinearity of any case lies within 1e-6 of a kink, so an fp64 kernel takes the
    oracle's side of every derivative jump;
  * the library asks for at least the workspace the generic backward and forward store into, ranks above H included;
  * a direction whose scan does not fit the LDS is refused (status 7) before the workspace check -- before anything
    could be launched -- and the plan reports it as it reports a direction no unrolled call runs; a direction that fits
    reaches the workspace check (status 5).  No kernel is launched: every pointer is a dummy and no workspace is given,
    as in tests/test_plan_cpu.py.
"""
import ctypes as C
import itertools

import pytest

from kws_amd import _lib
from tests import generic_cases as GC
from tests import support as S

GEN = _lib.FLAG_FORCE_GENERIC
ONE = C.c_void_p(256)
NULL = C.c_void_p(None)
OK, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 5, 7
DT = {"f32": _lib.F32, "f64": _lib.F64}


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def _desc(T, B, F, H, rw, ru, dtype, flags=GEN, gate=0, update=2):
    return _lib.Desc(T, B, F, H, rw, ru, gate, update, dtype, flags)


def _plan(lib, d):
    p = _lib.Plan()
    assert lib.fastgrnn_hip_plan(C.byref(d), C.byref(p)) == OK
    return p


def _forward(lib, d):
    """status of forward_unroll with every pointer given and no workspace"""
    p = _lib.Params(*([ONE] * 10))
    return lib.fastgrnn_hip_forward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, NULL, 0, NULL)


def _backward(lib, d):
    p = _lib.Params(*([ONE] * 10))
    g = _lib.Grads(*([ONE] * 12))
    return lib.fastgrnn_hip_backward_unroll(C.byref(d), C.byref(p), ONE, ONE, ONE, ONE, ONE, ONE, C.byref(g), NULL, 0,
                                            NULL)


def test_the_table_holds_what_it_is_there_for():
    names = {c.name for c in GC.TABLE}
    assert len(names) == len(GC.TABLE)
    hs = {(c.H, c.dtype) for c in GC.TABLE}
    assert all((H, dt) in hs for H in (63, 65, 130, 257, 300, 520) for dt in ("f32", "f64"))
    # the largest fp64 H that both directions admit at F = 1 is the backward's limit; the forward goes further
    H = GC.H_BOTH_FIT_F64
    assert (H, "f64") in hs and GC.largest_h(1, 1, 0, 0, GC.F64) == H < GC.largest_h(0, 1, 0, 0, GC.F64)
    seam = GC.ROWS_TILED_MAX_N                      # 64: the last N of the tiled row GEMM
    assert {c.F for c in GC.TABLE if c.H == 24} >= {1, seam, seam + 1, 300}
    assert {c.rw for c in GC.TABLE if (c.F, c.H) == (80, 72)} >= {1, seam, seam + 1}
    assert {c.ru for c in GC.TABLE if c.H == 72} >= {1, seam, seam + 1}
    assert {(c.F, c.rw, c.ru) for c in GC.TABLE if c.H == 8} == {(32, 16, 0), (13, 0, 20), (32, 16, 20)}
    assert {c.T * c.B for c in GC.TABLE} >= {2047, 2048, 2049, 4096}
    assert {c.B for c in GC.TABLE if c.T == 2} >= {7, 8, 9}
    assert all((c.T <= 6 and c.B <= 20) or c.T * c.B >= 2047 for c in GC.TABLE)
    # LDS above 64 KiB is in the table, in both directions
    assert any(GC.lds_bytes(c, 0) > 65536 for c in GC.TABLE) and any(GC.lds_bytes(c, 1) > 65536 for c in GC.TABLE)
    assert all(GC.lds_fits(c, 0) and GC.lds_fits(c, 1) for c in GC.TABLE + GC.PAIRS + GC.PAIRS_F32)
    assert len(GC.PAIRS) == 72 and len({(c.gate, c.update, c.rw) for c in GC.PAIRS}) == 72
    assert len(GC.PAIRS_F32) == 12 and {c.update for c in GC.PAIRS_F32} == set(GC.NAMES)


def test_oracle_and_port_autograd_agree_on_every_pair():
    worst = ("", 0.0)
    for c in GC.PAIRS:
        b = GC.build(c.name, True)
        errs = {"hs": GC.rel_err(b.port_hs, b.hs)}
        names = GC.grad_names(b.grads)
        assert sorted(names) == sorted(b.port_grads), c.name
        errs.update({k: GC.rel_err(b.port_grads[k], b.grads[k]) for k in names})
        k = max(errs, key=errs.get)
        assert errs[k] <= 1e-12, (c.name, k, errs[k])
        worst = max(worst, (c.name + ":" + k, errs[k]), key=lambda w: w[1])
    print("oracle against port, worst of 72 cases: %s %.3g" % worst)


def test_no_case_sits_on_a_kink():
    checked = 0
    for c in GC.TABLE + GC.PAIRS + GC.PAIRS_F32:
        if c.gate not in GC.KINKS and c.update not in GC.KINKS:
            continue
        p, x, h0, _ = GC.operands(c)
        dist, _ = GC.kink_distance(p, x, h0, c.gate, c.update)
        assert dist >= GC.KINK_MARGIN, (c.name, dist)
        checked += 1
    assert checked >= 64 + 10           # 32 of the 36 pairs have a piecewise-linear member, twice; 10 of the 12 in fp32


def _grid():
    """(F, H, rw, ru) with every rank from 0 to 2 * max(H, F) in a few steps"""
    for F, H in ((32, 8), (13, 8), (8, 32), (24, 24), (80, 72), (13, 300)):
        m = max(F, H)
        ranks = sorted({0, 1, min(F, H), min(F, H) + 1, m, m + 1, 2 * m})
        for rw, ru in itertools.product(ranks, ranks):
            yield F, H, rw, ru


def test_library_workspaces_cover_what_the_generic_scans_store(lib):
    descs = [_desc(c.T, c.B, c.F, c.H, c.rw, c.ru, DT[c.dtype]) for c in GC.TABLE + GC.PAIRS[:2]]
    descs += [_desc(T, B, F, H, rw, ru, dt) for (F, H, rw, ru) in _grid() for (T, B) in ((3, 5), (2, 2049))
              for dt in (_lib.F32, _lib.F64)]
    short = []
    for d in descs:
        assert lib.fastgrnn_hip_kernel_path(C.byref(d), 0) == 0 and lib.fastgrnn_hip_kernel_path(C.byref(d), 1) == 0
        what = (d.T, d.B, d.F, d.H, d.w_rank, d.u_rank, d.dtype)
        have, need = lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)), GC.backward_workspace_need(d)
        if have < need:
            short.append(("backward",) + what + (have, need))
        have, need = lib.fastgrnn_hip_forward_workspace_bytes(C.byref(d)), GC.forward_workspace_need(d)
        if have < need:
            short.append(("forward",) + what + (have, need))
    assert not short, "%d of %d descriptors, the first: %s" % (len(short), len(descs), short[:4])
    assert len(descs) > 1000


def test_small_ranks_keep_their_backward_workspace(lib):
    """with ranks up to min(H, F) the split-K partials are those of H x max(H, F), as before ranks above H counted"""
    for F, H, rw, ru in ((32, 128, 8, 8), (13, 24, 4, 5), (32, 256, 16, 16), (64, 24, 24, 24), (13, 24, 0, 13)):
        for T, B, dt in ((3, 5, _lib.F32), (99, 4096, _lib.F32), (2, 2049, _lib.F64)):
            d = _desc(T, B, F, H, rw, ru, dt)
            es, TB, nwg, nsplit = (8 if dt else 4), T * B, -(-B // 8), -(-T * B // 2048)
            want = sum(-(-n * es // 256) * 256 for n in (TB * H, nwg * H, nwg * H, nwg * 2, TB * rw, TB * rw, TB * ru,
                                                          TB * ru, nsplit * H * max(H, F)))
            assert lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)) == want, (F, H, rw, ru, T, B, dt)


# (dtype, F, rw, ru) of the descriptors whose H walks over each direction's LDS limit
LDS_EDGES = [(dt, F, rw, ru) for dt in ("f32", "f64") for F, rw, ru in ((1, 0, 0), (32, 0, 0), (40, 16, 24), (13, 0, 70))]


@pytest.mark.parametrize("flags", [0, GEN], ids=["dispatch", "generic"])
@pytest.mark.parametrize("dt,F,rw,ru", LDS_EDGES, ids=["%s-F%d-r%d-%d" % e for e in LDS_EDGES])
def test_a_direction_outside_the_lds_is_refused_before_the_workspace_check(lib, dt, F, rw, ru, flags):
    calls = (_forward, _backward)
    edge = [GC.largest_h(direction, F, rw, ru, dt) for direction in (0, 1)]
    assert edge[1] < edge[0]                 # there are shapes whose forward fits and whose backward does not
    for H in sorted({edge[0], edge[0] + 1, edge[1], edge[1] + 1, 2 * edge[0]}):
        d = _desc(3, 9, F, H, rw, ru, DT[dt], flags)
        plan = _plan(lib, d)
        for direction in (0, 1):
            fits = H <= edge[direction]
            assert fits == GC.lds_fits(d, direction)
            what = (dt, F, H, rw, ru, direction, GC.lds_bytes(d, direction))
            if fits:
                assert plan.path[direction] == 0 and plan.workspace_bytes[direction] > 0, what
                assert calls[direction](lib, d) == ERR_WORKSPACE, what
            else:
                assert plan.path[direction] == -1 and plan.workspace_bytes[direction] == 0, what
                assert lib.fastgrnn_hip_kernel_path(C.byref(d), direction) == -1, what
                assert calls[direction](lib, d) == ERR_UNSUPPORTED, what


def test_the_fp64_edges_of_a_training_step(lib):
    """dense fp64 with F = 1: both directions up to H = 1109, the forward alone up to 1279 -- from the two carve-ups
    (16 H + 8 F and 18 H + 512 elements of 8 bytes against 160 KiB), not from the launchers"""
    assert (GC.largest_h(0, 1, 0, 0, "f64"), GC.largest_h(1, 1, 0, 0, "f64")) == (1279, 1109)
    for H, fwd, bwd in ((1109, ERR_WORKSPACE, ERR_WORKSPACE), (1110, ERR_WORKSPACE, ERR_UNSUPPORTED),
                        (1279, ERR_WORKSPACE, ERR_UNSUPPORTED), (1280, ERR_UNSUPPORTED, ERR_UNSUPPORTED)):
        d = _desc(2, 9, 1, H, 0, 0, _lib.F64, 0)
        assert (_forward(lib, d), _backward(lib, d)) == (fwd, bwd), H
