"""The case table of tests/h0_range_cases.py: every case's descriptor answers kernel path 2 in the direction it is run
(with FLAG_FWD_BF16X3 as well where the case compares with that run), the windowed cases are held by the windowed entry
points, and the table covers the axes each family has to.  fastgrnn_hip_kernel_path is a pure function of the descriptor:
no kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

from kws_amd import _lib
from tests import h0_range_cases as HC
from tests import support as S


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def _of(family):
    return [c for c in HC.CONFIGS if c.family == family]


@pytest.mark.parametrize("case", HC.ALL_CASES, ids=HC.case_id)
def test_every_case_runs_on_kernel_path_2(lib, case):
    c = case.cfg
    extras = [0] + ([_lib.FLAG_FWD_BF16X3] if c.ref == "x3" else [])
    if c.entry in ("windows", "train_windows"):
        # what the gathered comparison calls: forward_unroll / forward_unroll_affine with the same flags
        extras = [0] if c.entry == "windows" else [_lib.FLAG_SAVE_PREACT]
        d = HC.descriptor(case)
        query = lib.fastgrnn_hip_windows_supported if c.entry == "windows" else lib.fastgrnn_hip_train_windows_supported
        assert query(C.byref(d)) == 1
    for extra in extras:
        d = HC.descriptor(case, extra)
        for direction in HC.directions(case):
            assert lib.fastgrnn_hip_kernel_path(C.byref(d), direction) == 2, (HC.case_id(case), hex(d.flags), direction)
    if c.zext:                                             # the padded route, not a shape that is on path 2 anyway
        plan = _lib.Plan()
        assert lib.fastgrnn_hip_plan(C.byref(HC.descriptor(case)), C.byref(plan)) == 0
        assert plan.zext.forward == 1 and (plan.zext.Hp, plan.zext.Fp) == ((128, 32) if c.H == 100 else (256, 64))


def test_case_ids_are_unique_and_the_shapes_are_the_small_ones():
    ids = [HC.case_id(c) for c in HC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert HC.B == 37 and HC.T_DEFAULT == 5
    assert {c.T for c in HC.ALL_CASES} == {1, 2, 5}


def test_every_configuration_runs_ragged_tile_and_every_corner():
    for c in HC.CONFIGS:
        pats = {k.pattern for k in HC.CASES if k.cfg == c and k.T == HC.T_DEFAULT}
        assert set(HC.BASIC) <= pats, (c, pats)
    for fam in "ABCDEFGH":
        assert _of(fam), fam


def test_extra_patterns_run_once_per_kernel_file_and_under_prein():
    for H, F in ((128, 32), (256, 32), (256, 64)):
        pats = {k.pattern for k in HC.CASES if (k.cfg.H, k.cfg.F, k.cfg.entry) == (H, F, "unroll") and not k.cfg.bf16}
        assert set(HC.EXTRA) <= pats, (H, F)
    for H in (128, 256):                                   # what NaN means in a bf16 hs
        assert any(k.pattern == "nonfinite_nan" and k.cfg.bf16 and k.cfg.H == H for k in HC.CASES)
    for fam in "ABCDEFG":                                  # T = 1 and T = 2: one per kernel family and entry point
        assert {k.T for k in HC.CASES if k.cfg.family == fam} == {1, 2, 5}, fam


def test_family_axes():
    A = _of("A")
    assert {(c.H, c.F) for c in A} == {(128, 32)}
    assert {c.contract for c in A} == {"hs", "gates", "preact", "last"}
    assert {c.layout for c in A} == {"tm", "bm", "bft"} and {c.bf16 for c in A} == {False, True}
    assert {c.gate for c in A} == set(HC.BOUNDED_GATES)
    assert {c.contract for c in A if c.update == "quantTanh"} == {"hs", "preact"}
    Bf = _of("B")
    assert {(c.H, c.F) for c in Bf} == {(128, 64), (128, 256)}
    assert {c.contract for c in Bf if not c.bf16} == {"hs", "gates", "preact", "last"}
    assert any(c.layout == "bft" for c in Bf) and any(c.bf16 and c.gate == "sigmoid" for c in Bf)
    Cf = _of("C")
    assert {(c.H, c.F) for c in Cf} == {(256, 32)}
    assert {c.contract for c in Cf if not c.bf16} == {"hs", "gates", "preact", "last"}
    assert {c.layout for c in Cf} == {"tm", "bm", "bft"}
    assert {c.contract for c in Cf if c.bf16} == {"hs", "preact"}
    assert {c.gate for c in Cf} == set(HC.BOUNDED_GATES)
    D = _of("D")
    assert {(c.H, c.F) for c in D} == {(256, 64), (256, 128)}
    assert any(c.layout == "bft" for c in D) and any(c.bf16 for c in D)
    E = _of("E")
    assert {(c.H, c.F) for c in E} == {(128, 32), (128, 256), (256, 32), (256, 64)}
    for shape in {(c.H, c.F) for c in E}:
        assert {c.contract for c in E if (c.H, c.F) == shape} == {"hs", "last"}
    assert all(c.affine and c.gate == "sigmoid" for c in E)
    Ff = _of("F")
    assert {(c.H, c.F, c.affine, c.contract, c.layout) for c in Ff} == {
        (H, F, a, k, l) for H, F in ((128, 32), (256, 32), (256, 64)) for a in (False, True)
        for k, l in (("hs", "tm"), ("hs", "bm"), ("last", "tm"))}
    assert {(c.H, c.F) for c in _of("G")} == {(128, 32), (256, 32), (256, 64)}
    Hf = _of("H")
    assert {(c.H, c.F, c.rw, c.ru, c.zext) for c in Hf} == {(128, 32, 8, 8, False), (256, 32, 32, 32, False),
                                                            (100, 32, 0, 0, True), (200, 40, 0, 0, True)}
    assert (HC.CONTROL.H, HC.CONTROL.F, HC.CONTROL.rw, HC.CONTROL.ru) == (256, 32, 16, 16)
    assert {(c.H, c.F) for c in HC.BACKWARD} == {(128, 32), (256, 32), (128, 256)}
    assert (HC.MODULE.H, HC.MODULE.F) == (256, 32)


def test_patterns_are_what_they_say():
    for H in (100, 128, 200, 256):
        for name in HC.PATTERNS:
            h0, rows, falls = HC.h0_pattern(name, H)
            assert h0.shape == (HC.B, H) and h0.dtype == np.float32
            rest = np.delete(h0, rows, axis=0)
            assert np.isfinite(rest).all() and np.abs(rest).max() < 3.0            # inside fp16's range by far
            top = np.abs(h0[rows])
            if name.startswith("nonfinite"):
                lone = name == "nonfinite_nan_element"
                assert rows == [HC.NONFINITE_ROW] and int((~np.isfinite(h0[rows])).sum()) == (1 if lone else H)
                assert falls == (not lone or H > 128)          # (H=128: a lone NaN does not reach the device-side maximum)
            elif name.startswith("threshold"):
                m = np.float32(top.max())
                assert (m + np.float32(HC.T_DEFAULT) + np.float32(2.0) < np.float32(3.0e4)) == (not falls)
                assert float(m) in (29992.0, 29993.0) and (h0[rows] < -2e4).sum() == 1   # negative: the fabsf
            else:
                assert falls and top.max() >= 0.5 * HC.SCALE
                if name in ("ragged_tile", "middle_tile"):                          # both signs: the fabsf
                    assert (h0[rows] < -1e4).any() and (h0[rows] > 1e4).any()
        assert HC.tiles_of(HC.h0_pattern("ragged_tile", H)[1]) == [2]
        assert HC.tiles_of(HC.h0_pattern("middle_tile", H)[1]) == [1]
        for name, (b, n) in HC.CORNERS.items():
            h0, rows, _ = HC.h0_pattern(name, H)
            big = np.argwhere(np.abs(h0) > 1e4)
            assert big.tolist() == [[b, H // 2 if n is None else n % H]] and rows == [b]
    signs = {float(np.sign(HC.h0_pattern(name, 128)[0][b, n if n is not None else 64])) for name, (b, n) in HC.CORNERS.items()}
    assert signs == {-1.0, 1.0}


@pytest.mark.parametrize("H,F", [(c.H, c.F) for c in HC.BACKWARD])
def test_fp32_oracle_stays_within_the_backward_bound_for_the_chosen_seed(H, F):
    """Family J holds the kernels to the fuzz file's bound, whose last term is four times the fp32 oracle's own error:
    for the seeds of this table that error alone sits inside the rest of the expression, so the term does not carry
    the bound."""
    g_o, g_32, gscale = HC.backward_reference(H, F)
    assert float(np.abs(g_o["d_u"]).max()) > 1e4                                   # hs of order 1e5 reached the dU product
    for k, v in g_o.items():
        if k.startswith("_"):
            continue
        err = float(np.abs(g_32[k].reshape(v.shape) - v).max())
        lim = HC.gradient_limit(k, g_o, g_32, gscale, oracle_term=False)
        print("H=%d F=%d %s: fp32 oracle error %.3g, bound without the oracle term %.3g" % (H, F, k, err, lim))
        assert err <= lim, (k, err, lim)
