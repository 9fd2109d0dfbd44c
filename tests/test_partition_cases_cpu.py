"""The case table of tests/partition_cases.py covers every partition class it names, and its Python restatement of the
TN GEMM's chunk rule agrees with the library: the backward workspace of the dense H=256 / F=32 layer holds the GEMM's
partials, so its size follows the chunk count.  No kernel is launched here."""
import ctypes as C

import pytest

from kws_amd import _lib
from tests import partition_cases as PC
from tests import support as S

SLOT = 2 * 128 * 256 * 4          # one partial of dU = d_pre^T . H_prev at M = N = 256 (nblk = 2): 262 144 bytes


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


def test_table_covers_every_class():
    assert PC.missing() == [], PC.missing()
    cov = PC.coverage()
    assert set(cov) == set(PC.CLASSES)
    for T, B in PC.SHAPES:
        assert T * B <= PC.MAX_ROWS and PC.classes_of(T, B), (T, B)
    # a table without its multi-stage shapes is found wanting (the coverage is computed, not written down)
    small = [(T, B) for T, B in PC.SHAPES if PC.rows_gemm_cut(T * B).spw == 1]
    assert small and "rows chunks of 2" in PC.missing(small) and "tn2 chunks of 5, last full" in PC.missing(small)


def test_cut_arithmetic_on_known_shapes():
    """the launchers' integer arithmetic by hand, at the sizes the suite ran before this table and at three of its rows"""
    assert PC.rows_gemm_cut(99 * 4096) == PC.Cut(12672, 50, 254, 22, 2)
    assert PC.tn_cut(99 * 4096, 1) == PC.Cut(12672, 50, 254, 22, 2)
    assert PC.tn_cut(99 * 4096, 2) == PC.Cut(12672, 99, 128, 99, 0)
    assert PC.rows_gemm_cut(99 * 64) == PC.Cut(198, 1, 198, 1, 0) and PC.tn_cut(99 * 64, 2) == PC.Cut(198, 2, 99, 2, 5)
    assert PC.rows_gemm_cut(8193) == PC.Cut(257, 2, 129, 1, 127) and PC.tn_cut(8193, 1).idle == 7
    assert PC.tn_cut(8193, 2) == PC.Cut(257, 3, 86, 2, 2)
    assert PC.tn_cut(16489, 2) == PC.Cut(516, 5, 104, 1, 0) and PC.rows_gemm_cut(16489).last == 3
    assert PC.slab_rounds(257, 128) == (3, 1) and PC.slab_rounds(129, 64) == (3, 1) and PC.slab_rounds(128, 128) == (1, 128)
    for T, B in PC.SHAPES:
        bs = PC.seam_utterances(T, B)
        assert bs[0] == 0 and bs[-1] == B - 1 and 2 <= len(bs) <= 14 and len(set(bs)) == len(bs)


def _bwd_ws(lib, T, B, dtype=_lib.F32):
    d = _lib.Desc(T=T, B=B, F=32, H=256, w_rank=0, u_rank=0, gate_nl=0, update_nl=2, dtype=dtype,
                  flags=_lib.FLAG_SAVE_PREACT)
    assert lib.fastgrnn_hip_kernel_path(C.byref(d), 1) == 2
    return int(lib.fastgrnn_hip_backward_workspace_bytes(C.byref(d)))


SWEEP = PC.SHAPES + [(99, 4096), (99, 64), (31, 37), (3, 1377), (3, 1381), (5, 900), (7, 601), (96, 86), (99, 2500)]


@pytest.mark.parametrize("T,B", SWEEP, ids=lambda v: str(v))
def test_tn_chunk_rule_matches_the_workspace_the_library_asks_for(lib, T, B):
    """dpre_bwd_ws (kws_amd/csrc/kernels_gemm.hip), the H = 256 backward's layout: the slabs depend on B alone, d_pre is (T*B + 16) * 1024 bytes, the
    TN partials are 2 * nch * SLOT bytes (tn_gemm_big_ws): at fixed B the workspace grows from T = 1 by exactly
    1024 * B * dT + 2 * SLOT * dnch."""
    assert B < (1 << 21)
    grow = _bwd_ws(lib, T, B) - _bwd_ws(lib, 1, B)
    assert grow == 1024 * B * (T - 1) + 2 * SLOT * (PC.tn_cut(T * B, 2).nchunk - PC.tn_cut(B, 2).nchunk), (T, B)


@pytest.mark.parametrize("T,B", SWEEP, ids=lambda v: str(v))
def test_bf16_head_and_body_partials_fit_the_workspace(lib, T, B):
    """With bf16 sequences tn_gemm_big_run cuts dU into an fp32 head over the B rows of h0 and a bf16 body over the
    rest, each into chunks of its own; together they can be more than twice the chunks of the whole product ((3, 1377):
    87 + 44 against 2 * 65), and every one of them is written."""
    body, head = PC.tn_partials(T * B, 2, shift=B, bf16=True)
    # the anchor: at T = 1 every row pairs with h0, the product is not split (tn_partials: head 0)
    assert PC.tn_partials(B, 2, shift=B, bf16=True) == (PC.tn_cut(B, 2).nchunk, 0)
    slab_bytes = _bwd_ws(lib, 1, B, _lib.BF16_IO) - (B + 16) * 1024 - PC.tn_slots(B, 2) * SLOT
    assert slab_bytes == _bwd_ws(lib, 1, B) - (B + 16) * 1024 - PC.tn_slots(B, 2) * SLOT and slab_bytes > 0
    room = _bwd_ws(lib, T, B, _lib.BF16_IO) - slab_bytes - (T * B + 16) * 1024
    assert room % SLOT == 0
    assert room // SLOT == max(PC.tn_slots(T * B, 2), body + head), (T, B, room // SLOT, body, head)


def test_bf16_partials_fit_at_every_batch_of_an_epoch(lib):
    """every B an epoch's last minibatch can have, at the workload's T and at T = 3 (where most misfits were)"""
    for T in (3, 99):
        for B in range(1, 4097):
            body, head = PC.tn_partials(T * B, 2, shift=B, bf16=True)
            room = _bwd_ws(lib, T, B, _lib.BF16_IO) - _bwd_ws(lib, 1, B, _lib.BF16_IO) - 1024 * B * (T - 1)
            assert room // SLOT + PC.tn_slots(B, 2) >= body + head, (T, B)
