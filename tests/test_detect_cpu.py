"""CPU-side checks of the inference tail (fastgrnn_hip_head_predict, fastgrnn_hip_vote_windows): argument validation
without a launch, in the style of tests/test_abi_cpu.py, and the plain-Python vote the GPU tests compare against, held
to cases whose expected outputs are typed out in tests/detect_cases.py."""
import collections
import ctypes as C
import os
import re

import pytest

from tests import detect_cases as D
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = C.c_void_p(None), C.c_void_p(256)          # (a fake non-NULL, 256-byte aligned pointer: nothing is launched)
OK, NULLP, SHAPE, WS, UNSUP = 0, 1, 2, 5, 7


@pytest.fixture(scope="module")
def lib():
    return support.built_library()


def _predict(lib, B=37, H=128, Cn=12, h=ONE, w=ONE, b=ONE, labels=ONE, logp=ONE, pred=ONE, n=ONE, ws=ONE, nbytes=None):
    if nbytes is None:
        nbytes = lib.fastgrnn_hip_head_predict_workspace_bytes(B, H, Cn)
    return lib.fastgrnn_hip_head_predict(B, H, Cn, h, w, b, labels, logp, pred, n, ws, nbytes, NULL)


def _vote(lib, S=3, Nw=11, K=10, M=5, pred=ONE, maj=ONE, ev=ONE):
    return lib.fastgrnn_hip_vote_windows(S, Nw, K, M, pred, maj, ev, NULL)


def test_head_predict_refuses_missing_pointers(lib):
    for name in ("h", "w", "b", "pred"):
        assert _predict(lib, **{name: NULL}) == NULLP, name
    assert _predict(lib, n=NULL) == NULLP                       # labels without n_correct
    # log_probs is optional: every error precedes a launch, so a call that passes the pointer checks is shown by the
    # NEXT refusal in line, the workspace's.  (Without labels nothing is left to refuse -- no workspace is needed -- and
    # the call would launch: tests/test_hip_detect.py makes it, through the shim, with a NULL workspace.)
    assert _predict(lib, logp=NULL, nbytes=0) == WS


def test_head_predict_refuses_bad_and_unsupported_shapes(lib):
    for kw in (dict(B=0), dict(H=0), dict(Cn=0), dict(B=-3)):
        assert _predict(lib, nbytes=1 << 20, **kw) == SHAPE, kw
    assert _predict(lib, Cn=65, nbytes=1 << 20) == UNSUP
    assert _predict(lib, H=257, nbytes=1 << 20) == UNSUP
    assert _predict(lib, H=256, Cn=64, nbytes=0) == WS            # the largest head is supported
    assert _predict(lib, B=0, h=NULL) == SHAPE                     # (the order of the checks: shape, then pointers)
    assert _predict(lib, Cn=65, h=NULL) == UNSUP


def test_head_predict_workspace(lib):
    q = lib.fastgrnn_hip_head_predict_workspace_bytes
    need = q(37, 128, 12)
    assert need >= 3 * 4 and need % 256 == 0                       # one int32 per workgroup of 16 utterances (with labels)
    assert _predict(lib, ws=NULL) == WS
    assert _predict(lib, nbytes=need - 1) == WS
    assert _predict(lib, ws=C.c_void_p(256 + 64)) == WS            # misaligned
    sizes = [q(B, 128, 12) for B in (1, 16, 17, 1024, 1025, 4096, 4097, 1 << 20, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0                 # monotone in B
    assert sizes[-1] >= ((1 << 31) // 16) * 4
    assert q(4097, 128, 12) >= 257 * 4
    assert q(0, 128, 12) == 0 and q(4, 257, 12) == 0 and q(4, 128, 65) == 0


def test_vote_windows_argument_checks(lib):
    for name in ("pred", "maj", "ev"):
        assert _vote(lib, **{name: NULL}) == NULLP, name
    for kw in (dict(S=0), dict(Nw=0), dict(K=0, M=0), dict(M=0), dict(S=-1), dict(K=-2, M=-2)):
        assert _vote(lib, **kw) == SHAPE, kw
    assert _vote(lib, K=10, M=11) == SHAPE                         # M > K
    assert _vote(lib, K=65, M=33) == UNSUP
    assert _vote(lib, K=65, M=66) == SHAPE
    assert _vote(lib, S=(1 << 31) - 1, Nw=(1 << 31) - 1) == SHAPE  # S * Nw beyond the library's size limit
    assert _vote(lib, K=65, M=33, pred=NULL) == UNSUP              # (the order of the checks)


@pytest.mark.parametrize("case", D.TYPED_CASES, ids=[c[0] for c in D.TYPED_CASES])
def test_vote_reference_on_typed_out_cases(case):
    _, pred, K, M, majority, event = case
    assert D.vote_reference(pred, K, M) == (majority, event)


def test_vote_reference_tie_rule_and_slots():
    """The statements of the issue, each read off the typed-out cases."""
    by = {c[0]: c for c in D.TYPED_CASES}
    A, B = D.A_, D.B_
    assert by["tie_5_5_A_first"][1] == [A, B, A, B, A, B, A, B, A, B] and by["tie_5_5_A_first"][4][9] == A
    assert by["tie_5_5_B_first"][1] == [B, A, B, A, B, A, B, A, B, A] and by["tie_5_5_B_first"][4][9] == B
    assert by["tie_5_5_shifted"][4][10] == B                        # the list at the eleventh window starts with B
    assert by["event_once"][5].count(4) == 1
    assert all(m == -1 for m in by["needs_M_votes"][4][:4])


def test_seeded_vote_cases_cover_what_they_claim():
    src = open(os.path.join(ROOT, "kws_amd", "csrc", "kernels_head.hip")).read()
    assert int(re.search(r"constexpr int VOTE_CHUNK = (\d+)", src).group(1)) == D.VOTE_CHUNK   # the cases cross THIS chunk
    for name in ("chunk_plus_1", "two_chunks_plus_3"):
        p, K, M = D.vote_case(name)
        assert p.shape[1] == (D.VOTE_CHUNK + 1 if name == "chunk_plus_1" else 2 * D.VOTE_CHUNK + 3)
        maj, ev = D.vote_reference_streams(p.tolist(), K, M)
        for edge in range(D.VOTE_CHUNK, p.shape[1], D.VOTE_CHUNK):
            # a run of majorities, none at the chunk's last window, the same majority again at the next chunk's first
            assert all(m == 1 for m in maj[0][edge - 40:edge - 1]) and maj[0][edge - 1] == -1
            assert maj[0][edge] == 1 and ev[0][edge] == -1          # previous = 1 is carried: no event
            assert maj[1][edge - 1] == -1 and maj[1][edge] == 2 and ev[1][edge] == 2
    p, K, M = D.vote_case("leak")
    maj, _ = D.vote_reference_streams(p.tolist(), K, M)
    assert maj[0][-1] == 2 and maj[1][:4] == [-1] * 4               # four votes are no majority of five
    p, K, M = D.vote_case("k64")
    assert int((p < 0).sum()) > 0 and sorted(set(p[p >= 0].tolist())) == [0, 1, 2]


def _top_frequency(row, K):
    """the largest frequency of a non-negative value in each window's vote list"""
    out = []
    for w in range(len(row)):
        c = collections.Counter(v for v in row[max(0, w - K + 1):w + 1] if v >= 0)
        out.append(max(c.values()) if c else 0)
    return out


def test_the_large_K_cases_have_majorities_changes_and_ties():
    """K = 64: the expected outputs are not constant, so an under-count, a wrong list start or a broken tie rule at 63
    predecessors shows."""
    p, K, M = D.vote_case("k64")
    assert (K, M, p.shape[1]) == (64, 33, 200)
    maj, ev = D.vote_reference_streams(p.tolist(), K, M)
    # stream 0: a majority while the list is still filling, none for a while, another one with the list full
    assert any(m == 1 for m in maj[0][:64]) and any(m == 2 for m in maj[0][64:]) and -1 in maj[0][64:]
    assert [e for e in ev[0] if e >= 0] == [1, 2]
    # stream 1: 32 votes are not 33 -- nothing up to window 63 -- then 1, a lapse, then 0
    f = _top_frequency(p[1].tolist(), K)
    assert f[63] == 32 and all(m == -1 for m in maj[1][:64]) and f.count(M - 1) >= 2 and f.count(M) >= 2
    assert [e for e in ev[1] if e >= 0] == [1, 0]
    first = maj[1].index(1)
    assert first > 64 and f[first] == M and f[first - 1] == M - 1          # the threshold itself
    p, K, M = D.vote_case("k64_ties")
    maj, ev = D.vote_reference_streams(p.tolist(), K, M)
    # 32:32 from window 63 to 99, the older value alternating: 1 at odd windows' lists starting with 1, else 2
    assert maj[0][63:100] == [1 if w % 2 else 2 for w in range(63, 100)]
    assert maj[0][62] == 1 and ev[0][62] == 1                               # (32 of 63 votes: the first report)
    assert ev[0][64:100] == maj[0][64:100]                                   # then every window reports the other keyword


@pytest.mark.parametrize("name", D.VOTE_CASES)
def test_seeded_vote_cases_expect_something(name):
    """Every seeded case but the ones too short for five votes has majorities and events to get right."""
    p, K, M = D.vote_case(name)
    maj, ev = D.vote_reference_streams(p.tolist(), K, M)
    some_maj = sum(m >= 0 for row in maj for m in row)
    some_ev = sum(e >= 0 for row in ev for e in row)
    if name in ("nw1", "nw4"):                                   # fewer windows than M = 5 votes: -1 by design
        assert some_maj == 0 and some_ev == 0
    else:
        assert some_maj > 0 and some_ev > 0 and some_maj < p.numel(), (some_maj, some_ev)


@pytest.mark.parametrize("B,H,Cn", D.HEAD_SHAPES)
def test_head_seeds_excuse_no_row(B, H, Cn):
    """The seeds of the head cases leave every row's fp64 top-two gap above the bound: the GPU test may excuse rows
    below it, and with these operands there are none to excuse."""
    c = D.head_case(B, H, Cn)
    assert int(c["excused"].sum()) == 0
    assert int((c["y"] == -100).sum()) >= 1
    if B > 1:
        assert 0 < int((c["y"] == c["argmax64"]).sum()) < B
