"""The route record (kws_amd._route) implies what the modules were recorded handing to the operator shim
(tests/golden/routes/parent.json, recorded on the GPU before the modules read a record): for every ``forward`` row the
signature is built from the case alone -- no tensors -- and the record must give the first forward call's entry point,
flags, presented shape and strides and ``want_gates``, the backward's flags and gradient shape, and the result's shape.
Plus the bounds of the two host caches."""
import json
import os

import pytest
import torch

from kws_amd import _lib, _route, fastgrnn_cuda
from kws_amd.rnn import NON_LINEARITY
from tests import route_cases as RC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routes", "parent.json")
with open(FIXTURE) as _f:
    RECORDED = json.load(_f)
CASES = {c["id"]: c for c in RC.cases()}
MODES = {"grad_x": _route.AUTOGRAD, "grad": _route.AUTOGRAD, "grad_last": _route.AUTOGRAD, "nograd": _route.NO_GRAD,
         "nograd_last": _route.NO_GRAD, "inference": _route.INFERENCE}


def _dense(shape):
    return [shape[1] * shape[2], shape[2], 1]


def signature(case):
    H, F, wRank, uRank, dtype, gate = RC.CELLS[case["cell"]]
    shape, strides = RC.input_meta(case)
    affine = case["cls"] != "FastGRNNCUDA"
    return _route.Signature(_route.AFFINE if affine else _route.PLAIN, shape, strides, getattr(torch, dtype), True, H,
                            wRank or 0, uRank or 0, NON_LINEARITY[gate], 2, case["layout"] == "btf",
                            case["mode"].endswith("_last"), None if affine else MODES[case["mode"]])


def test_fixture_covers_the_table():
    assert set(RECORDED["cases"]) == set(CASES) and len(RECORDED["unstable"]) <= 3
    for k, row in RECORDED["cases"].items():
        assert ("digest" in row) != (k in RECORDED["unstable"]), k


ROUTED = sorted(k for k, c in CASES.items() if c["method"] == "forward" and c["cls"] != "RNNClassifierModel"
                and not c.get("training"))


@pytest.mark.parametrize("case_id", ROUTED)
def test_record_implies_the_recorded_calls(case_id):
    case, row = CASES[case_id], RECORDED["cases"][case_id]
    s = signature(case)
    r = _route.route(s)
    T, B, F = r.dims
    assert (T, B, F) == (RC.T, RC.B, RC.CELLS[case["cell"]][1])
    fwd = row["calls"][0]
    assert fwd["entry"] == ("forward_unroll_affine" if s.kind == _route.AFFINE else "forward_unroll")
    assert fwd["flags"] == r.flags
    if s.kind == _route.PLAIN:
        assert fwd["want_gates"] == (r.saved is not None)
        assert (r.saved == _route.PREACT) == bool(r.flags & _lib.FLAG_SAVE_PREACT)
    else:
        assert r.saved is None
    presented = {_route.AS_IS: [list(s.shape), list(s.strides)],
                 _route.CONTIGUOUS: [list(s.shape), _dense(s.shape)],
                 _route.BFT_BASE: [[B, F, T], _dense((B, F, T))],
                 _route.TRANSPOSE_COPY: [[T, B, F], _dense((T, B, F))]}[r.present]
    assert fwd["seq"][:2] == presented
    lead = [B, T] if r.flags & _lib.FLAG_BATCH_MAJOR else [T, B]
    bwd = [c for c in row["calls"] if c["entry"] == "backward_unroll"]
    assert len(bwd) == (case["mode"] in ("grad_x", "grad", "grad_last")) and len(row["calls"]) == 1 + len(bwd)
    for c in bwd:
        assert c["flags"] == r.flags | (_lib.FLAG_GRAD_LAST if r.grad_last else 0)
        assert c["grad_h"] == ([B, s.H] if r.grad_last else lead + [s.H])
        assert c["seq"] == fwd["seq"]
    assert row["result"][0] == {_route.AS_IS: lead + [s.H], _route.TRANSPOSE_BACK: [B, T, s.H],
                                _route.LAST_STEP: [B, s.H], _route.LAST_STATE: [B, s.H]}[r.post]


def test_route_cache_is_bounded_with_one_entry_per_signature():
    cache = _route.route
    assert cache.cache_info().maxsize == 1024
    cache.cache_clear()
    sigs = {signature(CASES[k]) for k in ROUTED}
    for _ in range(2):
        for k in ROUTED:
            cache(signature(CASES[k]))
    info = cache.cache_info()
    assert info.currsize == info.misses == len(sigs) and info.hits == 2 * len(ROUTED) - len(sigs)


def test_two_hidden_sizes_with_one_input_shape_get_their_own_entries():
    _route.route.cache_clear()
    a, b = (signature(CASES["FastGRNNCUDA-forward-%s-tbf-nograd" % c]) for c in ("h128f32", "h256f32"))
    assert a.shape == b.shape and a != b
    ra, rb = _route.route(a), _route.route(b)
    assert _route.route.cache_info().currsize == 2 and ra.saved is None and rb.saved is None


def test_seen_is_cleared_when_full():
    seen = fastgrnn_cuda._seen
    kept = dict(seen)
    try:
        seen.clear()
        for i in range(fastgrnn_cuda._SEEN_MAX):
            fastgrnn_cuda._remember(("stand-in", i), i)
        assert len(seen) == fastgrnn_cuda._SEEN_MAX == 1024 and seen is fastgrnn_cuda._seen
        fastgrnn_cuda._remember(("stand-in", "one more"), 0)
        assert seen == {("stand-in", "one more"): 0}
    finally:
        seen.clear()
        seen.update(kept)
