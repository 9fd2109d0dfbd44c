"""The modules hand the operator shim what they handed it before their routing was gathered into kws_amd._route: every
case of tests/route_cases.py replayed under the recorder's wrappers (tools/record_module_routes.py) against
tests/golden/routes/parent.json -- the same shim calls in the same order (entry point, presented shape / strides /
dtype, flags, want_gates, need_dx), the same result shape / strides / dtype, and bit-identical results and gradients
(one sha256 per case; a case whose two parent recordings differed is compared on its calls and metadata alone)."""
import json
import os
import sys

import pytest
import torch

from tests import route_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "routes", "parent.json")) as _f:
    RECORDED = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def recorder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import record_module_routes
    finally:
        sys.path.pop(0)
    return record_module_routes


@pytest.mark.parametrize("case", RC.cases(), ids=lambda c: c["id"])
def test_module_route(case, recorder):
    want = RECORDED[case["id"]]
    got = recorder.run_case(case, torch.device("cuda:0"))
    assert got["calls"] == want["calls"]
    assert got["result"] == want["result"]
    if "digest" in want:
        assert got["digest"] == want["digest"]
