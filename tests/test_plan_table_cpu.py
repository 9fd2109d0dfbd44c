"""The built library answers every query exactly as the recorded table says (tests/golden/plan/plan_table.npz, written by
tests/golden/make_plan_table.py from the library before its host code was reorganised): status and every field of
fastgrnn_plan over the grid of test_plan_cpu at the grid's and five more (T, B), the windowed, windowed-training and
BatchNorm-training queries, the two head queries.  No kernel is launched."""
import os

import numpy as np
import pytest

from tests.plan_table_cases import answers
from tests import support as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan", "plan_table.npz")


@pytest.fixture(scope="module")
def tables():
    return dict(np.load(GOLDEN)), answers(S.built_library())


def test_the_table_asks_what_was_recorded(tables):
    want, got = tables
    assert len(want["desc"]) > 70000
    assert np.array_equal(want["desc"], got["desc"])


@pytest.mark.parametrize("name", ["plan", "extra", "head"])
def test_every_answer_is_the_recorded_one(tables, name):
    want, got = tables
    assert want[name].shape == got[name].shape
    rows = np.flatnonzero((want[name] != got[name]).any(axis=1))
    assert rows.size == 0, (name, rows.size, [(want["desc"][r].tolist() if name != "head" else r, want[name][r].tolist(),
                                               got[name][r].tolist()) for r in rows[:5]])
