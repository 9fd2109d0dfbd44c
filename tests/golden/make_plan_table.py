#!/usr/bin/env python3
"""Record tests/golden/plan/plan_table.npz: what a library built from the commit BEFORE a reorganisation of the host code
answers to every question of tests/plan_table_cases.py.

    FASTGRNN_HIP_LIB=/path/to/the/parent/commit's/libfastgrnn_hip.so python tests/golden/make_plan_table.py

The fixture is recorded data.  It is never regenerated from the code it checks: the library has to be named, and a
change that is meant to alter an answer regenerates the file from the commit that introduces the new answer and says
so."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    if not os.environ.get("FASTGRNN_HIP_LIB"):
        sys.exit("name the recorded library through FASTGRNN_HIP_LIB (see the docstring)")
    from kws_amd import _lib
    from tests.plan_table_cases import answers
    out = os.path.join(ROOT, "tests", "golden", "plan", "plan_table.npz")
    table = answers(_lib.load())
    np.savez_compressed(out, **table)
    print("%s: %d rows, %d bytes" % (out, len(table["desc"]), os.path.getsize(out)))
