#!/usr/bin/env python3
"""Record the learning rates of the reference's five schedulers, for tests/test_schedule_cpu.py.

Run where a checkout of the reference is at hand (it is only imported, never copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/schedule/make_schedule_golden.py /path/to/reference

Writes DATA only, next to this script: lr_tables.npz.  For each configuration ``(num_epochs, ticks, lr_peaks)`` of
``CONFIGS`` the constants are computed as the reference's ``configure_lr`` computes them (trainClassifier.py:97-123), each
scheduler -- the reference's ``TriangularLR`` and ``ExponentialResettingLR`` (utils.py:116-143), torch's
``CosineAnnealingLR``, ``ExponentialLR`` and ``StepLR`` -- is built on a dummy SGD and stepped; row ``it`` of a table is the
optimizer's learning rate after ``it`` calls of ``scheduler.step()`` (row 0: as constructed), in float64.  Keys:
``c{i}_{name}`` the table ``[ROWS]``, ``c{i}_{name}_valid`` how many of its rows were recorded before the scheduler
raised (torch's recursive cosine divides by zero at some ``T_max``), ``c{i}_constants`` = (lr, lr_min, gamma, stepsize,
t_max, step_size, reset), ``c{i}_config`` = (num_epochs, ticks, lr_peaks), ``names``.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = ((30, 10, 1), (9, 7, 1))
LR, LR_MIN, GAMMA, STEP_SIZE, ROWS = 1e-3, 1e-5, 0.97, 4, 100
NAMES = ("TriangleLR", "CosineAnnealingLR", "ExponentialLR", "StepLR", "ExponentialResettingLR")


def main(ref):
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(ref, "utils.py"))
    ref_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_utils)
    sched = torch.optim.lr_scheduler
    out = {"names": np.array(NAMES)}
    for i, (num_epochs, ticks, peaks) in enumerate(CONFIGS):
        steps = peaks * 2 + 1                                        # configure_lr, line by line
        stepsize = num_epochs / steps
        total_iterations = ticks * num_epochs
        reset = (num_epochs * ticks) / 3
        build = {
            "TriangleLR": lambda o: ref_utils.TriangularLR(o, stepsize * ticks, LR_MIN, LR, GAMMA),
            "CosineAnnealingLR": lambda o: sched.CosineAnnealingLR(o, T_max=total_iterations / steps, eta_min=LR_MIN),
            "ExponentialLR": lambda o: sched.ExponentialLR(o, GAMMA),
            "StepLR": lambda o: sched.StepLR(o, step_size=STEP_SIZE, gamma=GAMMA),
            "ExponentialResettingLR": lambda o: ref_utils.ExponentialResettingLR(o, GAMMA, reset),
        }
        out["c%d_config" % i] = np.array([num_epochs, ticks, peaks], dtype=np.int64)
        out["c%d_constants" % i] = np.array([LR, LR_MIN, GAMMA, stepsize * ticks, total_iterations / steps, STEP_SIZE,
                                             int(reset)], dtype=np.float64)
        for name in NAMES:
            opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR)
            table, valid = np.zeros(ROWS, dtype=np.float64), 0
            try:
                s = build[name](opt)
                for it in range(ROWS):
                    table[it] = opt.param_groups[0]["lr"]
                    valid = it + 1
                    opt.step()
                    s.step()
            except ZeroDivisionError:
                pass
            out["c%d_%s" % (i, name)] = table
            out["c%d_%s_valid" % (i, name)] = np.int64(valid)
            print("config %d %-24s valid %3d  first %.6g  last %.6g" % (i, name, valid, table[0], table[valid - 1]))
    np.savez_compressed(os.path.join(HERE, "lr_tables.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
