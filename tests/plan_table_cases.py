"""The questions of the plan table (tests/golden/plan/plan_table.npz): every descriptor of test_plan_cpu._both_grids(), each
B = 37 descriptor again at five more (T, B), and what the library answers to every query about them.  Shared by
tests/golden/make_plan_table.py, which recorded the answers of the library before its host code was reorganised, and
tests/test_plan_table_cpu.py, which asks the built library the same questions."""
import ctypes as C

import numpy as np

from kws_amd import _lib
from tests.test_plan_cpu import _both_grids

# (T, B) asked on top of the grid's own; (50, 83) and (3, 1377) are the shapes whose bf16 dU product once wrote past
# the H = 256 backward's workspace (first item)
EXTRA_TB = ((1, 1), (3, 17), (50, 83), (3, 1377), (99, 130))
POOL_ROWS = (None, 1000, 2 ** 31 - 1)          # None: the descriptor's own T
HEAD_SHAPES = ((1, 128, 12), (37, 128, 12), (4096, 256, 35))
DESC_FIELDS = [n for n, _ in _lib.Desc._fields_]


def descriptors():
    for d in _both_grids():
        yield d
        if d.B == 37:
            for T, B in EXTRA_TB:
                yield _lib.Desc(T, B, *[getattr(d, n) for n in DESC_FIELDS[2:]])


def answers(lib):
    """desc [N, 10], plan [N, 1 + 15] (status, then every field of fastgrnn_plan, zext included), extra [N, 14] (the
    windowed, windowed-training and BatchNorm-training queries; the workspace queries only where the call is
    supported, 0 elsewhere), head [3, 2]"""
    desc, plan, extra = [], [], []
    p = _lib.Plan()
    for d in descriptors():
        r = C.byref(d)
        st = lib.fastgrnn_hip_plan(r, C.byref(p))
        z = p.zext
        desc.append([getattr(d, n) for n in DESC_FIELDS])
        plan.append([st, p.path[0], p.path[1], p.forward_ws_optional, p.dx_optional, p.rank_space_cols, p.reserved,
                     p.workspace_bytes[0], p.workspace_bytes[1], z.forward, z.backward, z.Hp, z.Fp, z.dx_optional,
                     z.reserved, z.saved_bytes])
        pools = [d.T if n is None else n for n in POOL_ROWS]
        win, twin, bn = (lib.fastgrnn_hip_windows_supported(r), lib.fastgrnn_hip_train_windows_supported(r),
                         lib.fastgrnn_hip_bn_train_supported(r))
        row = [win, twin, bn]
        row += [lib.fastgrnn_hip_forward_windows_workspace_bytes(r, n) if win else 0 for n in pools]
        row += [lib.fastgrnn_hip_train_windows_forward_workspace_bytes(r, n) if twin else 0 for n in pools]
        row += [lib.fastgrnn_hip_train_windows_backward_workspace_bytes(r, n) if twin else 0 for n in pools]
        row += [f(r) if bn else 0 for f in (lib.fastgrnn_hip_bn_train_forward_workspace_bytes,
                                            lib.fastgrnn_hip_bn_train_backward_workspace_bytes)]
        extra.append(row)
        assert len(row) == 14
    head = [[lib.fastgrnn_hip_head_workspace_bytes(*s), lib.fastgrnn_hip_head_predict_workspace_bytes(*s)]
            for s in HEAD_SHAPES]
    return dict(desc=np.array(desc, dtype=np.int64), plan=np.array(plan, dtype=np.int64),
                extra=np.array(extra, dtype=np.int64), head=np.array(head, dtype=np.int64))
