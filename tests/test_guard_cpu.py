"""CPU-side checks of the gradient guard (fastgrnn_hip_grad_guard and the guarded update calls, kws_amd/optim.py's
``guard()``): the restatement of tests/guard_cases.py held to torch.nn.utils.clip_grad_norm_ in fp64; every refusal of
the three entry points without a launch; ``guard()``'s argument errors; checkpoints of guarded and unguarded optimizers
on CPU tensors; a schedule's logs on an unguarded optimizer; and the static scans of kernels_guard.hip."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import _lib, optim
from tests import guard_cases as G
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_guard.hip")
NULL, ONE = None, 256                                   # (a fake non-NULL, 8-byte aligned pointer: nothing is launched)
OK, NULLP, SHAPE, WORKSPACE, UNSUP = 0, 1, 2, 5, 7


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


# ---- the restatement against clip_grad_norm_ ---------------------------------------------------------------------------
def torch_clip(grads, max_norm):
    """clip_grad_norm_ (error_if_nonfinite=False) on fp64 copies -> (total_norm, the clipped gradients)"""
    ps = [torch.nn.Parameter(torch.zeros(len(g), dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(np.asarray(g, dtype=np.float64).copy())
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False, foreach=False)
    return float(total), [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("ratio", (0.25, 0.999, 1.0, 1.001, 10.0, 1e4))
def test_coef_is_clip_grad_norms(ratio):
    """norm / max_norm below, at and above one"""
    grads = [G.gradient(n, 3) for n in (1, 37, 1025)]
    root = math.sqrt(G.sumsq(grads))
    max_norm = root / ratio
    r = G.restate(grads, max_norm)
    total, clipped = torch_clip(grads, max_norm)
    assert abs(total - root) <= 1e-13 * root
    assert r["norm"] == np.float32(root) and r["skip"] == 0 and (r["applied"], r["skipped"]) == (1, 0)
    want = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(r["coef"]) - want) <= 2.0 ** -24 * want            # one rounding to fp32 of the same double
    if ratio < 1.0:
        assert r["coef"] == 1.0 and all(np.array_equal(c, g.astype(np.float64)) for c, g in zip(clipped, grads))
    else:                                                               # (at max_norm: max_norm / (max_norm + 1e-6) < 1)
        assert r["coef"] < 1.0
        big = int(np.argmax(np.abs(grads[2])))
        assert abs(clipped[2][big] / float(grads[2][big]) - want) <= 1e-12 * want
    assert G.restate(grads)["coef"] == 1.0                              # max_norm = inf: no clipping at any norm


@pytest.mark.parametrize("bad", G.BAD_VALUES)
def test_nonfinite_gradients_as_clip_grad_norm_treats_them(bad):
    g = np.array(G.gradient(37, 4))
    g[5] = bad
    grads = [G.gradient(9, 4), g]
    total, clipped = torch_clip(grads, 1.0)
    r = G.restate(grads, 1.0, skip_nonfinite=False)
    assert r["skip"] == 0 and (r["applied"], r["skipped"]) == (1, 0)
    if math.isnan(bad):
        assert math.isnan(total) and math.isnan(r["S"]) and np.isnan(r["norm"]) and np.isnan(r["coef"])
        assert all(np.isnan(c).all() for c in clipped)                   # torch's coefficient was a NaN too
    else:
        assert total == math.inf and r["S"] == math.inf and r["norm"] == np.float32(np.inf) and r["coef"] == 0.0
        assert (clipped[0] == 0).all()                                   # torch's coefficient was 0
    assert G.restate(grads, skip_nonfinite=False)["coef"] == 1.0          # max_norm = inf: nothing is scaled
    s = G.restate(grads, 1.0, skip_nonfinite=True, applied=4, skipped=2)
    assert s["skip"] == 1 and s["coef"] == 0.0 and (s["applied"], s["skipped"]) == (4, 3)


def test_sumsq_is_exact_where_it_can_be_checked():
    assert G.sumsq([np.array([3.0, 4.0], np.float32)]) == 25.0
    assert G.sumsq([np.array([2.0 ** 100], np.float32), np.array([1.0], np.float32)]) == 2.0 ** 200      # (1 is below an ulp)
    big = np.full(1000, np.finfo(np.float32).max, np.float32)
    assert math.isfinite(G.sumsq([big]))                                 # finite gradients cannot overflow the double
    assert G.ulps_apart(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1 and G.ulps_apart(0.5, 0.5) == 0


# ---- the entry points' refusals, no launch -------------------------------------------------------------------------------
def _guard(lib, segs=None, n_segs=None, max_norm=1.0, flags=1, state=ONE, ws=ONE, ws_bytes=None, no_segs=False):
    segs = [_lib.GuardSeg(ONE, 100)] if segs is None else segs
    arr = (_lib.GuardSeg * len(segs))(*segs)
    n = len(segs) if n_segs is None else n_segs
    if ws_bytes is None:
        ws_bytes = lib.fastgrnn_hip_grad_guard_workspace_bytes(n)
    return lib.fastgrnn_hip_grad_guard(None if no_segs else arr, n, max_norm, flags, state, ws, ws_bytes, None)


def test_symbols_struct_sizes_and_the_abi_version(lib):
    for name in ("fastgrnn_hip_grad_guard_workspace_bytes", "fastgrnn_hip_grad_guard", "fastgrnn_hip_train_update_guarded",
                 "fastgrnn_hip_optim_update_guarded"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.fastgrnn_hip_abi_version() == 1
    assert C.sizeof(_lib.GuardState) == 32 and C.sizeof(_lib.GuardSeg) == 16
    assert _lib.GuardState.applied.offset == 16 and _lib.GuardState.skipped.offset == 24 and _lib.GuardState.skip.offset == 8
    assert C.sizeof(_lib.UpdateSeg) == 64 and C.sizeof(_lib.UpdateHyper) == 40 and C.sizeof(_lib.OptimSeg) == 72
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    assert "float norm, coef; int32_t skip, reserved; int64_t applied, skipped;" in header
    assert "#define FASTGRNN_GUARD_SKIP_NONFINITE 1" in header


def test_workspace_size(lib):
    f = lib.fastgrnn_hip_grad_guard_workspace_bytes
    assert [f(n) for n in (-3, 0, 1, 32, 33, 1000)] == [0, 0, 256, 256, 512, 8192]
    for n in (1, 31, 32, 33, 64, 65, 777):
        assert f(n) >= 8 * n and f(n) % 256 == 0


def test_grad_guard_refusals(lib):
    assert _guard(lib, no_segs=True) == NULLP
    assert _guard(lib, state=NULL) == NULLP
    assert _guard(lib, ws=NULL) == NULLP
    assert _guard(lib, [_lib.GuardSeg(ONE, 5), _lib.GuardSeg(NULL, 5)]) == NULLP       # every segment is looked at
    assert _guard(lib, n_segs=0, ws_bytes=256) == SHAPE
    assert _guard(lib, n_segs=-1, ws_bytes=256) == SHAPE
    for n in (0, -5, (1 << 22) + 1):
        assert _guard(lib, [_lib.GuardSeg(ONE, n)]) == SHAPE, n
    for m in (0.0, -1.0, float("nan"), -math.inf):
        assert _guard(lib, max_norm=m) == SHAPE, m
    for flags in (2, 3, -1, 1 << 16):
        assert _guard(lib, flags=flags) == UNSUP, flags
    assert _guard(lib, ws_bytes=255) == WORKSPACE
    assert _guard(lib, [_lib.GuardSeg(ONE, 5)] * 33, ws_bytes=256) == WORKSPACE          # 33 segments need 512 bytes
    assert _guard(lib, ws=ONE + 4) == WORKSPACE                                          # not 8-byte aligned


def _useg(**kw):
    d = dict(param=ONE, grad=ONE, state0=ONE, state1=ONE, support=NULL, n=100, keep_rank=0, iht=0, reserved=0)
    d.update(kw)
    return _lib.UpdateSeg(**d)


def _train(lib, segs=None, h=None, n_segs=None, lr=ONE, guard=ONE, mode=ONE):
    segs = [_useg()] if segs is None else segs
    arr = (_lib.UpdateSeg * len(segs))(*segs)
    h = _lib.UpdateHyper(_lib.ADAM, 0, 0.9, 0.999, 1e-8, 0.0) if h is None else h
    return lib.fastgrnn_hip_train_update_guarded(C.byref(h) if h is not False else None, arr,
                                                 len(segs) if n_segs is None else n_segs, lr, guard, mode, None)


def test_train_update_guarded_refuses_what_train_update_refuses(lib):
    assert _train(lib, guard=NULL) == NULLP                               # the state stands where `step` stood
    assert _train(lib, h=False) == NULLP and _train(lib, lr=NULL) == NULLP
    for name in ("param", "grad", "state0", "state1"):
        assert _train(lib, [_useg(**{name: NULL})]) == NULLP, name
    assert _train(lib, [_useg(iht=1, support=NULL)]) == NULLP
    assert _train(lib, [_useg(iht=1, support=ONE)], mode=NULL) == NULLP
    assert _train(lib, n_segs=0) == SHAPE
    for n in (0, (1 << 22) + 1):
        assert _train(lib, [_useg(n=n)]) == SHAPE
    assert _train(lib, [_useg(n=10, keep_rank=10)]) == SHAPE
    for h in (_lib.UpdateHyper(_lib.ADAM, 0, 1.0, 0.999, 1e-8, 0.0), _lib.UpdateHyper(_lib.ADAM, 0, 0.9, 0.999, 0.0, 0.0),
              _lib.UpdateHyper(_lib.ADAM, 0, 0.9, 0.999, 1e-8, -1.0), _lib.UpdateHyper(_lib.SGD, 1, 0.0, 0.0, 0.0, 0.0),
              _lib.UpdateHyper(_lib.ADAM, 0, float("nan"), 0.999, 1e-8, 0.0)):
        assert _train(lib, h=h) == SHAPE
    for algo in (2, -1, 7):
        assert _train(lib, h=_lib.UpdateHyper(algo, 0, 0.9, 0.999, 1e-8, 0.0)) == UNSUP


def _oseg(**kw):
    d = dict(param=ONE, grad=ONE, state=(ONE, ONE, ONE), support=NULL, n=100, keep_rank=0, iht=0, reserved=0)
    d.update(kw)
    return _lib.OptimSeg(**d)


def _optim(lib, segs=None, h=None, n_segs=None, lr=ONE, guard=ONE, mode=ONE, scalars=ONE):
    segs = [_oseg()] if segs is None else segs
    arr = (_lib.OptimSeg * len(segs))(*segs)
    h = _lib.OptimHyper(_lib.ADAMAX, 0, (0.9, 0.999, 1e-8), 0.0) if h is None else h
    return lib.fastgrnn_hip_optim_update_guarded(C.byref(h), arr, len(segs) if n_segs is None else n_segs, lr, guard, mode,
                                                 scalars, None)


def test_optim_update_guarded_refuses_what_optim_update_refuses(lib):
    assert _optim(lib, guard=NULL) == NULLP and _optim(lib, lr=NULL) == NULLP
    assert _optim(lib, [_oseg(param=NULL)]) == NULLP and _optim(lib, [_oseg(state=(NULL, ONE, ONE))]) == NULLP
    assert _optim(lib, [_oseg(state=(ONE, NULL, NULL))]) == NULLP         # Adamax reads two state tensors
    assert _optim(lib, [_oseg(iht=1)]) == NULLP
    assert _optim(lib, h=_lib.OptimHyper(_lib.ASGD, 0, (1e-4, 0.75, 1e6), 0.0), scalars=NULL) == NULLP
    assert _optim(lib, n_segs=0) == SHAPE and _optim(lib, [_oseg(n=0)]) == SHAPE
    assert _optim(lib, h=_lib.OptimHyper(_lib.ADAMAX, 0, (1.0, 0.999, 1e-8), 0.0)) == SHAPE
    assert _optim(lib, h=_lib.OptimHyper(_lib.RPROP, 0, (0.5, 1.2, 1e-6, 50.0), 1e-5)) == SHAPE
    assert _optim(lib, h=_lib.OptimHyper(_lib.RMSPROP, 0, (0.99, 0.0, 0.0), 0.0)) == SHAPE
    for algo in (0, 1, 8):
        assert _optim(lib, h=_lib.OptimHyper(algo, 0, (0.9, 0.999, 1e-8), 0.0)) == UNSUP


# ---- guard() on CPU tensors ----------------------------------------------------------------------------------------------
def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(5, 7, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g)),
            torch.nn.Parameter(torch.randn(1, 1, generator=g))]


def test_guard_allocates_its_state_and_returns_self():
    opt = optim.FusedAdam(_params())
    assert not opt.guarded
    assert opt.guard(max_grad_norm=2.5) is opt and opt.guarded
    assert opt.grad_norm_t.dtype == opt.clip_coef_t.dtype == torch.float32 and opt.skip_t.dtype == torch.int32
    assert opt.applied_t.dtype == opt.skipped_t.dtype == torch.int64
    state = opt._guard[2]
    assert state.numel() * state.element_size() == 32
    for t, off in ((opt.grad_norm_t, 0), (opt.clip_coef_t, 4), (opt.skip_t, 8), (opt.applied_t, 16), (opt.skipped_t, 24)):
        assert t.numel() == 1 and t.data_ptr() == state.data_ptr() + off                   # views of the one state
    assert opt._guard[:2] == (2.5, _lib.GUARD_SKIP_NONFINITE) and int(state.abs().sum()) == 0
    assert opt._guard[3].numel() * 8 >= S.built_library().fastgrnn_hip_grad_guard_workspace_bytes(3)
    assert optim.FusedSGD(_params(), lr=0.1).guard()._guard[:2] == (math.inf, 1)             # the default: skip only
    assert optim.FusedRprop(_params()).guard(1.0, skip_nonfinite=False)._guard[:2] == (1.0, 0)
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    segs, n = opt._segments()
    gsegs = opt._table[5]
    assert n == 3 and [(gsegs[i].grad, gsegs[i].n) for i in range(3)] == [(segs[i].grad, segs[i].n) for i in range(3)]
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()


def test_guard_argument_errors():
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FusedAdam(_params()).guard(max_grad_norm=bad)
    with pytest.raises(ValueError, match="nothing to guard"):
        optim.FusedAdam(_params()).guard(None, skip_nonfinite=False)
    opt = optim.FusedAdam(_params()).guard()
    with pytest.raises(RuntimeError, match="once"):
        opt.guard(1.0)
    late = optim.FusedAdam(_params())
    late.step_t.fill_(1)                                                   # (what a step leaves behind)
    with pytest.raises(RuntimeError, match="before the first step"):
        late.guard(1.0)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_a_guarded_checkpoint_resumes_in_torch_adam_with_the_applied_count():
    ps = _params()
    ref = torch.optim.Adam(ps, lr=0.02, betas=(0.8, 0.99), eps=1e-6, foreach=False)
    for k in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        ref.step()
    fused = optim.FusedAdam(ps).guard(max_grad_norm=1.0)
    fused.load_state_dict(copy.deepcopy(ref.state_dict()))                 # torch's checkpoint: every step was applied
    assert (int(fused.applied_t), int(fused.skipped_t), int(fused.step_t)) == (3, 0, 3)
    # as if two further iterations had been rejected
    fused.skipped_t.fill_(2)
    fused.step_t.fill_(5)
    out = fused.state_dict()
    assert out["guard"] == {"applied": 3, "skipped": 2} and out["fused_step"] == 5
    assert all(float(st["step"]) == 3.0 for st in out["state"].values())    # the bias correction's count: steps taken
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch.optim.Adam(ps2, foreach=False)
    back.load_state_dict(copy.deepcopy(out))                               # torch ignores the extra keys
    for p, q in zip(ps, ps2):
        p.grad = torch.full_like(p, -0.3)
        q.grad = torch.full_like(q, -0.3)
    ref.step()
    back.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, ps2))                  # ... and goes on as the original does
    again = optim.FusedAdam(ps).guard(max_grad_norm=1.0)
    again.load_state_dict(out)
    assert (int(again.applied_t), int(again.skipped_t), int(again.step_t)) == (3, 2, 5)
    assert float(again.grad_norm_t) == 0.0 and int(again.skip_t) == 0
    plain = optim.FusedAdam(ps)                                             # an unguarded optimizer takes it too
    plain.load_state_dict(out)
    assert int(plain.step_t) == 3 and not plain.guarded


@pytest.mark.parametrize("cls", ("FusedAdam", "FusedSGD", "FusedASGD", "FusedRprop"))
def test_an_unguarded_checkpoint_has_no_new_key(cls):
    ps = _params()
    kw = dict(lr=0.1, momentum=0.9) if cls == "FusedSGD" else {}
    opt = getattr(optim, cls)(ps, **kw)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "iht_support", "fused_step"}
    guarded = getattr(optim, cls)(_params(), **kw).guard()
    assert set(guarded.state_dict()) == set(sd) | {"guard"}
    assert sd["param_groups"] == guarded.state_dict()["param_groups"]      # guard() is no hyper-parameter of the group


def test_the_schedules_logs_on_an_unguarded_optimizer_are_unchanged():
    from kws_amd import TrainSchedule
    opt = optim.FusedAdam(_params(), capturable=True)
    sched = TrainSchedule(opt, 64, 8, 3, seed=1)
    assert sched.norm_log is None and sched.skip_log is None
    sched.where[2] = 5
    sched.record(torch.tensor(0.75))
    assert float(sched.loss_log[5]) == 0.75 and sched.norm_log is None
    log = sched.epoch_log()
    assert len(log) == 3 and all(set(e) == {"epoch", "loss", "accuracy", "learning_rate"} for e in log)
    # a guard, before or after the schedule is built, adds the two logs
    for early in (True, False):
        o = optim.FusedAdam(_params(), capturable=True)
        if early:
            o.guard(1.0)
        s = TrainSchedule(o, 64, 8, 3, seed=1)
        if not early:
            o.guard(1.0)
        o.grad_norm_t.fill_(2.5)
        o.skip_t.fill_(1)
        for slot in (7, 15, 23):                                            # the last slot of each epoch (8 ticks)
            s.where[2] = slot
            s.record(torch.tensor(0.5))
        assert s.norm_log.dtype == torch.float32 and s.skip_log.dtype == torch.int32 and s.norm_log.numel() == 24
        log = s.epoch_log()
        assert [e["skipped"] for e in log] == [1, 1, 1] and [e["grad_norm"] for e in log] == [2.5] * 3
        assert all(set(e) == {"epoch", "loss", "accuracy", "learning_rate", "skipped", "grad_norm"} for e in log)


def test_run_state_holds_the_guards_tensors():
    from kws_amd import RNNClassifierModel, TrainSchedule
    model = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=12, device=torch.device("cpu"))
    opt = optim.FusedAdam(model.parameters(), capturable=True).guard(1.0)
    sched = TrainSchedule(opt, 64, 8, 3, seed=1)
    from kws_amd import RunSnapshot
    held = {t.data_ptr() for t, _ in RunSnapshot([model, opt, sched]).held}
    assert {opt._guard[2].data_ptr(), sched.norm_log.data_ptr(), sched.skip_log.data_ptr()} <= held
    plain = optim.FusedAdam(model.parameters(), capturable=True)
    n_plain = len(RunSnapshot([model, plain, TrainSchedule(plain, 64, 8, 3, seed=1)]).held)
    assert len(RunSnapshot([model, opt, sched]).held) == n_plain + 3


# ---- static scans of kernels_guard.hip ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guard_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_guard.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(guard_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), guard_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(guard_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), guard_asm, "--strict"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_the_kernels_use_no_scratch_and_stay_inside_update_ks_limits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = resource_usage.usage(SRC)
    assert sorted(r["pretty"] for r in rows) == (["grad_sumsq_k", "guard_finish_k"]
                                                 + ["void guarded_update_k<%d>" % a for a in range(8)])
    for r in rows:
        assert r["scratch"] == 0 and r["lds"] <= 2048 and r["vgpr"] <= 64, r               # tests/test_update_cpu.py's limits


def test_the_guard_source_holds_no_copy_of_the_rules():
    """kernels_guard.hip includes kernels_update.hip with UPDATE_GUARD 1 (the eight kernels that file gives on its own
    are tests/test_update_cpu.py's to list)"""
    text = open(SRC).read()
    assert '#define UPDATE_GUARD 1\n#include "kernels_update.hip"' in text
    assert "fmaf(hy.wd" not in text and "atomicAdd" not in text
