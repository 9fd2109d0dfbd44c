"""The device-side schedule without a GPU: the permutation oracle of tests/schedule_cases.py is a bijection that spreads
evenly, its learning rates match the reference's schedulers (tests/golden/schedule/lr_tables.npz), the integer IHT rule
is ``kws_amd.iht_phase``, the C ABI refuses what the header says it refuses (all before any launch), ``TrainSchedule``
checks its arguments and derives ``configure_lr``'s constants, and the static scans of DESIGN.md 4.0 pass on the new
kernel file."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import FusedAdam, FusedSGD, TrainSchedule, _lib
from tests import schedule_cases as K
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_schedule.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "schedule", "lr_tables.npz")
OK, NULLP, SHAPE, UNSUP = 0, 1, 2, 7
SEED = 0x9E3779B97F4A7C15
SHARDS = ((50, 8, 1), (64, 8, 2), (8, 8, 1), (17, 1, 4))


# ---- the permutation -----------------------------------------------------------------------------------------------------
def test_domain_bits():
    assert [K.domain_bits(n) for n in (1, 2, 4, 5, 16, 17, 256, 257, 85511, 2 ** 31 - 1)] == [2, 2, 2, 4, 4, 6, 8, 10, 18, 32]


@pytest.mark.parametrize("N", K.SIZES)
def test_epoch_perm_is_a_bijection_and_epochs_differ(N):
    """Seed 99, the spread check's.  N = 2 has two orders in all, so for half of all seeds epochs 0 and 1 agree there
    (N = 3: a sixth): "consecutive epochs differ" is a statement about this seed at the small sizes and about the
    epoch entering the key at the large ones, where the bijection is checked under the other seed too."""
    orders = []
    for epoch in K.EPOCHS:
        order, passes = K.epoch_perm(99, epoch, np.arange(N), N, count_passes=True)
        assert np.array_equal(np.sort(order), np.arange(N)), (N, epoch)
        assert passes <= 64, (N, epoch, passes)                      # (the domain is below 4 N: a walk this long is a bug)
        orders.append(order)
    if N > 1:
        assert not np.array_equal(orders[0], orders[1]), N
    # a scalar position, the seed's and the epoch's high words
    assert K.epoch_perm(99, 1, N - 1, N) == orders[1][N - 1]
    if N >= 255:
        other = K.epoch_perm(SEED, 0, np.arange(N), N)
        assert np.array_equal(np.sort(other), np.arange(N)) and not np.array_equal(other, orders[0])
        assert not np.array_equal(K.epoch_perm(99 + (1 << 32), 0, np.arange(N), N), orders[0])
        assert not np.array_equal(K.epoch_perm(99, 1 << 32, np.arange(N), N), orders[0])


@pytest.mark.parametrize("N,B,world", SHARDS)
def test_the_ranks_batches_of_an_epoch_are_disjoint_clips(N, B, world):
    ticks = N // (B * world)
    for epoch in (0, 3):
        seen = np.concatenate([K.batch_index(SEED, epoch * ticks + i, N, B, world, rank)
                               for i in range(ticks) for rank in range(world)])
        assert seen.dtype == np.int32 and len(seen) == ticks * B * world == len(set(seen.tolist()))
        assert seen.min() >= 0 and seen.max() < N
    assert K.position(-5, N, B, world) == (0, 0, ticks) and K.position(3 * ticks + 1, N, B, world)[:2] == divmod(3 * ticks + 1, ticks)
    assert np.array_equal(K.batch_index(SEED, -7, N, B, world, 0), K.batch_index(SEED, 0, N, B, world, 0))


@pytest.mark.parametrize("pos", (0, 5))
def test_every_clip_lands_on_a_position_about_equally_often(pos):
    """N = 16, seed 99, epochs 0..4095: each clip's count on a fixed position is binomial(4096, 1/16), mean 256,
    sigma 15.5; the bound is five sigma.  The oracle alone: deterministic."""
    counts = np.zeros(16, dtype=np.int64)
    for epoch in range(4096):
        counts[K.epoch_perm(99, epoch, pos, 16)] += 1
    print("position %d: counts %d..%d" % (pos, counts.min(), counts.max()))
    assert counts.sum() == 4096 and counts.min() >= 178 and counts.max() <= 334, counts


# ---- the learning rate -----------------------------------------------------------------------------------------------------
def _ulps_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("config", (0, 1))
def test_lr_at_matches_the_recorded_schedulers(config):
    d = np.load(GOLDEN)
    num_epochs, ticks, peaks = (int(v) for v in d["c%d_config" % config])
    lr, lr_min, gamma, stepsize, t_max, step_size, reset = (float(v) for v in d["c%d_constants" % config])
    kw = K.constants(lr, num_epochs, ticks, peaks, lr_min, gamma, int(step_size))
    assert kw == dict(lr_base=lr, lr_min=lr_min, gamma=gamma, stepsize=stepsize, t_max=t_max, step_size=int(step_size),
                      reset=int(reset))
    assert (num_epochs, ticks, peaks) == ((30, 10, 1), (9, 7, 1))[config] and gamma == 0.97
    for name in (str(n) for n in d["names"]):
        table, valid = d["c%d_%s" % (config, name)], int(d["c%d_%s_valid" % (config, name)])
        assert table.shape == (100,) and valid >= 50, (name, valid)
        worst = max(_ulps_apart(K.lr_at(name, it, **kw), table[it]) for it in range(valid))
        print("config %d %s: %d rows, at most %d fp32 ulp apart" % (config, name, valid, worst))
        assert worst <= 1, (name, worst)
        assert len(set(table[:valid].tolist())) > 10, name            # (a schedule, not a constant)
    assert K.lr_at(None, 17, **kw) == lr and K.lr_at(0, 0, **kw) == lr


def test_lr_at_spot_values():
    kw = dict(lr_base=0.5, lr_min=0.1, gamma=0.5, stepsize=4.0, t_max=8.0, step_size=3, reset=5)
    assert K.lr_at("StepLR", 8, **kw) == 0.5 * 0.25 and K.lr_at("ExponentialLR", 3, **kw) == 0.0625
    assert K.lr_at("ExponentialResettingLR", 5, **kw) == 0.5 * 0.5 ** 5 and K.lr_at("ExponentialResettingLR", 6, **kw) == 0.25
    assert K.lr_at("CosineAnnealingLR", 0, **kw) == 0.5 and abs(K.lr_at("CosineAnnealingLR", 8, **kw) - 0.1) < 1e-16
    assert K.lr_at("TriangleLR", 0, **kw) == 0.5 and K.lr_at("TriangleLR", 4, **kw) == 0.1
    assert K.lr_at("CosineAnnealingLR", 101, **dict(kw, t_max=100 / 3)) > 0          # where torch's recursion divides by 0


# ---- the IHT phase ---------------------------------------------------------------------------------------------------------
def test_the_integer_phase_rule_is_iht_phase():
    for num_epochs in range(1, 41):
        for epoch in range(num_epochs + 2):
            for trim in (1, 2, 3):
                for i_batch in range(7):
                    assert K.phase_by_integers(epoch, num_epochs, i_batch, trim) == K.phase(epoch, num_epochs, i_batch, trim), \
                        (epoch, num_epochs, i_batch, trim)
    assert K.phase(5, 9, 0, 1, sparsify=False) == 0 and {K.phase(e, 3, 0, 2) for e in range(3)} == {0, 1, 2}


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return S.built_library()


ONE = C.c_void_p(256)                          # a non-NULL pointer that no refused call may touch


def _desc(**kw):
    f = dict(N=50, B=8, world=1, rank=0, seed=SEED, num_epochs=3, trim_level=2, sparsify=1, lr_kind=0, lr_lead=1,
             reserved=0, log_len=18, lr_base=0.01, lr_min=0.001, gamma=0.97, stepsize=6.0, t_max=6.0, step_size=1, reset=6)
    f.update(kw)
    return _lib.ScheduleDesc(**f)


def _call(lib, d=None, step=ONE, index=ONE, lr=ONE, iht=ONE, where=ONE, no_desc=False):
    d = _desc() if d is None else d
    return lib.fastgrnn_hip_train_schedule(None if no_desc else C.byref(d), step, index, lr, iht, where, None)


def test_the_symbol_the_struct_and_the_header(lib):
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    assert hasattr(lib, "fastgrnn_hip_train_schedule") and "fastgrnn_hip_train_schedule" in _lib.EXPORTS
    assert "fastgrnn_hip_train_schedule(" in header and "fastgrnn_schedule_desc;" in header
    assert lib.fastgrnn_hip_abi_version() == 1 and C.sizeof(_lib.ScheduleDesc) == 112
    assert _lib.ScheduleDesc.log_len.offset == 48 and _lib.ScheduleDesc.lr_base.offset == 56
    for name, code in (("CONSTANT", 0), ("TRIANGLE", 1), ("COSINE", 2), ("EXPONENTIAL", 3), ("STEP", 4),
                       ("EXPONENTIAL_RESETTING", 5)):
        assert "#define FASTGRNN_LR_%s %d\n" % (name, code) in header
    assert _lib.LR_KINDS == K.KINDS


def test_the_call_refuses_null_pointers(lib):
    assert _call(lib, no_desc=True) == NULLP
    for kw in (dict(step=None), dict(index=None), dict(lr=None), dict(where=None), dict(iht=None)):
        assert _call(lib, **kw) == NULLP, kw
    # without sparsify the phase's pointer may be NULL (the next refusal in line shows it)
    assert _call(lib, _desc(sparsify=0, lr_kind=9), iht=None) == UNSUP


def test_the_call_refuses_bad_shapes(lib):
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(B=-1), dict(world=0), dict(rank=-1), dict(rank=1), dict(world=2, rank=2), dict(N=7),
               dict(N=0), dict(N=-3), dict(world=7), dict(B=1 << 16, world=1 << 15, N=2 ** 31 - 1),
               dict(B=2 ** 31 - 1, world=2, rank=1, N=2 ** 31 - 1), dict(num_epochs=0), dict(trim_level=0),
               dict(log_len=0), dict(log_len=-1), dict(lr_lead=2), dict(lr_lead=-1),
               dict(lr_base=-1e-9), dict(lr_base=nan), dict(lr_base=inf), dict(lr_min=-1.0), dict(lr_min=nan),
               dict(lr_min=inf)):
        assert _call(lib, _desc(**kw)) == SHAPE, kw
    for kinds, bad in (((1, 3, 4, 5), (dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=nan), dict(gamma=inf))),
                       ((1,), (dict(stepsize=0.0), dict(stepsize=-1.0), dict(stepsize=nan), dict(stepsize=inf))),
                       ((2,), (dict(t_max=0.0), dict(t_max=-2.0), dict(t_max=nan), dict(t_max=inf))),
                       ((4,), (dict(step_size=0), dict(step_size=-1))),
                       ((5,), (dict(reset=-1),))):
        for kind in kinds:
            for kw in bad:
                assert _call(lib, _desc(lr_kind=kind, **kw)) == SHAPE, (kind, kw)
    for kind in (-1, 6, 100):
        assert _call(lib, _desc(lr_kind=kind)) == UNSUP, kind


def test_a_kind_does_not_read_the_fields_it_does_not_name(lib):
    """The edges pass, and what a kind does not use may hold anything (the next refusal in line -- a NULL output -- shows
    that the descriptor went through)."""
    nan = float("nan")
    for kw in (dict(), dict(N=8), dict(lr_base=0.0, lr_min=0.0), dict(lr_kind=0, gamma=nan, stepsize=nan, t_max=-1.0,
                                                                      step_size=0, reset=-5),
               dict(lr_kind=2, gamma=0.0, stepsize=0.0, step_size=0, reset=-1), dict(lr_kind=1, t_max=0.0, step_size=0),
               dict(lr_kind=3, stepsize=0.0, t_max=0.0, step_size=0, reset=-1), dict(lr_kind=4, stepsize=nan, reset=-1),
               dict(lr_kind=5, reset=0, step_size=0), dict(lr_lead=0), dict(world=6, rank=5, N=48), dict(log_len=1),
               dict(B=2 ** 31 - 1, N=2 ** 31 - 1)):
        assert _call(lib, _desc(**kw), where=None) == NULLP, kw


# ---- TrainSchedule ---------------------------------------------------------------------------------------------------------
def _opt(cls=FusedAdam, capturable=True, lr=0.01):
    return cls([torch.nn.Parameter(torch.zeros(4))], lr=lr, capturable=capturable)


def test_the_constructor_derives_configure_lrs_constants():
    opt = _opt()
    s = TrainSchedule(opt, 307, 10, 30, seed=5, lr_scheduler="TriangleLR", lr_min=1e-5, gamma=0.97, lr_step_size=4,
                      sparsify=True, trim_level=2, world=3, rank=2)
    assert (s.ticks, s.total_iterations, s.steps, s.log_len) == (10, 300, 3, 300)
    want = K.constants(0.01, 30, 10, 1, 1e-5, 0.97, 4)
    assert (s.lr_base, s.lr_min, s.gamma, s.stepsize, s.t_max, s.lr_step_size, s.reset) == \
        (want["lr_base"], want["lr_min"], want["gamma"], want["stepsize"], want["t_max"], want["step_size"], want["reset"])
    assert s.stepsize == 30 / 3 * 10 and s.t_max == 10 * 30 / 3 and s.reset == 100
    d = s.desc
    assert (d.N, d.B, d.world, d.rank, d.seed, d.num_epochs, d.trim_level, d.sparsify, d.lr_kind, d.lr_lead, d.log_len) == \
        (307, 10, 3, 2, 5, 30, 2, 1, 1, 1, 300)
    assert (d.lr_base, d.lr_min, d.gamma, d.stepsize, d.t_max, d.step_size, d.reset) == (0.01, 1e-5, 0.97, 100.0, 100.0, 4, 100)
    assert s.index.shape == (10,) and s.index.dtype == torch.int32 and s.where.shape == (4,) and s.where.dtype == torch.int64
    assert s.loss_log.shape == s.lr_log.shape == (300,) and s.loss_log.dtype == s.lr_log.dtype == torch.float32
    # the fall-backs: lr_min to the rate, two peaks, a non-integer t_max, an explicit log, torch's order
    t = TrainSchedule(_opt(FusedSGD, lr=0.5), 63, 7, 9, seed=(1 << 64) - 1, lr_scheduler="CosineAnnealingLR", lr_peaks=2,
                      lr_lead=0, log_len=4)
    assert (t.lr_min, t.steps, t.ticks, t.t_max, t.reset, t.log_len, t.desc.lr_lead) == (0.5, 5, 9, 9 * 9 / 5, 27, 4, 0)
    assert t.desc.lr_kind == 2 and t.desc.sparsify == 0 and t.desc.seed == (1 << 64) - 1 and t.loss_log.shape == (4,)
    for name, code in K.KINDS.items():
        assert TrainSchedule(opt, 50, 8, 3, seed=0, lr_scheduler=name).desc.lr_kind == code


def test_the_constructors_argument_errors():
    opt = _opt()
    with pytest.raises(TypeError, match="FusedAdam or kws_amd.FusedSGD"):
        TrainSchedule(torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))]), 50, 8, 3, seed=0)
    with pytest.raises(ValueError, match="capturable=True"):
        TrainSchedule(_opt(capturable=False), 50, 8, 3, seed=0)
    for args, kw in (((7, 8, 3), {}), ((50, 0, 3), {}), ((50, 8, 0), {}), ((50.0, 8, 3), {}), ((50, 8, 3), dict(world=0)),
                     ((50, 8, 3), dict(world=2, rank=2)), ((50, 8, 3), dict(rank=-1)), ((50, 8, 3), dict(world=7)),
                     ((50, 8, 3), dict(seed=-1)), ((50, 8, 3), dict(seed=1 << 64)), ((50, 8, 3), dict(lr_scheduler="OneCycleLR")),
                     ((50, 8, 3), dict(lr_lead=2)), ((50, 8, 3), dict(trim_level=0)), ((50, 8, 3), dict(gamma=0.0)),
                     ((50, 8, 3), dict(gamma=float("nan"))), ((50, 8, 3), dict(lr_min=-1.0)), ((50, 8, 3), dict(lr_peaks=0)),
                     ((50, 8, 3), dict(lr_step_size=0)), ((50, 8, 3), dict(log_len=0))):
        kw.setdefault("seed", 0)
        with pytest.raises(ValueError):
            TrainSchedule(opt, *args, **kw)
    with pytest.raises(TypeError):
        TrainSchedule(opt, 50, 8, 3)                                 # the seed is required
    with pytest.raises(RuntimeError, match="GPU"):
        TrainSchedule(opt, 50, 8, 3, seed=0).advance()


def test_record_files_under_the_slot_on_the_host():
    """``record`` is plain torch: it runs on CPU tensors."""
    opt = _opt(lr=0.25)
    s = TrainSchedule(opt, 50, 8, 3, seed=0)
    s.where[2] = 4
    s.record(torch.tensor(1.5))
    s.where[2] = 17
    opt.lr_t.fill_(0.125)
    s.record(torch.tensor(-2.0))
    assert s.loss_log[4] == 1.5 and s.loss_log[17] == -2.0 and s.lr_log[4] == 0.25 and s.lr_log[17] == 0.125
    assert int((s.loss_log != 0).sum()) == 2
    log = s.epoch_log([0.5, None, 0.75])
    assert [e["epoch"] for e in log] == [0, 1, 2] and log[2] == dict(epoch=2, loss=-2.0, accuracy=0.75, learning_rate=0.125)
    assert log[0]["loss"] == 0.0 and log[1]["accuracy"] is None


# ---- static scans of the new kernel source ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schedule_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_schedule.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(schedule_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), schedule_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(schedule_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), schedule_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_the_kernel_uses_no_scratch_and_no_lds():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = [r for r in resource_usage.usage(SRC) if "sched_k" in r["pretty"]]
    assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["lds"] == 0 and rows[0]["vgpr"] <= 64, rows


def test_philox_has_one_definition():
    csrc = os.path.dirname(SRC)
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and "0xD2511F53" in open(os.path.join(csrc, f)).read()]
    assert holders == ["philox.h"]
    for f in ("kernels_augment.hip", "kernels_schedule.hip"):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read()
