"""The rolling mode without a GPU: the closed-form position of tests/rolling_cases.py against a transcription of the
reference's loop, the bag permutation and its inverse, the order-free exchange against scatter-then-slice, every refusal
of the two C-ABI calls (all before any launch), the arguments of ``TrainSchedule(rolling=True)`` and ``RollingBags``, the
untouched non-rolling ``TrainSchedule``, and the static scans of DESIGN.md 4.0 on the new kernel file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import FusedAdam, FusedSGD, RNNClassifierModel, RollingBags, TrainSchedule, _lib
from tests import rolling_cases as R
from tests import schedule_cases as K
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kws_amd", "csrc")
SRC = os.path.join(CSRC, "kernels_rolling.hip")
OK, NULLP, SHAPE, UNSUP = 0, 1, 2, 7
SEED = (0xC0FFEE << 32) | 0x1234
SIZES = (6, 8, 16, 51, 800, 13000)


# ---- the position ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,world", ((1, 1), (4, 1), (8, 1), (1, 2), (4, 2), (8, 2)))
def test_the_position_is_the_reference_loops(B, world):
    checked = 0
    for N in (8, 9, 16, 17, 33, 50, 64, 100, 333, 1000):
        if N // (B * world) < 2:
            continue
        for num_epochs in range(1, 31):
            for mrl in (0, 1, 2, 5, 100):
                sched = (N, B, world, num_epochs, mrl)
                loop = list(R.literal_loop(*sched))
                ticks_full, n_short, total = R.constants(*sched)
                assert total == len(loop) == R.reference_total(*sched), sched
                assert n_short == sum(1 for e, i, fresh, zero in loop if zero), sched
                # (every iteration where the run is short, its head and tail where it is long)
                for s in (range(total) if total <= 200 else list(range(120)) + list(range(total - 80, total))):
                    assert R.position(s, *sched) == loop[s], (sched, s)
                checked += 1
    assert checked >= 150 * 3
    print("B = %d, world = %d: %d schedules" % (B, world, checked))


def test_position_spot_values_and_the_tail():
    sched = (50, 8, 1, 4, 2)                                         # short epochs of 2 and 3, then full ones of 6
    assert R.constants(*sched) == (6, 2, 17)
    want = [(0, 0, True, True), (0, 1, False, False), (1, 0, True, True), (1, 1, False, False), (1, 2, False, False),
            (2, 0, True, False)] + [(2, i, False, False) for i in range(1, 6)] + [(3, i, False, False) for i in range(6)]
    assert [R.position(s, *sched) for s in range(17)] == want
    assert R.position(-3, *sched) == want[0] and R.position(17, *sched) == (4, 0, False, False)      # past the end: full
    assert R.position((1 << 40), *sched) == (2 + ((1 << 40) - 5) // 6, ((1 << 40) - 5) % 6, False, False)
    assert R.constants(64, 8, 2, 3, 100) == (4, 2, 9) and R.constants(17, 1, 4, 30, 5) == (4, 2, 117)
    assert R.constants(4097, 1030, 1, 3, 0) == (3, 0, 9) and R.position(0, 4097, 1030, 1, 3, 0) == (0, 0, True, False)


# ---- the bag permutation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_bag_perm_is_a_bijection_and_the_inverse_inverts_it(M):
    rows, seen = np.arange(M), set()
    for s in list(range(62)) + [(1 << 33) + 5, (1 << 40)]:
        there = R.bag_perm(SEED, s, rows, M)
        back = R.bag_perm(SEED, s, rows, M, inverse=True)
        assert np.array_equal(np.sort(there), rows), (M, s)
        assert np.array_equal(back[there], rows) and np.array_equal(there[back], rows), (M, s)
        seen.add(tuple(there[:6].tolist()))
    assert len(seen) > 32                                            # (the step enters the key)
    assert R.bag_perm(SEED, 3, M - 1, M) == R.bag_perm(SEED, 3, rows, M)[M - 1]
    assert R.bag_perm(SEED, -4, 1, M) == R.bag_perm(SEED, 0, 1, M)
    # apart from the epoch order's counters under the same seed and the same counter words
    if M >= 51:
        assert not np.array_equal(R.bag_perm(SEED, 1, rows, M), K.epoch_perm(SEED, 1, rows, M))


def test_the_batchs_rows_hit_every_bag_row_about_equally_often():
    """B = 8, bag_count = 2, seed SEED, steps 0..63: each of the 16 rows is hit binomial(64, 1/2) times, mean 32,
    sigma 4.  ``rolling_cases.bag_perm`` gives a worst deviation of 7 (counts 25..37); the bound is that plus one
    sigma, 11: 2.75 sigma, which a sound shuffle exceeds on some of 16 rows about one time in fifteen and a Feistel
    network that ignored the step or favoured a half of the rows (deviation 32) never meets."""
    counts = np.zeros(16, dtype=np.int64)
    for s in range(64):
        counts[R.bag_perm(SEED, s, np.arange(8), 16)] += 1
    worst = int(np.abs(counts - 32).max())
    print("counts %d..%d, worst deviation %d" % (counts.min(), counts.max(), worst))
    assert counts.sum() == 512 and worst <= 7 + 4, counts


# ---- the exchange ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,bag_count", ((8, 2), (8, 1), (3, 2), (5, 100)))
def test_the_order_free_exchange_is_scatter_then_slice(B, bag_count):
    rng = np.random.default_rng(B * 1000 + bag_count)
    sched = (B * 6 + 2, B, 1, 4, 2)
    M, sizes = B * bag_count, (5, 4)
    oracle = R.Exchange(SEED, B, bag_count, sizes, sched)
    mixed = plain = 0
    for s in range(17):
        states = [rng.integers(1, 1 << 32, (B, h), dtype=np.uint32) for h in sizes]
        before = [bag.copy() for bag in oracle.bags]
        _, _, fresh, zero = R.position(s, *sched)
        h0 = oracle.step(s, states)
        if fresh:
            assert all((h == 0).all() for h in h0) and (not zero or all((bag == 0).all() for bag in oracle.bags))
            assert zero or all(np.array_equal(a, b) for a, b in zip(before, oracle.bags))
            continue
        for l in range(2):
            got, from_state = R.h0_by_inverse(SEED, s, B, M, states[l], before[l])
            assert np.array_equal(got, h0[l]), (s, l)
            # the rows of the bag that no batch row lands on are the ones it keeps
            hit = np.zeros(M, dtype=bool)
            hit[R.bag_perm(SEED, s, np.arange(B), M)] = True
            assert np.array_equal(hit[:B], from_state) and np.array_equal(oracle.bags[l][~hit], before[l][~hit])
        plain += 1
        mixed += bool(from_state.any() and not from_state.all())
    assert plain == 14 and (bag_count > 1 or mixed == 0)
    if (B, bag_count) == (8, 2):
        assert 2 * mixed >= plain, (mixed, plain)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return S.built_library()


ONE = C.c_void_p(256)                          # a non-NULL pointer that no refused call may touch
NULL3 = (C.c_void_p * 3)(None, None, None)


def _three(n=3):
    return (C.c_void_p * 3)(*([256] * n + [None] * (3 - n)))


def _desc(**kw):
    f = dict(N=50, B=8, world=1, rank=0, seed=SEED, num_epochs=4, trim_level=2, sparsify=1, lr_kind=0, lr_lead=1,
             reserved=0, log_len=17, lr_base=0.01, lr_min=0.001, gamma=0.97, stepsize=6.0, t_max=6.0, step_size=1, reset=6)
    f.update(kw)
    return _lib.ScheduleDesc(**f)


def _roll(H=(256, 128, 100), **kw):
    f = dict(max_rolling_length=2, bag_count=2, layers=len(H), reserved=0)
    f.update(kw)
    return _lib.RollingDesc(f["max_rolling_length"], f["bag_count"], f["layers"], f["reserved"],
                            (C.c_int32 * 4)(*(tuple(H) + (0,) * (4 - len(H)))))


def _sched(lib, d=None, r=None, step=ONE, index=ONE, lr=ONE, iht=ONE, where=ONE, no_desc=False, no_roll=False):
    d, r = _desc() if d is None else d, _roll() if r is None else r
    return lib.fastgrnn_hip_train_schedule_rolling(None if no_desc else C.byref(d), None if no_roll else C.byref(r),
                                                   step, index, lr, iht, where, None)


def _xchg(lib, d=None, r=None, step=ONE, state=None, bag=None, h0=None, no_desc=False, no_roll=False):
    d, r = _desc() if d is None else d, _roll() if r is None else r
    arrays = [None if a is False else C.byref(_three() if a is None else a) for a in (state, bag, h0)]
    return lib.fastgrnn_hip_rolling_exchange(None if no_desc else C.byref(d), None if no_roll else C.byref(r), step,
                                             *arrays, None)


def test_the_symbols_the_struct_and_the_header(lib):
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    for name in ("fastgrnn_hip_train_schedule_rolling", "fastgrnn_hip_rolling_exchange"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header
    assert "fastgrnn_rolling_desc;" in header and C.sizeof(_lib.RollingDesc) == 32 and _lib.RollingDesc.H.offset == 16
    assert lib.fastgrnn_hip_abi_version() == 1 and C.sizeof(_lib.ScheduleDesc) == 112
    assert "kernels_rolling.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_calls_refuse_null_pointers(lib):
    assert _sched(lib, no_desc=True) == NULLP and _sched(lib, no_roll=True) == NULLP
    for kw in (dict(step=None), dict(index=None), dict(lr=None), dict(where=None), dict(iht=None)):
        assert _sched(lib, **kw) == NULLP, kw
    assert _sched(lib, _desc(sparsify=0, lr_kind=9), iht=None) == UNSUP      # (no phase pointer without sparsify)
    assert _xchg(lib, no_desc=True) == NULLP and _xchg(lib, no_roll=True) == NULLP and _xchg(lib, step=None) == NULLP
    for which in ("state", "bag", "h0"):
        assert _xchg(lib, **{which: False}) == NULLP, which
        assert _xchg(lib, **{which: NULL3}) == NULLP, which
        assert _xchg(lib, **{which: _three(2)}) == NULLP, which               # the third layer's entry
    # the entries past `layers` are not read (the next refusal in line shows that the arrays went through)
    assert _xchg(lib, r=_roll(H=(256, 128)), state=_three(2), bag=_three(2), h0=_three(2), step=None) == NULLP
    assert _xchg(lib, r=_roll(H=(256, 128), bag_count=0), state=_three(2), bag=_three(2), h0=_three(2)) == SHAPE


def test_the_calls_refuse_bad_shapes(lib):
    nan = float("nan")
    both = (dict(d=dict(B=0)), dict(d=dict(world=0)), dict(d=dict(rank=1)), dict(d=dict(N=7)), dict(d=dict(num_epochs=0)),
            dict(d=dict(trim_level=0)), dict(d=dict(log_len=0)), dict(d=dict(lr_lead=2)), dict(d=dict(lr_base=nan)),
            dict(d=dict(lr_min=-1.0)), dict(d=dict(lr_kind=1, gamma=0.0)), dict(d=dict(lr_kind=1, stepsize=nan)),
            dict(d=dict(lr_kind=2, t_max=0.0)), dict(d=dict(lr_kind=4, step_size=0)), dict(d=dict(lr_kind=5, reset=-1)),
            # ticks_full < 2
            dict(d=dict(N=8)), dict(d=dict(N=15)), dict(d=dict(N=31, world=2)), dict(d=dict(N=2 ** 31 - 1, B=2 ** 30)),
            dict(r=dict(max_rolling_length=-1)), dict(r=dict(bag_count=0)), dict(r=dict(bag_count=-100)),
            dict(d=dict(N=2 ** 31 - 1, B=1 << 20), r=dict(bag_count=1 << 11)),
            dict(d=dict(N=2 ** 31 - 1, B=1 << 16), r=dict(bag_count=1 << 15)))
    for kw in both:
        d, r = _desc(**kw.get("d", {})), _roll(**kw.get("r", {}))
        assert _sched(lib, d, r) == SHAPE, kw
        assert _xchg(lib, d, r) == SHAPE, kw
    for kind in (-1, 6):
        assert _sched(lib, _desc(lr_kind=kind)) == UNSUP and _xchg(lib, _desc(lr_kind=kind)) == UNSUP
    # the layers are the exchange's alone
    for kw in (dict(layers=0), dict(layers=4), dict(layers=-1), dict(H=(256, 0, 100)), dict(H=(0,)), dict(H=(256, -4))):
        assert _xchg(lib, r=_roll(**kw)) == SHAPE, kw
        assert _sched(lib, r=_roll(**kw), where=None) == NULLP, kw             # (not read there: the next refusal)
    # the edges pass (the next refusal in line -- a NULL step -- shows that the descriptors went through)
    for kw in (dict(d=dict(N=16)), dict(d=dict(N=32, world=2, rank=1)), dict(r=dict(max_rolling_length=0)),
               dict(r=dict(max_rolling_length=2 ** 31 - 1)), dict(r=dict(bag_count=1)),
               dict(d=dict(N=2 ** 31 - 1, B=1 << 20), r=dict(bag_count=(1 << 11) - 1)), dict(r=dict(H=(1,))),
               dict(r=dict(H=(256, 33), layers=2)), dict(r=dict(H=(256, 0, 0), layers=1))):
        d, r = _desc(**kw.get("d", {})), _roll(**kw.get("r", {}))
        assert _sched(lib, d, r, step=None) == NULLP, kw
        assert _xchg(lib, d, r, step=None) == NULLP, kw


# ---- TrainSchedule and RollingBags -----------------------------------------------------------------------------------------
def _opt(cls=FusedAdam, lr=0.01):
    return cls([torch.nn.Parameter(torch.zeros(4))], lr=lr, capturable=True)


def test_the_non_rolling_schedule_is_untouched():
    """The constructor calls of tests/test_schedule_cpu.py: the descriptor's bytes are those of the struct filled in by
    hand with the values that file states, and the attributes that the rolling mode redefines keep their meaning."""
    opt = _opt()
    s = TrainSchedule(opt, 307, 10, 30, seed=5, lr_scheduler="TriangleLR", lr_min=1e-5, gamma=0.97, lr_step_size=4,
                      sparsify=True, trim_level=2, world=3, rank=2)
    want = _lib.ScheduleDesc(307, 10, 3, 2, 5, 30, 2, 1, 1, 1, 0, 300, 0.01, 1e-5, 0.97, 100.0, 100.0, 4, 100)
    assert bytes(s.desc) == bytes(want) and not s.rolling and not hasattr(s, "rolling_desc")
    assert (s.ticks, s.full_ticks, s.n_short, s.total_iterations, s.log_len) == (10, 10, 0, 300, 300)
    assert isinstance(s.ticks, int) and isinstance(s.reset, int)
    t = TrainSchedule(_opt(FusedSGD, lr=0.5), 63, 7, 9, seed=(1 << 64) - 1, lr_scheduler="CosineAnnealingLR", lr_peaks=2,
                      lr_lead=0, log_len=4)
    want = _lib.ScheduleDesc(63, 7, 1, 0, (1 << 64) - 1, 9, 15, 0, 2, 0, 0, 4, 0.5, 0.5, 1.0, 9 / 5 * 9, 9 * 9 / 5, 1, 27)
    assert bytes(t.desc) == bytes(want) and (t.ticks, t.t_max, t.stepsize) == (9, 9 * 9 / 5, 9 / 5 * 9)
    for name, code in K.KINDS.items():
        u = TrainSchedule(opt, 50, 8, 3, seed=0, lr_scheduler=name)
        want = _lib.ScheduleDesc(50, 8, 1, 0, 0, 3, 15, 0, code, 1, 0, 18, 0.01, 0.01, 1.0, 6.0, 6.0, 1, 6)
        assert bytes(u.desc) == bytes(want), name
    # the keywords of the rolling mode are not read without it
    v = TrainSchedule(opt, 50, 8, 3, seed=0, max_rolling_length=-7, bag_count=0)
    want = _lib.ScheduleDesc(50, 8, 1, 0, 0, 3, 15, 0, 0, 1, 0, 18, 0.01, 0.01, 1.0, 6.0, 6.0, 1, 6)
    assert bytes(v.desc) == bytes(want) and v.ticks == 6
    for step in (0, 5, 6, 17, 40, -2):
        assert v.position(step) == K.position(step, 50, 8)[:2] and v.epoch_end(step) == ((max(step, 0) + 1) % 6 == 0)
    assert [v.epoch_start(e) for e in range(4)] == [0, 6, 12, 18]


def test_the_rolling_constructor_follows_the_reference():
    opt = _opt()
    s = TrainSchedule(opt, 50, 8, 4, seed=SEED, rolling=True, max_rolling_length=2, bag_count=2,
                      lr_scheduler="CosineAnnealingLR", lr_min=1e-5)
    assert s.rolling and (s.full_ticks, s.n_short, s.total_iterations, s.log_len) == (6, 2, 17, 17)
    assert s.ticks == 17 / 4 and s.stepsize == 4 / 3 * (17 / 4) and s.t_max == 17 / 3 and s.reset == int(4 * (17 / 4) / 3)
    assert (s.desc.N, s.desc.B, s.desc.num_epochs, s.desc.log_len, s.desc.t_max) == (50, 8, 4, 17, 17 / 3)
    r = s.rolling_desc
    assert (r.max_rolling_length, r.bag_count, r.layers) == (2, 2, 0)
    assert [s.epoch_start(e) for e in range(5)] == [0, 2, 5, 11, 17]
    assert [i for i in range(17) if s.epoch_end(i)] == [1, 4, 10, 16]
    d = TrainSchedule(opt, 64, 8, 3, seed=1, rolling=True, world=2, rank=1)       # the defaults: the reference's 100, 100
    assert (d.max_rolling_length, d.bag_count, d.n_short, d.total_iterations) == (100, 100, 2, 9)
    for sched in ((50, 8, 1, 4, 2), (64, 8, 2, 3, 100), (17, 1, 4, 30, 5), (4097, 1030, 1, 3, 0), (1000, 4, 1, 30, 100)):
        N, B, world, num_epochs, mrl = sched
        t = TrainSchedule(opt, N, B, num_epochs, seed=0, rolling=True, max_rolling_length=mrl, world=world)
        assert (t.full_ticks, t.n_short, t.total_iterations) == R.constants(*sched)
        for i in list(range(-1, min(t.total_iterations, 300) + 4)) + [t.total_iterations - 1, 1 << 40]:
            assert t.position(i) == R.position(i, *sched)[:2], (sched, i)
            assert t.epoch_end(i) == (R.position(max(i, 0) + 1, *sched)[1] == 0), (sched, i)
    # the log reads the true last slot of every epoch
    s.loss_log.copy_(torch.arange(17.0))
    assert [e["loss"] for e in s.epoch_log()] == [1.0, 4.0, 10.0, 16.0]


def test_the_rolling_argument_errors():
    opt = _opt()
    for args, kw in (((8, 8, 3), {}), ((15, 8, 3), {}), ((31, 8, 3), dict(world=2)), ((50, 8, 3), dict(max_rolling_length=-1)),
                     ((50, 8, 3), dict(max_rolling_length=2.0)), ((50, 8, 3), dict(bag_count=0)),
                     ((50, 8, 3), dict(bag_count=True)), ((50, 8, 3), dict(bag_count=1 << 29)),
                     ((50, 8, 3), dict(max_rolling_length=1 << 31))):
        with pytest.raises(ValueError):
            TrainSchedule(opt, *args, seed=0, rolling=True, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        TrainSchedule(opt, 50, 8, 3, seed=0, rolling=True).advance()

    def model(layers, hidden):
        return RNNClassifierModel("FastGRNNCUDA", 32, layers, hidden, [None] * layers, [None] * layers, [1.0] * layers,
                                  [1.0] * layers, "sigmoid", "tanh", num_classes=12, device="cpu")

    m = model(2, [128, 100])
    sched = TrainSchedule(opt, 50, 8, 4, seed=SEED, rolling=True, max_rolling_length=2, bag_count=3)
    bags = RollingBags(m, sched)
    assert [tuple(t.shape) for t in bags.state] == [tuple(t.shape) for t in bags.h0] == [(8, 128), (8, 100)]
    assert [tuple(t.shape) for t in bags.bag] == [(24, 128), (24, 100)] and len(bags.tensors()) == 6
    assert all(t.dtype == torch.float32 and not t.any() for t in bags.tensors())
    assert (bags.desc.max_rolling_length, bags.desc.bag_count, bags.desc.layers, list(bags.desc.H)) == (2, 3, 2, [128, 100, 0, 0])
    assert sched.rolling_desc.layers == 0                            # (the schedule's own descriptor is not written)
    with pytest.raises(ValueError, match="rolling=True"):
        RollingBags(m, TrainSchedule(opt, 50, 8, 4, seed=SEED))
    with pytest.raises(ValueError, match="rolling=True"):
        RollingBags(m, None)
    with pytest.raises(ValueError, match="1 to 3 layers"):
        RollingBags(model(4, [16, 16, 16, 16]), sched)
    with pytest.raises(RuntimeError, match="GPU"):
        bags.exchange()
    m.hidden_states = [torch.full((8, 128), 2.0), torch.full((8, 100), 3.0)]
    bags.commit()                                                    # (plain torch: runs on CPU tensors)
    assert float(bags.state[0].min()) == 2.0 and float(bags.state[1].max()) == 3.0


# ---- static scans of the new kernel source ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rolling_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_rolling.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=CSRC, capture_output=True)
    return out


def test_war_scan_clean(rolling_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), rolling_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(rolling_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), rolling_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_the_kernels_use_no_scratch_no_lds_and_no_atomics(rolling_asm):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = {r["pretty"]: r for r in resource_usage.usage(SRC)}
    assert sorted(rows) == ["roll_exchange_k", "roll_sched_k"], rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["lds"] == 0 and r["vgpr"] <= 128, r
    asm = open(rolling_asm).read()
    assert "global_atomic" not in asm and "ds_write" not in asm and "ds_read" not in asm
    assert "global_load_dwordx4" in asm and "global_store_dwordx4" in asm      # the 16-byte rows


def test_the_shared_code_has_one_definition():
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    assert [f for f, t in text.items() if "0xD2511F53" in t] == ["philox.h"]
    for f in ("kernels_rolling.hip", "kernels_schedule.hip"):
        assert '#include "philox.h"' in text[f] and '#include "schedule_common.h"' in text[f]
    for name in ("uint32_t feistel_pass(", "double lr_of("):
        assert [f for f, t in text.items() if name in t] == ["schedule_common.h"], name
