"""The rolling mode on the GPU: the rolling schedule kernel against the numpy restatement of tests/rolling_cases.py at every
iteration of four runs (``index`` bit for bit between canaries, ``where`` with its fresh and zero bits and the IHT phase
exactly, the six learning-rate kinds within ``schedule_cases.lr_bound``), the bag exchange against the stateful
scatter-then-slice oracle bit for bit (between canaries, aligned and not), one captured ``advance + exchange + commit``
following the step scalar, and a whole rolling ``fit_audio`` run from one graph against the eager loop and against a
host-driven twin that does the exchange in torch index ops."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import mfcc_cases as M
from tests import rolling_cases as R
from tests import schedule_cases as K
from tests import support as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import (AudioAugment, FusedAdam, GraphedStep, MFCCFrontend, RNNClassifierModel, RollingBags,
                         TrainSchedule, iht_phase)
DEV = torch.device("cuda:0")
SEED = (0xC0FFEE << 32) | 0x1234
# N, B, world, rank, num_epochs, max_rolling_length
CASES = ((50, 8, 1, 0, 4, 2), (64, 8, 2, 1, 3, 100), (17, 1, 4, 3, 30, 5), (4097, 1030, 1, 0, 3, 0))
TRIM, PAD, CANARY = 2, 64, -1234567
LR, LR_MIN, GAMMA, STEP_SIZE = 0.01, 1e-5, 0.97, 4


def _opt(lr=LR):
    return FusedAdam([torch.nn.Parameter(torch.zeros(4, device=DEV))], lr=lr, capturable=True)


# ---- 1. the schedule kernel against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,world,rank,num_epochs,mrl", CASES)
def test_the_rolling_schedule_kernel_equals_the_oracle(N, B, world, rank, num_epochs, mrl):
    sched_key = (N, B, world, num_epochs, mrl)
    ticks_full, n_short, total = R.constants(*sched_key)
    opt = _opt()
    scheds = {name: TrainSchedule(opt, N, B, num_epochs, seed=SEED, lr_scheduler=name, lr_min=LR_MIN, gamma=GAMMA,
                                  lr_step_size=STEP_SIZE, sparsify=True, trim_level=TRIM, world=world, rank=rank,
                                  lr_lead=(0 if name == "StepLR" else 1), rolling=True, max_rolling_length=mrl, bag_count=2)
              for name in K.KINDS}
    wholes = {}
    for name, sched in scheds.items():                           # ``index`` between two canary stretches
        assert (sched.full_ticks, sched.n_short, sched.total_iterations) == (ticks_full, n_short, total)
        wholes[name] = torch.full((B + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
        sched.index = wholes[name][PAD:PAD + B]
    # configure_lr's constants from the reference's fractional ticks; T_max is total_iterations / cycles there
    kw = dict(K.constants(LR, num_epochs, total / num_epochs, 1, LR_MIN, GAMMA, STEP_SIZE), t_max=total / 3)
    worst, flags = 0.0, set()
    for s in list(range(total + 4)) + [-1, 1 << 40]:
        opt.step_t.fill_(s)
        epoch, i_batch, fresh, zero = R.position(s, *sched_key)
        q = (i_batch * world + rank) * B + np.arange(B, dtype=np.int64)
        want_index = K.epoch_perm(SEED, epoch, q, N).astype(np.int32)
        flags.add((fresh, zero))
        for name, sched in scheds.items():
            opt.iht_t.fill_(7)
            sched.where.fill_(-1)
            assert sched.advance() is sched.index
            whole = wholes[name].cpu().numpy()
            assert np.array_equal(whole[PAD:PAD + B], want_index), (name, s)
            assert (whole[:PAD] == CANARY).all() and (whole[PAD + B:] == CANARY).all(), (name, s)
            assert sched.where.tolist() == [epoch, i_batch, min(max(s, 0), total - 1), int(fresh) | int(zero) << 1], (name, s)
            assert int(opt.iht_t) == K.phase(epoch, num_epochs, i_batch, TRIM), (name, s)
            want = K.lr_at(name, max(s, 0) + sched.lr_lead, **kw)
            got = float(opt.lr_t)
            worst = max(worst, abs(got - want) / K.lr_bound(LR)(want))
            assert abs(got - want) <= K.lr_bound(LR)(want), (name, s, got, want)
    assert flags == ({(True, True), (True, False), (False, False)} if n_short else {(True, False), (False, False)})
    print("%s: %d iterations, largest lr error %.3f of its bound" % (sched_key, total, worst))


# ---- 2. the exchange against the stateful oracle ---------------------------------------------------------------------------
class _Layers(torch.nn.Module):
    """What ``RollingBags`` reads of a model: the layers' sizes and a parameter's device."""

    def __init__(self, sizes):
        super().__init__()
        self.hidden_units_list, self.num_layers = list(sizes), len(sizes)
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.hidden_states = [None] * len(sizes)


def _guarded(rows, h, offset):
    """``[rows, h]`` fp32 zeros between two canary stretches, ``offset`` floats off a 256-byte boundary."""
    whole = torch.full((rows * h + 2 * PAD + offset,), float(CANARY), dtype=torch.float32, device=DEV)
    view = whole[PAD + offset:PAD + offset + rows * h].view(rows, h)
    view.zero_()
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return whole, view


def _canaries_intact(whole, rows, h, offset):
    w = whole.cpu().numpy()
    return (w[:PAD + offset] == float(CANARY)).all() and (w[PAD + offset + rows * h:] == float(CANARY)).all()


def _states(rng, B, h):
    """Random bit patterns (NaNs with payloads, infinities and denormals among them) with the special values placed."""
    a = rng.integers(0, 1 << 32, (B, h), dtype=np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32)
    flat = a.reshape(-1)
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return a


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B,bag_count,sizes,offset", ((8, 2, (256, 128, 100), 0), (8, 1, (256, 128, 100), 0),
                                                       (3, 2, (256, 128, 100), 0), (130, 100, (256, 33), 0),
                                                       (8, 2, (256, 128, 100), 1), (130, 100, (256, 33), 1)))
def test_the_exchange_equals_scatter_then_slice_bit_for_bit(B, bag_count, sizes, offset):
    N = 50 if B == 8 else 6 * B + 2                              # six batches: short epochs of 2 and 3, full ones of 6
    sched_key = (N, B, 1, 4, 2)
    assert R.constants(*sched_key) == (6, 2, 17)
    opt = _opt()
    sched = TrainSchedule(opt, N, B, 4, seed=SEED, rolling=True, max_rolling_length=2, bag_count=bag_count)
    bags = RollingBags(_Layers(sizes), sched)
    Mrows = B * bag_count
    guards = {}
    for l, h in enumerate(sizes):
        guards["bag", l], bags.bag[l] = _guarded(Mrows, h, offset)
        guards["h0", l], bags.h0[l] = _guarded(B, h, offset)
        guards["state", l], bags.state[l] = _guarded(B, h, offset)
    bags.bind()
    oracle = R.Exchange(SEED, B, bag_count, sizes, sched_key)
    rng = np.random.default_rng(7 * B + bag_count)
    mixed = plain = 0
    for s in range(17):
        states = [_states(rng, B, h) for h in sizes]
        for l, st in enumerate(states):
            bags.state[l].view(torch.int32).copy_(torch.from_numpy(st.view(np.int32)).to(DEV))
        before = oracle.bags[0].copy()
        opt.step_t.fill_(s)
        for h0 in bags.h0:
            h0.fill_(3.0)                                            # (a fresh step has to write its zeros)
        assert bags.exchange() is bags.h0 and all(a is b for a, b in zip(bags.model.hidden_states, bags.h0))
        want = oracle.step(s, states)
        for l, h in enumerate(sizes):
            assert np.array_equal(_bits(bags.h0[l]), want[l]), (s, l, "h0")
            assert np.array_equal(_bits(bags.bag[l]), oracle.bags[l]), (s, l, "bag")
            assert np.array_equal(_bits(bags.state[l]), states[l]), (s, l, "state")
            assert _canaries_intact(guards["bag", l], Mrows, h, offset), (s, l)
            assert _canaries_intact(guards["h0", l], B, h, offset) and _canaries_intact(guards["state", l], B, h, offset)
        if not R.position(s, *sched_key)[2]:
            _, from_state = R.h0_by_inverse(SEED, s, B, Mrows, states[0], before)
            plain += 1
            mixed += bool(from_state.any() and not from_state.all())
            assert bag_count > 1 or from_state.all()                 # one bag row per batch row: all from state
    assert plain == 14
    if (B, bag_count) == (8, 2):
        # coverage: both kinds of h0 row, from state and from the bag, in one launch on at least half of the steps
        assert 2 * mixed >= plain, (mixed, plain)
        both = 0
        for s in range(64):
            src = R.bag_perm(SEED, s, np.arange(8), 16, inverse=True)
            both += bool((src < 8).any() and (src >= 8).any())
        assert both == 62
    # past the run's end and below zero no write leaves the buffers either
    for s in (17, 1 << 40, -5):
        opt.step_t.fill_(s)
        bags.exchange()
    torch.cuda.synchronize()
    for (what, l), whole in guards.items():
        assert _canaries_intact(whole, Mrows if what == "bag" else B, sizes[l], offset), (what, l)


# ---- 3. one captured exchange follows the step scalar ----------------------------------------------------------------------
def test_a_captured_advance_exchange_commit_follows_the_step_scalar():
    opt = _opt()
    sched = TrainSchedule(opt, 50, 8, 4, seed=SEED, lr_scheduler="TriangleLR", lr_min=LR_MIN, gamma=GAMMA, sparsify=True,
                          trim_level=TRIM, rolling=True, max_rolling_length=2, bag_count=2)
    bags = RollingBags(_Layers((256, 100)), sched)
    gen = torch.Generator(device="cpu").manual_seed(3)
    for t in bags.tensors():
        t.copy_(torch.randn(t.shape, generator=gen))
    start = [t.clone() for t in bags.tensors()]
    moves = [torch.randn(t.shape, generator=gen).to(DEV) for t in bags.h0]
    held = lambda: [t.clone() for t in [sched.index, opt.lr_t, opt.iht_t, sched.where] + bags.tensors()]

    def fn():
        sched.advance()
        bags.exchange()
        for h0, move in zip(bags.h0, moves):
            h0.add_(move)                                            # (stands for the training step between the two)
        bags.commit()

    def restore():
        for t, v in zip(bags.tensors(), start):
            t.copy_(v)

    graphed = GraphedStep(fn)
    steps = (0, 1, 5, 4, 16)
    restore()
    eager = []
    for s in steps:
        opt.step_t.fill_(s)
        fn()
        eager.append(held())
    restore()
    for s, want in zip(steps, eager):
        opt.step_t.fill_(s)                                          # the host writes the scalar, the graph follows
        graphed()
        torch.cuda.synchronize()
        for i, (got, w) in enumerate(zip(held(), want)):
            assert S.bits_equal(got, w), (s, i)
    assert [int(e[3][3]) for e in eager] == [3, 0, 1, 0, 0] and len({tuple(e[0].tolist()) for e in eager}) == 5
    assert not S.bits_equal(eager[1][-1], eager[3][-1])              # (h0 moves from step to step)


# ---- 4. a whole rolling run from one graph ---------------------------------------------------------------------------------
N_CLIPS, L_MAX, BATCH, NUM_EPOCHS, MRL, BAG_COUNT = 50, 4000, 8, 4, 2, 2
RUN = (N_CLIPS, BATCH, 1, NUM_EPOCHS, MRL)


@functools.lru_cache(maxsize=None)
def _bank():
    rng = np.random.default_rng(11)
    lengths = rng.integers(1280, L_MAX + 1, N_CLIPS).astype(np.int32)
    lengths[:2] = (1280, L_MAX)
    bank = np.zeros((N_CLIPS, L_MAX), dtype=np.float32)
    for c, n in enumerate(lengths):
        bank[c, :n] = M.speech_like(100 + c, int(n)) if c % 2 else M.noise(200 + c, int(n), 0.2)
    labels = rng.integers(0, 12, N_CLIPS)
    noises = [torch.from_numpy(M.noise(300, 700, 0.3)), torch.from_numpy(M.noise(301, 5000, 0.1))]
    aug = AudioAugment(p_augment=0.75, max_shift=400, gain=(0.5, 1.5), p_noise=0.5, noise_gain=(0.05, 0.3), seed=SEED,
                       noises=noises, device=DEV)
    fe = MFCCFrontend(n_mfcc=16, feature_type="delta", max_len=1 + L_MAX // 160, device=DEV)
    return torch.from_numpy(bank).to(DEV), torch.from_numpy(lengths).to(DEV), torch.from_numpy(labels).to(DEV), aug, fe


def _trainer(start):
    model = copy.deepcopy(start)
    opt = FusedAdam(model.parameters(), lr=LR, capturable=True)
    assert opt.register_iht(model) == 4
    sched = TrainSchedule(opt, N_CLIPS, BATCH, NUM_EPOCHS, seed=SEED, lr_scheduler="StepLR", gamma=0.5, lr_step_size=6,
                          sparsify=True, trim_level=TRIM, rolling=True, max_rolling_length=MRL, bag_count=BAG_COUNT)
    return model, opt, sched


def _same_run(a, b, what):
    (ma, oa, sa), (mb, ob, sb) = a, b
    for (name, p), q in zip(ma.named_parameters(), mb.parameters()):
        S.assert_same_bits(p.detach(), q.detach(), "%s: %s" % (what, name))
        for k in ("exp_avg", "exp_avg_sq"):
            S.assert_same_bits(oa.state[p][k], ob.state[q][k], "%s: %s of %s" % (what, k, name))
    for rnn_a, rnn_b in zip(ma.rnn_list, mb.rnn_list):
        for pa, pb in ((rnn_a.W, rnn_b.W), (rnn_a.U, rnn_b.U)):
            S.assert_same_bits(oa.support(pa), ob.support(pb), what + ": a support mask")
    assert int(oa.step_t) == int(ob.step_t) == sa.total_iterations == 17


def test_rolling_fit_audio_from_one_graph_equals_the_eager_loop_and_a_host_driven_twin():
    bank, lengths, labels, aug, fe = _bank()
    torch.manual_seed(5)
    start = RNNClassifierModel("FastGRNNCUDA", 32, 2, [128, 128], [None, None], [None, None], [0.5, 0.5], [0.5, 0.5],
                               "sigmoid", "tanh", num_classes=12, device=DEV)
    val = [(fe(bank[:10], lengths[:10]).transpose(0, 1).contiguous(), labels[:10])]
    graphed, eager, twin = _trainer(start), _trainer(start), _trainer(start)
    g_bags, e_bags = RollingBags(graphed[0], graphed[2]), RollingBags(eager[0], eager[2])
    log = graphed[0].fit_audio(bank, lengths, labels, fe, aug, graphed[1], graphed[2], graph=True, validation=lambda: val,
                               bags=g_bags)
    e_log = eager[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], eager[2], graph=False, bags=e_bags)
    sched = graphed[2]
    assert (sched.full_ticks, sched.n_short, sched.total_iterations) == (6, 2, 17)
    # (the graph run validated after every epoch, the eager one never: the carried state does not see it)
    _same_run(graphed, eager, "graph against eager")
    S.assert_same_bits(sched.loss_log, eager[2].loss_log, "loss_log, graph against eager")
    S.assert_same_bits(sched.lr_log, eager[2].lr_log, "lr_log, graph against eager")
    for a, b in zip(g_bags.tensors(), e_bags.tensors()):
        S.assert_same_bits(a, b, "bags and states, graph against eager")
    # the twin: position, index and phase from the oracle, the exchange in torch index ops, the step called by hand
    model, opt, _ = twin
    sizes, rows = (128, 128), BATCH * BAG_COUNT
    bag = [torch.zeros(rows, h, device=DEV) for h in sizes]
    hs, losses, carried, plain = None, [], 0, 0
    for s in range(17):
        epoch, i_batch, fresh, zero = R.position(s, *RUN)
        q = i_batch * BATCH + np.arange(BATCH, dtype=np.int64)
        index = torch.from_numpy(K.epoch_perm(SEED, epoch, q, N_CLIPS).astype(np.int32)).to(DEV)
        opt.lr_t.copy_(sched.lr_log[s:s + 1])
        if zero:
            for b in bag:
                b.zero_()
        if fresh:
            hs = [torch.zeros(BATCH, h, device=DEV) for h in sizes]
        else:
            idx = torch.from_numpy(R.bag_perm(SEED, s, np.arange(BATCH), rows)).to(DEV)
            for l in range(2):
                bag[l][idx] = hs[l]
                hs[l] = bag[l][:BATCH].clone()
            plain += 1
            carried += all(bool(h.any()) for h in hs)
        model.hidden_states = list(hs)
        losses.append(model.train_step_audio(bank, lengths, labels, index, fe, aug, opt,
                                             iht=iht_phase(epoch, NUM_EPOCHS, i_batch, TRIM)))
        hs = [h.clone() for h in model.hidden_states]
    _same_run(graphed, twin, "graph against the host-driven twin")
    S.assert_same_bits(sched.loss_log, torch.stack(losses).reshape(-1), "loss_log against the twin's losses")
    for l in range(2):
        S.assert_same_bits(g_bags.bag[l], bag[l], "bag %d against the twin's" % l)
        S.assert_same_bits(g_bags.state[l], hs[l], "state %d against the twin's" % l)
    assert plain == 14 and 2 * carried >= plain, (carried, plain)       # the carried state is real
    loss_log, lr_log = sched.loss_log.tolist(), sched.lr_log.tolist()
    assert all(np.isfinite(loss_log)) and len(set(loss_log)) == 17
    for s in range(17):
        want = K.lr_at("StepLR", s + 1, LR, gamma=0.5, step_size=6)
        assert abs(lr_log[s] - want) <= K.lr_bound(LR)(want), (s, lr_log[s], want)
    # the returned log: four epochs, ending at slots 1, 4, 10 and 16
    assert [e["epoch"] for e in log] == [0, 1, 2, 3] and [e["loss"] for e in log] == [loss_log[i] for i in (1, 4, 10, 16)]
    assert [e["learning_rate"] for e in log] == [lr_log[i] for i in (1, 4, 10, 16)]
    assert all(isinstance(e["accuracy"], float) and 0.0 <= e["accuracy"] <= 1.0 for e in log)
    assert [e["loss"] for e in e_log] == [e["loss"] for e in log] and all(e["accuracy"] is None for e in e_log)
    # fit_audio builds the bags itself where none are passed, and refuses another run's
    with pytest.raises(ValueError, match="bags"):
        graphed[0].fit_audio(bank, lengths, labels, fe, aug, graphed[1], sched, bags=e_bags)
    again = _trainer(start)
    again[0].fit_audio(bank, lengths, labels, fe, aug, again[1], again[2], graph=False)
    _same_run(again, eager, "bags built by fit_audio")
