"""The device-side schedule on the GPU: the kernel against the numpy restatement of tests/schedule_cases.py (``index`` bit
for bit between canaries, ``where`` and the IHT phase exactly, the learning rate within ``max(1 fp32 ulp, 1e-12 lr_base)``
of the Python-double formula for all six kinds), one captured ``advance`` following the step scalar, a whole ``fit_audio``
run replayed from one graph against the eager loop and against a host-driven twin, and the ranks' shards."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import mfcc_cases as M
from tests import schedule_cases as K
from tests import support as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import (AudioAugment, FusedAdam, FusedSGD, GraphedStep, MFCCFrontend, RNNClassifierModel, TrainSchedule,
                         iht_phase)
DEV = torch.device("cuda:0")
SEED = (0xC0FFEE << 32) | 0x1234
CASES = ((50, 8, 1, 0), (64, 8, 2, 1), (8, 8, 1, 0), (17, 1, 4, 3), (4097, 1030, 3, 2))
NUM_EPOCHS, TRIM, PAD, CANARY = 3, 2, 64, -1234567
LR, LR_MIN, GAMMA, STEP_SIZE = 0.01, 1e-5, 0.97, 4


def _opt(cls=None, lr=LR):
    return (cls or FusedAdam)([torch.nn.Parameter(torch.zeros(4, device=DEV))], lr=lr, capturable=True)


def _guard(sched):
    """Move the schedule's ``index`` between two canary stretches; returns the whole buffer."""
    whole = torch.full((sched.batch_size + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    sched.index = whole[PAD:PAD + sched.batch_size]
    return whole


def _close(got, want, lr_base):
    return abs(float(got) - want) <= K.lr_bound(lr_base)(want)


# ---- 1. the kernel against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,world,rank", CASES)
def test_the_kernel_equals_the_oracle(N, B, world, rank):
    ticks = N // (B * world)
    steps = sorted({0, 1, ticks - 1, ticks, 3 * ticks + 1, (1 << 33) + 5})
    opt = _opt()
    scheds = {name: TrainSchedule(opt, N, B, NUM_EPOCHS, seed=SEED, lr_scheduler=name, lr_min=LR_MIN, gamma=GAMMA,
                                  lr_step_size=STEP_SIZE, sparsify=True, trim_level=TRIM, world=world, rank=rank,
                                  lr_lead=(0 if name == "StepLR" else 1))
              for name in K.KINDS}
    zero_min = TrainSchedule(opt, N, B, NUM_EPOCHS, seed=SEED, lr_scheduler="CosineAnnealingLR", world=world, rank=rank)
    zero_min.desc.lr_min = 0.0                                    # (the constructor's fall-back never passes a zero)
    wholes = {name: _guard(s) for name, s in scheds.items()}
    kw = K.constants(LR, NUM_EPOCHS, ticks, 1, LR_MIN, GAMMA, STEP_SIZE)
    worst = 0.0
    for s in steps + [-1, -(1 << 40)]:
        opt.step_t.fill_(s)
        epoch, i_batch, _ = K.position(s, N, B, world)
        want_index = K.batch_index(SEED, s, N, B, world, rank)
        for name, sched in scheds.items():
            opt.iht_t.fill_(7)
            sched.where.fill_(-1)
            assert sched.advance() is sched.index
            whole = wholes[name].cpu().numpy()
            assert np.array_equal(whole[PAD:PAD + B], want_index), (name, s)
            assert (whole[:PAD] == CANARY).all() and (whole[PAD + B:] == CANARY).all(), (name, s)
            assert sched.where.tolist() == [epoch, i_batch, min(max(s, 0), sched.log_len - 1), 0], (name, s)
            assert int(opt.iht_t) == K.phase(epoch, NUM_EPOCHS, i_batch, TRIM), (name, s)
            want = K.lr_at(name, max(s, 0) + sched.lr_lead, **kw)
            got = float(opt.lr_t)
            worst = max(worst, abs(got - want) / K.lr_bound(LR)(want))
            assert _close(got, want, LR), (name, s, got, want)
        zero_min.advance()
        want = K.lr_at("CosineAnnealingLR", max(s, 0) + 1, **dict(kw, lr_min=0.0))
        assert _close(opt.lr_t, want, LR), ("lr_min = 0", s, float(opt.lr_t), want)
        assert int(opt.iht_t) == 0 and np.array_equal(zero_min.index.cpu().numpy(), want_index)      # no sparsify: phase 0
    print("(N, B, world, rank) = %s: largest lr error %.3f of its bound" % ((N, B, world, rank), worst))


def test_both_optimizers_and_a_short_log():
    opt = _opt(FusedSGD, lr=0.5)
    sched = TrainSchedule(opt, 50, 8, NUM_EPOCHS, seed=7, lr_scheduler="ExponentialResettingLR", gamma=0.5, log_len=4)
    for s, slot in ((0, 0), (3, 3), (4, 3), (17, 3)):
        opt.step_t.fill_(s)
        sched.advance()
        sched.record(torch.tensor(float(s), device=DEV))
        assert int(sched.where[2]) == slot
        assert _close(opt.lr_t, K.lr_at("ExponentialResettingLR", s + 1, 0.5, gamma=0.5, reset=sched.reset), 0.5)
    assert sched.reset == 6 and sched.loss_log.tolist() == [0.0, 0.0, 0.0, 17.0]
    assert sched.lr_log[3] == opt.lr_t[0] and sched.lr_log[0] == 0.25


# ---- 2. one captured call follows the step scalar --------------------------------------------------------------------------
def test_a_captured_advance_follows_the_step_scalar():
    opt = _opt()
    sched = TrainSchedule(opt, 50, 8, NUM_EPOCHS, seed=SEED, lr_scheduler="TriangleLR", lr_min=LR_MIN, gamma=GAMMA,
                          sparsify=True, trim_level=TRIM)
    outs = lambda: tuple(t.clone() for t in (sched.index, opt.lr_t, opt.iht_t, sched.where))
    eager = []
    for s in range(13):
        opt.step_t.fill_(s)
        sched.advance()
        eager.append(outs())

    def fn():
        sched.advance()
        opt.step_t.add_(1)                                        # the step advances on the device, inside the graph

    graphed = GraphedStep(fn)
    opt.step_t.zero_()
    for s, want in enumerate(eager):
        graphed()
        torch.cuda.synchronize()
        assert int(opt.step_t) == s + 1
        for got, w, what in zip(outs(), want, ("index", "lr", "iht", "where")):
            assert S.bits_equal(got, w), (s, what)
    assert len({tuple(e[0].tolist()) for e in eager}) == 13 and {int(e[2]) for e in eager} == {0, 1, 2}


# ---- 3. a whole run from one graph ------------------------------------------------------------------------------------------
N_CLIPS, L_MAX, BATCH = 50, 4000, 8


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
    assert opt.register_iht(model) == 2
    sched = TrainSchedule(opt, N_CLIPS, BATCH, NUM_EPOCHS, seed=SEED, lr_scheduler="StepLR", gamma=0.5, lr_step_size=6,
                          sparsify=True, trim_level=TRIM)
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
    assert int(oa.step_t) == int(ob.step_t) == sa.total_iterations


def test_fit_audio_from_one_graph_equals_the_eager_loop_and_a_host_driven_twin():
    bank, lengths, labels, aug, fe = _bank()
    torch.manual_seed(5)
    start = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [0.5], [0.5], "sigmoid", "tanh",
                               num_classes=12, device=DEV)
    val = [(fe(bank[:10], lengths[:10]).transpose(0, 1).contiguous(), labels[:10])]
    graphed, eager, twin = _trainer(start), _trainer(start), _trainer(start)
    log = graphed[0].fit_audio(bank, lengths, labels, fe, aug, graphed[1], graphed[2], graph=True, validation=lambda: val)
    e_log = eager[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], eager[2], graph=False)
    sched = graphed[2]
    assert (sched.ticks, sched.total_iterations) == (6, 18)
    _same_run(graphed, eager, "graph against eager")
    S.assert_same_bits(sched.loss_log, eager[2].loss_log, "loss_log, graph against eager")
    S.assert_same_bits(sched.lr_log, eager[2].lr_log, "lr_log, graph against eager")
    # the twin: index and phase from the oracle, the learning rate from the log, the step itself called by hand
    model, opt, t_sched = twin
    losses = []
    for s in range(18):
        epoch, i_batch, _ = K.position(s, N_CLIPS, BATCH)
        index = torch.from_numpy(K.batch_index(SEED, s, N_CLIPS, BATCH)).to(DEV)
        opt.lr_t.copy_(sched.lr_log[s:s + 1])
        model.init_hidden()
        losses.append(model.train_step_audio(bank, lengths, labels, index, fe, aug, opt,
                                             iht=iht_phase(epoch, NUM_EPOCHS, i_batch, TRIM)))
    _same_run(graphed, twin, "graph against the host-driven twin")
    S.assert_same_bits(sched.loss_log, torch.stack(losses).reshape(-1), "loss_log against the twin's losses")
    loss_log, lr_log = sched.loss_log.tolist(), sched.lr_log.tolist()
    assert all(np.isfinite(loss_log)) and len(set(loss_log)) == 18
    for s in range(18):
        want = K.lr_at("StepLR", s + 1, LR, gamma=0.5, step_size=6)
        assert _close(lr_log[s], want, LR), (s, lr_log[s], want)
    # the phases ran: the middle third thresholded to the layer's sparsity, the last third kept the support
    for p in (graphed[0].rnn_list[0].W, graphed[0].rnn_list[0].U):
        kept = int((p != 0).sum())
        assert kept <= int(graphed[1].support(p).sum()) < p.numel() and 0.45 * p.numel() < kept < 0.55 * p.numel()
    # the returned log
    assert [e["epoch"] for e in log] == [0, 1, 2] and [e["loss"] for e in log] == [loss_log[i] for i in (5, 11, 17)]
    assert [e["learning_rate"] for e in log] == [lr_log[i] for i in (5, 11, 17)]
    assert all(isinstance(e["accuracy"], float) and 0.0 <= e["accuracy"] <= 1.0 for e in log)
    assert [e["loss"] for e in e_log] == [e["loss"] for e in log] and all(e["accuracy"] is None for e in e_log)
    with pytest.raises(ValueError, match="another optimizer"):
        graphed[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], sched)
    with pytest.raises(TypeError):
        graphed[0].fit_audio(bank, lengths, labels, fe, aug, torch.optim.Adam(graphed[0].parameters()), sched)


# ---- 4. sharding ------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_device_get_disjoint_batches():
    opt = _opt()
    ranks = [TrainSchedule(opt, 64, 8, NUM_EPOCHS, seed=SEED, world=2, rank=r) for r in (0, 1)]
    assert ranks[0].ticks == 4
    for epoch in (0, 1):
        seen = set()
        for i in range(4):
            opt.step_t.fill_(epoch * 4 + i)
            a, b = (set(r.advance().tolist()) for r in ranks)
            assert len(a) == len(b) == 8 and not (a & b) and not (seen & (a | b)), (epoch, i)
            seen |= a | b
        assert seen == set(range(64))
