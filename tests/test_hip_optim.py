"""The six further fused optimizers on the GPU: fastgrnn_hip_optim_update (RMSprop, Adagrad, Adadelta, Adamax, ASGD, Rprop;
then the exact hard threshold or the support mask) and what is built on it (kws_amd.FusedRMSprop ... FusedRprop,
RNNClassifierModel.train_step, one captured graph for a run, fit_audio).

Operands, fp64 oracles and the derived bounds come from tests/optim_cases.py; tests/test_optim_cpu.py holds torch's own
fp32 step to the same bounds on the same operands, and every test here that holds the kernel to a bound asserts torch
against it first.  Everything the threshold does, Rprop's sign decisions and every eager-against-graph comparison are
exact.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mfcc_cases as M
from tests import optim_cases as OC
from tests import support as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import (AudioAugment, GraphedStep, MFCCFrontend, RNNClassifierModel, TrainSchedule, _lib, optim, utils)
DEV = torch.device("cuda:0")
GUARD = 256                        # sentinel floats on each side of every buffer
SENTINEL = -7.25e11


class Buf:
    """A device buffer of n elements with GUARD sentinel floats (4 * GUARD bytes for masks) on each side."""

    def __init__(self, values, dtype=torch.float32):
        values = torch.as_tensor(np.array(values)).to(dtype).reshape(-1)
        self.pad = GUARD if dtype == torch.float32 else 4 * GUARD
        self.fill = SENTINEL if dtype == torch.float32 else 0xA5
        self.whole = torch.full((values.numel() + 2 * self.pad,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[self.pad:self.pad + values.numel()]
        self.t.copy_(values)

    def guards_intact(self):
        return bool((self.whole[:self.pad] == self.fill).all()) and bool((self.whole[-self.pad:] == self.fill).all())

    def numpy(self):
        return self.t.cpu().numpy()


class Seg:
    """One segment's device state: p, g, the rule's state tensors in their slots and (IHT segments) the support mask."""

    def __init__(self, rule, ops, keep_rank=None):
        self.p, self.g = Buf(ops["p"]), Buf(ops["g"])
        self.keys = OC.RULES[rule][2]
        self.state = [Buf(ops[k]) if k else None for k in self.keys]
        self.keep_rank = keep_rank
        self.sup = Buf(np.full(len(ops["p"]), 9), torch.uint8) if keep_rank is not None else None

    def clone(self):
        return copy.deepcopy(self)

    def bufs(self):
        return [b for b in [self.p, self.g, self.sup] + self.state if b is not None]

    def states(self):
        return [b for b in self.state if b is not None]

    def c_seg(self):
        return _lib.OptimSeg(self.p.t.data_ptr(), self.g.t.data_ptr(),
                             tuple(b.t.data_ptr() if b else None for b in self.state),
                             self.sup.t.data_ptr() if self.sup else None, self.p.t.numel(), self.keep_rank or 0,
                             1 if self.sup else 0, 0)

    def got(self):
        out = {"p": self.p.numpy()}
        out.update({k: b.numpy() for k, b in zip(self.keys, self.state) if k})
        return out


UNWRITTEN = 123.0


def scalars_for(rule, t, ops):
    """ASGD's double buffer before step t: what step t-1 left in its pair, a marker in the pair step t writes"""
    if OC.kind(rule) != "ASGD":
        return None
    vals = [UNWRITTEN] * 4
    vals[2 * ((t - 1) & 1):2 * ((t - 1) & 1) + 2] = [ops["eta"], ops["mu"]]
    return Buf(np.array(vals, np.float32))


def run(rule, wd, segs, t, mode, scalars=None, lr=None):
    """One library call on the current stream; the device scalars are made here."""
    lib = _lib.load()
    lr_t = torch.tensor([OC.RULES[rule][1]["lr"] if lr is None else lr], dtype=torch.float32, device=DEV)
    step_t = torch.tensor([t], dtype=torch.int64, device=DEV)
    mode_t = torch.tensor([mode], dtype=torch.int32, device=DEV)
    arr = (_lib.OptimSeg * len(segs))(*[s.c_seg() for s in segs])
    hy = OC.c_hyper(rule, wd)
    st = lib.fastgrnn_hip_optim_update(C.byref(hy), arr, len(segs), lr_t.data_ptr(), step_t.data_ptr(),
                                       mode_t.data_ptr(), scalars.t.data_ptr() if scalars else None,
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "optim_update")
    torch.cuda.synchronize()
    for s in segs:
        assert all(b.guards_intact() for b in s.bufs()), "a sentinel next to a buffer of %d elements changed" % s.p.t.numel()
    assert scalars is None or scalars.guards_intact()


def same_bits(a, b):
    return all(torch.equal(x.t, y.t) for x, y in zip(a.bufs(), b.bufs()))


# ---- 1. update parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,t,wd", OC.CASES)
def test_update_matches_the_fp64_oracle(rule, t, wd):
    ops = [OC.segment(rule, n, t, 1) for n in OC.SIZES]
    segs = [Seg(rule, o) for o in ops]
    twin = [s.clone() for s in segs]
    sc = scalars_for(rule, t, ops[0])
    sc_twin = copy.deepcopy(sc)
    run(rule, wd, segs, t, 0, sc)
    for n, o, s in zip(OC.SIZES, ops, segs):
        ref = OC.oracle(rule, wd, t, o)
        w_torch = OC.worst(OC.torch_cpu_step(rule, wd, t, o), ref)
        assert max(w_torch.values()) <= 1.0, ("the bound is wrong: torch's fp32 step misses it", n, w_torch)
        got = s.got()
        if sc is not None:
            read, written = sc.numpy()[2 * ((t - 1) & 1):][:2], sc.numpy()[2 * (t & 1):][:2]
            assert read.tolist() == [np.float32(o["eta"]), np.float32(o["mu"])]            # the pair it read: untouched
            got.update(eta=np.float64(written[0]), mu=np.float64(written[1]))
        w = OC.worst(got, ref)
        print("%s t=%d wd=%g n=%d: error / bound %s (torch fp32: %s)" % (rule, t, wd, n, w, w_torch))
        assert max(w.values()) <= 1.0, (n, w)
        assert n == 1 or not np.array_equal(got["p"], o["p"])             # (something happened)
        if rule == "rprop":
            assert np.array_equal(s.g.numpy(), o["g"])
            if t == 1:                                                     # from torch's fresh state: prev = 0, so sign 0
                assert np.array_equal(got["step_size"], o["step_size"]) and np.array_equal(got["prev"], o["g"])
            elif n >= 1023:                                                # both clamps, and both of them exactly
                assert (got["step_size"] == np.float32(1e-6)).any() and (got["step_size"] == np.float32(50.0)).any()
                assert (got["prev"][o["g"] * o["prev"] < 0] == 0).all()
    run(rule, wd, twin, t, 0, sc_twin)                                     # the same call from the same state: same bits
    assert all(same_bits(a, b) for a, b in zip(segs, twin))
    assert sc is None or torch.equal(sc.t, sc_twin.t)


def test_asgd_first_step_reads_lr_and_one_not_the_buffer():
    rule, t, n = "asgd_avg", 1, 3079
    o = OC.segment(rule, n, t, 1)
    assert (o["eta"], o["mu"]) == (OC.f32(0.01), 1.0)
    s, sc = Seg(rule, o), Buf(np.full(4, UNWRITTEN, np.float32))
    run(rule, 1e-5, [s], t, 0, sc)
    w = OC.worst(s.got(), {k: v for k, v in OC.oracle(rule, 1e-5, t, o).items() if k in ("p", "ax")})
    assert max(w.values()) <= 1.0, w
    assert sc.numpy()[:2].tolist() == [UNWRITTEN, UNWRITTEN] and np.array_equal(s.state[0].numpy(), s.p.numpy())


# ---- 2. a mixed call across the launch split ---------------------------------------------------------------------------
MIXED = ("rmsprop_centered_mom", "adagrad_decay", "adadelta", "adamax", "asgd_avg", "rprop")


@pytest.mark.parametrize("rule", MIXED)
def test_33_mixed_segments_equal_each_run_alone(rule):
    sizes, t = list(range(5, 38)), 1000
    wd = OC.wds_of(rule)[-1]
    assert len(sizes) == 33 > _lib.UPDATE_MAX_SEGS

    def build():
        out = []
        for i, n in enumerate(sizes):
            rank = None if i % 3 == 0 else 0 if i == 7 else optim.keep_rank(n, 0.4)
            out.append(Seg(rule, OC.segment(rule, n, t, 2), rank))
        return out

    together, alone = build(), build()
    assert sum(x.sup is not None for x in together) == 22 and together[7].keep_rank == 0 and together[32].sup is not None
    o0 = OC.segment(rule, sizes[0], t, 2)
    sc = scalars_for(rule, t, o0)
    run(rule, wd, together, t, 1, sc)
    for x in alone:
        sc1 = scalars_for(rule, t, o0)
        run(rule, wd, [x], t, 1, sc1)
        assert sc is None or torch.equal(sc.t, sc1.t)                      # both launches wrote the same eta and mu
    for i, (a, b) in enumerate(zip(together, alone)):
        assert same_bits(a, b), sizes[i]
        start = OC.segment(rule, sizes[i], t, 2)["p"]
        assert not np.array_equal(a.p.numpy(), start)                      # every segment was updated, the 33rd included
        if a.sup is not None:
            assert torch.equal(a.sup.t, (a.p.t != 0).to(torch.uint8))
            zeros = int((a.p.t == 0).sum())
            assert zeros == (0 if i == 7 else a.keep_rank), (i, zeros)    # distinct magnitudes: exactly keep_rank go


# ---- 3. the IHT phases, every rule --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sorted(OC.RULES))
def test_threshold_is_hard_threshold_of_the_plain_step_and_support_mode_keeps_zeros(rule):
    n, t, s = 3079, 2, 0.3
    wd = OC.wds_of(rule)[-1]
    o = OC.segment(rule, n, t, 1)
    plain = Seg(rule, o, optim.keep_rank(n, s))
    thr = plain.clone()
    scs = [scalars_for(rule, t, o) for _ in range(2)]
    run(rule, wd, [plain], t, 0, scs[0])
    run(rule, wd, [thr], t, 1, scs[1])
    want = utils.hardThreshold(plain.p.t.clone(), s)
    assert torch.equal(thr.p.t, want), int((thr.p.t != want).sum())
    assert torch.equal(thr.sup.t, (thr.p.t != 0).to(torch.uint8))
    assert int(thr.sup.t.sum()) == n - optim.keep_rank(n, s) < n
    assert all(torch.equal(a.t, b.t) for a, b in zip(plain.states(), thr.states()))          # state: never masked
    assert torch.equal(plain.sup.t, torch.full_like(plain.sup.t, 9))      # mode 0 does not write the mask
    assert scs[0] is None or torch.equal(scs[0].t, scs[1].t)
    # the next step in support mode, on a fresh gradient
    t2 = t + 1
    support = thr.sup.t.clone()
    keep = support.bool()
    o2 = OC.segment(rule, n, t2, 11)
    thr.g.t.copy_(torch.from_numpy(np.array(o2["g"])))
    free = thr.clone()
    sc2 = [copy.deepcopy(scs[1]) for _ in range(2)]
    run(rule, wd, [free], t2, 0, sc2[0])
    run(rule, wd, [thr], t2, 2, sc2[1])
    assert torch.equal(thr.sup.t, support)                                 # the mask is only read
    assert bool((thr.p.t[~keep] == 0).all())                               # zeros stay zero
    assert torch.equal(thr.p.t[keep], free.p.t[keep])                      # survivors take the plain update
    assert bool((free.p.t[~keep] != 0).any())                              # (which would have moved the zeros)
    assert all(torch.equal(a.t, b.t) for a, b in zip(free.states(), thr.states()))           # state: not masked
    run(rule, wd, [free], t2 + 1, 3, sc2[0])                               # an unknown mode value behaves as none
    assert bool((free.sup.t == support).all())


# ---- 4. module level -------------------------------------------------------------------------------------------------
T, B, F, NCLS = 9, 37, 32, 12
MODULE_RULES = MIXED


def fused_class(rule):
    return getattr(optim, "Fused" + OC.kind(rule))


def default_model(seed=0):
    torch.manual_seed(seed)
    return RNNClassifierModel("FastGRNNCUDA", F, 2, [256, 128], [None, None], [None, None], [0.3, 0.5], [0.2, 0.5],
                              "sigmoid", "tanh", num_classes=NCLS, device=DEV)


def batch(seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randn(T, B, F, generator=g).to(DEV), torch.randint(0, NCLS, (B,), generator=g).to(DEV)


def asgd_pair(opt):
    """(eta, mu) the next step of a FusedASGD reads"""
    t = int(opt.step_t)
    return (float(opt.lr_t), 1.0) if t == 0 else tuple(opt.scalars[2 * (t & 1):][:2].tolist())


def iht_matrices(model):
    return {id(p): s for rnn in model.rnn_list for p, s in ((rnn.W, rnn._wSparsity), (rnn.U, rnn._uSparsity))}


@pytest.mark.parametrize("rule", MODULE_RULES)
def test_train_step_against_torch_optim_and_sparsify(rule):
    """Three iterations -- plain, thresholded, support-masked -- by train_step and by the chain it replaces
    (torch.optim.X(foreach=False).step(), then sparsify() / sparsifyWithSupport()).  Before every iteration the twin
    takes the fused run's parameters and state, so each step is held to the one-step bound: torch first, then the kernel.
    Where the threshold cuts, an entry whose fp64 magnitude lies within two bounds of the fp64 threshold may fall either
    way; every other entry must be zero, or within its bound, in both."""
    k, wd = OC.kind(rule), OC.wds_of(rule)[-1]
    h = OC.hyper(rule, wd)
    model = default_model()
    twin = copy.deepcopy(model)
    opt = fused_class(rule)(model.parameters(), **h)
    assert opt.register_iht(model) == 4
    ref_opt = getattr(torch.optim, k)(twin.parameters(), foreach=False, **h)
    sparsities = iht_matrices(model)
    twin_old = {id(q): (rnn, i) for rnn in twin.rnn_list for i, q in enumerate((rnn.W, rnn.U))}     # oldmats = [W, U]
    assert len(sparsities) == 4 == len(twin_old)
    worst = {"fused": 0.0, "torch": 0.0}
    for step, phase in enumerate(("none", "threshold", "support"), 1):
        x, y = batch(step)
        start = [p.detach().clone() for p in model.parameters()]
        state0 = [{key: opt.state[p][key].clone() for key in OC.keys(rule)} if opt.state.get(p) else None
                  for p in model.parameters()]
        pair = asgd_pair(opt) if k == "ASGD" else None
        support0 = {id(p): opt.support(p).clone() for p in model.parameters() if id(p) in sparsities}
        with torch.no_grad():                                              # the twin starts where the fused run stands
            for p, q in zip(model.parameters(), twin.parameters()):
                q.copy_(p)
                if ref_opt.state.get(q):
                    for key in OC.keys(rule):
                        ref_opt.state[q][key].copy_(opt.state[p][key])
                    if k == "ASGD":
                        ref_opt.state[q]["eta"].fill_(pair[0])
                        ref_opt.state[q]["mu"].fill_(pair[1])
        model.init_hidden()
        twin.init_hidden()
        loss = model.train_step(x, y, opt, iht=phase)
        for q in twin.parameters():
            q.grad = None
        ref_loss = twin.loss(x, y)
        ref_loss.backward()
        ref_opt.step()
        if phase == "threshold":
            twin.sparsify()
        elif phase == "support":
            twin.sparsifyWithSupport()
        assert not loss.requires_grad and torch.equal(loss, ref_loss.detach())
        assert int(opt.step_t) == step
        for i, ((name, p), q) in enumerate(zip(model.named_parameters(), twin.parameters())):
            assert torch.equal(p.grad, q.grad), name                       # same parameters, same gradients
            n = p.numel()
            ops = {"p": start[i].cpu().numpy().reshape(-1), "g": p.grad.cpu().numpy().reshape(-1)}
            for key in OC.keys(rule):
                ops[key] = state0[i][key].cpu().numpy().reshape(-1) if state0[i] else OC.segment(rule, n, 1, 0)[key]
            if k == "ASGD":
                ops["eta"], ops["mu"] = pair
            ref = OC.oracle(rule, wd, step, ops)
            p64, bound = ref["p"]
            for who, tensor, o, mask0 in (("torch", q, ref_opt, None), ("fused", p, opt, support0.get(id(p)))):
                got = tensor.detach().cpu().numpy().reshape(-1)
                ratio = np.abs(got - p64) / np.maximum(bound, 1e-300)
                if id(p) in sparsities and phase == "threshold":
                    th = np.sort(np.abs(p64))[optim.keep_rank(n, sparsities[id(p)])]
                    margin = 2 * bound.max()
                    gone, stays = np.abs(p64) < th - margin, np.abs(p64) > th + margin
                    assert gone.any() and stays.any() and (gone | stays).mean() > 0.99, (who, name)
                    assert (got[gone] == 0).all() and (got[stays] != 0).all(), (who, name)
                    checked = stays
                elif id(p) in sparsities and phase == "support":
                    mask0 = mask0 if who == "fused" else twin_old[id(q)][0].oldmats[twin_old[id(q)][1]]
                    mask = mask0.cpu().numpy().reshape(-1) != 0
                    assert (got[~mask] == 0).all() and 0 < mask.sum() < n, (who, name)
                    checked = mask
                else:
                    checked = np.ones(n, bool)
                assert (ratio[checked] <= 1.0).all(), (who, name, phase, float(ratio[checked].max()))
                worst[who] = max(worst[who], float(ratio[checked].max()))
                st = o.state[tensor]
                for key in OC.keys(rule):                                  # the state: never masked, always within its bound
                    val, b = ref[key]
                    err = np.abs(st[key].cpu().numpy().reshape(-1) - val)
                    assert (err <= b).all(), (who, name, key, phase)
            if id(p) in sparsities and phase == "threshold":
                assert torch.equal(opt.support(p), (p != 0).to(torch.uint8))
                assert abs(float((p != 0).float().mean()) - sparsities[id(p)]) < 0.01
            assert not torch.equal(p.detach(), start[i]), name
        if k == "ASGD":
            got = asgd_pair(opt)
            for g_, name in zip(got, ("eta", "mu")):
                assert abs(g_ - ref[name][0]) <= ref[name][1], (name, g_, ref[name])
    print("%s module steps: error / bound %.3f (torch.optim fp32 on the GPU: %.3f)" % (rule, worst["fused"], worst["torch"]))
    for rnn in model.rnn_list:
        assert rnn.oldmats == []                                           # the layers' own IHT state is not touched


# ---- 5. one graph for the run -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ("rmsprop_centered_mom", "adagrad_decay", "asgd_avg", "rprop"))
def test_one_captured_graph_serves_changing_lr_and_iht_phase(rule):
    """Adagrad's decayed rate follows step_t; ASGD's eta and mu are carried from replay to replay through both pairs of
    the double buffer (four steps: both parities read and written, mu below one at the fourth); Rprop's step sizes
    start at the constructor's lr, which is the plan's first, on both sides."""
    plan = [("none", 0.01), ("threshold", 0.004), ("support", 0.02), ("support", 0.007)]
    k, h = OC.kind(rule), OC.hyper(rule, 1e-5)
    model = default_model(5)
    eager = copy.deepcopy(model)
    x, y = batch(5)

    e_opt = fused_class(rule)(eager.parameters(), **h)
    e_opt.register_iht(eager)
    for iht, lr in plan:
        e_opt.param_groups[0]["lr"] = lr
        eager.init_hidden()
        eager.train_step(x, y, e_opt, iht=iht)

    # one capture; its warm-up steps are undone before the first replay
    opt = fused_class(rule)(model.parameters(), capturable=True, **h)
    opt.register_iht(model)

    def fn():
        model.init_hidden()
        return model.train_step(x, y, opt, iht=None)

    step = GraphedStep(fn, undo=(model, opt))
    if k == "ASGD":
        opt.scalars.fill_(777.0)                                           # (step 1 reads neither pair)
    for iht, lr in plan:
        opt.lr_t.fill_(lr)
        opt.iht_t.fill_(optim.IHT_MODES[iht])
        step()
    torch.cuda.synchronize()
    assert int(opt.step_t) == 4 == int(e_opt.step_t)
    for (name, p), q in zip(model.named_parameters(), eager.parameters()):
        assert torch.equal(p, q), name
        for key in OC.keys(rule):
            assert torch.equal(opt.state[p][key], e_opt.state[q][key]), (name, key)
    for a, b in zip(model.rnn_list, eager.rnn_list):
        for pa, pb in ((a.W, b.W), (a.U, b.U)):
            assert torch.equal(opt.support(pa), e_opt.support(pb))
            assert 0 < int(opt.support(pa).sum()) < pa.numel() and bool((pa[opt.support(pa) == 0] == 0).all())
    if k == "ASGD":
        assert torch.equal(opt.scalars, e_opt.scalars) and 777.0 not in opt.scalars.tolist()
        eta3, mu3, eta4, mu4 = opt.scalars[2:].tolist() + opt.scalars[:2].tolist()          # pairs 3 & 1 and 4 & 1
        lam, al = h["lambd"], h["alpha"]
        for got, lr, t in ((eta3, 0.02, 3), (eta4, 0.007, 4)):             # each from the lr of ITS replay
            want = OC.f32(lr) / (1 + lam * OC.f32(lr) * t) ** al
            assert abs(got - want) <= 2 * OC.u * want, (t, got, want)
        assert (mu3, mu4) == (0.5, OC.f32(1 / 3))
        sd = opt.state_dict()
        assert float(sd["state"][0]["eta"]) == eta4 and float(sd["state"][0]["mu"]) == mu4 and float(sd["state"][0]["step"]) == 4.0


# ---- 6. a short run from one graph --------------------------------------------------------------------------------------
N_CLIPS, L_MAX, BATCH, NUM_EPOCHS, TRIM, SEED = 16, 4000, 8, 3, 2, (0xC0FFEE << 32) | 0x1234


@functools.lru_cache(maxsize=None)
def audio_run():
    """the bank, the augmenter, the front end and the start model of the fit_audio tests: built once, only read"""
    rng = np.random.default_rng(11)
    lengths = rng.integers(1280, L_MAX + 1, N_CLIPS).astype(np.int32)
    lengths[:2] = (1280, L_MAX)
    bank = np.zeros((N_CLIPS, L_MAX), dtype=np.float32)
    for c, n in enumerate(lengths):
        bank[c, :n] = M.speech_like(100 + c, int(n)) if c % 2 else M.noise(200 + c, int(n), 0.2)
    labels = torch.from_numpy(rng.integers(0, 12, N_CLIPS)).to(DEV)
    bank, lengths = torch.from_numpy(bank).to(DEV), torch.from_numpy(lengths).to(DEV)
    noises = [torch.from_numpy(M.noise(300, 700, 0.3)), torch.from_numpy(M.noise(301, 5000, 0.1))]
    aug = AudioAugment(p_augment=0.75, max_shift=400, gain=(0.5, 1.5), p_noise=0.5, noise_gain=(0.05, 0.3), seed=SEED,
                       noises=noises, device=DEV)
    fe = MFCCFrontend(n_mfcc=16, feature_type="delta", max_len=1 + L_MAX // 160, device=DEV)
    torch.manual_seed(5)
    start = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [0.5], [0.5], "sigmoid", "tanh",
                               num_classes=12, device=DEV)
    return bank, lengths, labels, fe, aug, start


def test_fit_audio_with_rmsprop_from_one_graph_equals_the_eager_loop():
    bank, lengths, labels, fe, aug, start = audio_run()

    def trainer():
        model = copy.deepcopy(start)
        opt = optim.FusedRMSprop(model.parameters(), lr=0.01, momentum=0.9, centered=True, weight_decay=1e-5, capturable=True)
        assert opt.register_iht(model) == 2
        sched = TrainSchedule(opt, N_CLIPS, BATCH, NUM_EPOCHS, seed=SEED, lr_scheduler="StepLR", gamma=0.5, lr_step_size=2,
                              sparsify=True, trim_level=TRIM)
        return model, opt, sched

    (gm, go, gs), (em, eo, es) = trainer(), trainer()
    log = gm.fit_audio(bank, lengths, labels, fe, aug, go, gs, graph=True)
    e_log = em.fit_audio(bank, lengths, labels, fe, aug, eo, es, graph=False)
    assert (gs.ticks, gs.total_iterations) == (2, 6) and int(go.step_t) == int(eo.step_t) == 6
    for (name, p), q in zip(gm.named_parameters(), em.parameters()):
        S.assert_same_bits(p.detach(), q.detach(), name)
        assert set(go.state[p]) >= {"square_avg", "momentum_buffer", "grad_avg"}
        for key in ("square_avg", "momentum_buffer", "grad_avg"):
            S.assert_same_bits(go.state[p][key], eo.state[q][key], "%s of %s" % (key, name))
    S.assert_same_bits(gs.loss_log, es.loss_log, "loss_log")
    S.assert_same_bits(gs.lr_log, es.lr_log, "lr_log")
    assert all(np.isfinite(gs.loss_log.tolist())) and len(set(gs.loss_log.tolist())) == 6 and len(set(gs.lr_log.tolist())) >= 2
    assert [e["loss"] for e in log] == [e["loss"] for e in e_log]
    for pa, pb in ((gm.rnn_list[0].W, em.rnn_list[0].W), (gm.rnn_list[0].U, em.rnn_list[0].U)):
        S.assert_same_bits(go.support(pa), eo.support(pb), "a support mask")
        kept = int((pa != 0).sum())                                        # the middle third thresholded, the last kept it
        assert kept <= int(go.support(pa).sum()) < pa.numel() and 0.45 * pa.numel() < kept < 0.55 * pa.numel()


def fit_trainer(cls, **h):
    model = copy.deepcopy(audio_run()[5])
    opt = cls(model.parameters(), capturable=True, **h)
    assert opt.register_iht(model) == 2
    sched = TrainSchedule(opt, N_CLIPS, BATCH, NUM_EPOCHS, seed=SEED, lr_scheduler="StepLR", gamma=0.5, lr_step_size=2,
                          sparsify=True, trim_level=TRIM)
    assert (sched.ticks, sched.total_iterations) == (2, 6)
    return model, opt, sched


def assert_same_run(graphed, eager, keys):
    (gm, go, gs), (em, eo, es) = graphed, eager
    assert int(go.step_t) == int(eo.step_t) == 6
    for (name, p), q in zip(gm.named_parameters(), em.parameters()):
        S.assert_same_bits(p.detach(), q.detach(), name)
        for key in keys:
            S.assert_same_bits(go.state[p][key], eo.state[q][key], "%s of %s" % (key, name))
    S.assert_same_bits(gs.loss_log, es.loss_log, "loss_log")
    S.assert_same_bits(gs.lr_log, es.lr_log, "lr_log")
    assert all(np.isfinite(gs.loss_log.tolist())) and len(set(gs.loss_log.tolist())) == 6
    for pa, pb in ((gm.rnn_list[0].W, em.rnn_list[0].W), (gm.rnn_list[0].U, em.rnn_list[0].U)):
        S.assert_same_bits(go.support(pa), eo.support(pb), "a support mask")


def test_fit_audio_with_rprop_from_one_graph_equals_the_eager_loop():
    """The warm-up creates Rprop's state; undone, step_size is the lr again (not zero) when the first replay reads it."""
    bank, lengths, labels, fe, aug, _ = audio_run()
    h = OC.hyper("rprop", 0.0)
    graphed, eager = fit_trainer(optim.FusedRprop, **h), fit_trainer(optim.FusedRprop, **h)
    graphed[0].fit_audio(bank, lengths, labels, fe, aug, graphed[1], graphed[2], graph=True)
    eager[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], eager[2], graph=False)
    assert_same_run(graphed, eager, ("prev", "step_size"))
    sizes = torch.cat([graphed[1].state[p]["step_size"].reshape(-1) for p in graphed[0].parameters()])
    assert float(sizes.min()) < h["lr"] < float(sizes.max())                # (they adapted both ways from the lr)


def test_fit_audio_with_asgd_resumed_at_step_three_from_one_graph_equals_the_eager_loop():
    """A run that begins at step_t = 3: step 4 reads the pair of eta and mu that step 3 left, which the capture's
    warm-up (steps 4, 5 and 6) overwrites at step 5 -- the undo has to put the double buffer back."""
    bank, lengths, labels, fe, aug, _ = audio_run()
    h = OC.hyper("asgd_avg", 1e-5)
    graphed, eager = fit_trainer(optim.FusedASGD, **h), fit_trainer(optim.FusedASGD, **h)
    eager[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], eager[2], graph=False)
    model, opt, sched = graphed
    model.train()
    for _ in range(3):
        model.init_hidden()
        sched.advance()
        sched.record(model.train_step_audio(bank, lengths, labels, sched.index, fe, aug, opt, iht=None))
    assert int(opt.step_t) == 3
    model.fit_audio(bank, lengths, labels, fe, aug, opt, sched, graph=True)
    assert_same_run(graphed, eager, ("ax",))
    S.assert_same_bits(opt.scalars, eager[1].scalars, "scalars")
    eta, mu = opt.scalars[:2].tolist()                                      # the pair of step 6
    assert 0.0 < eta < OC.f32(h["lr"]) and mu == OC.f32(1 / 5)              # (both moved: t0 = 1)


# ---- 7. versions --------------------------------------------------------------------------------------------------------
def test_a_fused_step_moves_the_parameters_versions():
    model = default_model(7)
    opt = optim.FusedAdadelta(model.parameters(), rho=0.0, eps=1e-8)       # (the reference's default options)
    x, y = batch(7)
    before = [p._version for p in model.parameters()]
    model.train_step(x, y, opt)
    assert all(p._version > v for p, v in zip(model.parameters(), before))
