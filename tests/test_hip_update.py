"""The fused optimizer step on the GPU: fastgrnn_hip_train_update (Adam / SGD update, exact hard threshold, support mask)
and what is built on it (kws_amd.FusedAdam / FusedSGD, RNNClassifierModel.train_step, one captured graph for a run).

Operands, fp64 oracles and the derived bound (8u times the magnitudes of an output's terms) come from
tests/update_cases.py; tests/test_update_cpu.py holds torch's own fp32 step to the same bound on the same operands, and
the parity test repeats that before it looks at the kernel.  Everything the threshold does is compared exactly.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import update_cases as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import FastGRNNCUDA, FusedAdam, FusedSGD, GraphedStep, RNNClassifierModel, _lib, optim, utils
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


class Seg:
    """One segment's device state: p, g, s0, s1 and (IHT segments) the support mask."""

    def __init__(self, p, g, s0, s1=None, keep_rank=None):
        self.p, self.g, self.s0 = Buf(p), Buf(g), Buf(s0)
        self.s1 = Buf(s1) if s1 is not None else None
        self.keep_rank = keep_rank
        self.sup = Buf(np.full(len(p), 9), torch.uint8) if keep_rank is not None else None

    def clone(self):
        return copy.deepcopy(self)

    def bufs(self):
        return [b for b in (self.p, self.g, self.s0, self.s1, self.sup) if b is not None]

    def c_seg(self):
        return _lib.UpdateSeg(self.p.t.data_ptr(), self.g.t.data_ptr(), self.s0.t.data_ptr(),
                              self.s1.t.data_ptr() if self.s1 else None, self.sup.t.data_ptr() if self.sup else None,
                              self.p.t.numel(), self.keep_rank or 0, 1 if self.sup else 0, 0)


def c_hyper(algo, wd):
    h = U.hyper(algo, wd)
    if algo == "adam":
        return _lib.UpdateHyper(_lib.ADAM, 0, h["betas"][0], h["betas"][1], h["eps"], wd)
    return _lib.UpdateHyper(_lib.SGD, int(h["nesterov"]), h["momentum"], h["dampening"], 0.0, wd)


def run(segs, hy, lr, t, mode):
    """One library call on the current stream; the device scalars are made here."""
    lib = _lib.load()
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    step_t = torch.tensor([t], dtype=torch.int64, device=DEV)
    mode_t = torch.tensor([mode], dtype=torch.int32, device=DEV)
    arr = (_lib.UpdateSeg * len(segs))(*[s.c_seg() for s in segs])
    st = lib.fastgrnn_hip_train_update(C.byref(hy), arr, len(segs), lr_t.data_ptr(), step_t.data_ptr(), mode_t.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "train_update")
    torch.cuda.synchronize()
    for s in segs:
        assert all(b.guards_intact() for b in s.bufs()), "a sentinel next to a buffer of %d elements changed" % s.p.t.numel()


def make_seg(algo, n, t, keep_rank=None, seed=1):
    p, g, m, v, b = U.segment(n, t, seed)
    return Seg(p, g, m, v, keep_rank) if algo == "adam" else Seg(p, g, b, None, keep_rank)


def same_bits(a, b):
    return all(torch.equal(x.t, y.t) for x, y in zip(a.bufs(), b.bufs()))


# ---- 1. update parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", U.WDS)
@pytest.mark.parametrize("t", U.STEPS)
@pytest.mark.parametrize("algo", U.ALGOS)
def test_update_matches_the_fp64_oracle(algo, t, wd):
    lr = U.hyper(algo, wd)["lr"]
    segs = [make_seg(algo, n, t) for n in U.SIZES]
    twin = [s.clone() for s in segs]
    run(segs, c_hyper(algo, wd), lr, t, 0)
    for n, s in zip(U.SIZES, segs):
        ops = U.segment(n, t, 1)
        ref = U.oracle(algo, wd, t, *ops)
        w_torch = U.worst(U.torch_cpu_step(algo, wd, t, *ops), ref)
        assert max(w_torch.values()) <= 1.0, ("the bound is wrong: torch's fp32 step misses it", n, w_torch)
        got = {"p": s.p.t.cpu().numpy()}
        if algo == "adam":
            got.update(m=s.s0.t.cpu().numpy(), v=s.s1.t.cpu().numpy())
        else:
            got.update(b=s.s0.t.cpu().numpy())
        w = U.worst(got, ref)
        print("%s t=%d wd=%g n=%d: error / bound %s (torch fp32: %s)" % (algo, t, wd, n, w, w_torch))
        assert max(w.values()) <= 1.0, (n, w)
        assert not np.array_equal(got["p"], ops[0])                        # (something happened)
    run(twin, c_hyper(algo, wd), lr, t, 0)                                 # the same call from the same state: same bits
    assert all(same_bits(a, b) for a, b in zip(segs, twin))


def test_sgd_without_momentum_and_with_dampening():
    """torch keeps no buffer without momentum (and ignores dampening then); with momentum, dampening scales the
    gradient from the second step on."""
    n, t = 3079, 2
    p, g, _, _, b = U.segment(n, t, 1)
    s = Seg(p, g, b)
    run([s], _lib.UpdateHyper(_lib.SGD, 0, 0.0, 0.3, 0.0, 0.0), 0.05, t, 0)
    p64, _, bound, _ = U.sgd_oracle(p, g, b, U.lr32(0.05), 0.0, 0.0, 0.0, False, 1)          # p - lr g
    assert (np.abs(s.p.t.cpu().numpy() - p64) <= bound).all()
    assert np.array_equal(s.s0.t.cpu().numpy(), b)                        # the buffer is left alone
    s = Seg(p, g, b)
    run([s], _lib.UpdateHyper(_lib.SGD, 0, 0.9, 0.1, 0.0, 1e-5), 0.05, t, 0)
    p64, b64, bp, bb = U.sgd_oracle(p, g, b, U.lr32(0.05), 0.9, 0.1, 1e-5, False, t)
    ref = torch.nn.Parameter(torch.from_numpy(np.array(p)))
    ref.grad = torch.from_numpy(np.array(g))
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-5, foreach=False)
    opt.state[ref] = {"momentum_buffer": torch.from_numpy(np.array(b))}
    opt.step()
    assert (np.abs(ref.detach().numpy() - p64) <= bp).all()               # torch first
    assert (np.abs(s.p.t.cpu().numpy() - p64) <= bp).all() and (np.abs(s.s0.t.cpu().numpy() - b64) <= bb).all()


# ---- 2. the threshold is exact ----------------------------------------------------------------------------------------
def check_threshold(plain, thr, s_of):
    """thr (mode 1) against plain (mode 0) from the same state: hardThreshold of the updated values, its support, and
    untouched moments."""
    for a, b, s in zip(plain, thr, s_of):
        want = utils.hardThreshold(a.p.t.clone(), s)
        assert torch.equal(b.p.t, want), (a.p.t.numel(), s, int((b.p.t != want).sum()))
        assert torch.equal(b.sup.t, (b.p.t != 0).to(torch.uint8)), (a.p.t.numel(), s)
        assert torch.equal(a.s0.t, b.s0.t) and (a.s1 is None or torch.equal(a.s1.t, b.s1.t))
        assert torch.equal(a.sup.t, torch.full_like(a.sup.t, 9))          # mode 0 does not write the mask


@pytest.mark.parametrize("s", U.SPARSITIES)
@pytest.mark.parametrize("algo", ("adam", "sgd"))
def test_hard_threshold_equals_utils_hard_threshold(algo, s):
    t = 2
    plain = [make_seg(algo, n, t, optim.keep_rank(n, s)) for n in U.SIZES]
    thr = [x.clone() for x in plain]
    hy = c_hyper(algo, 1e-5)
    run(plain, hy, 0.01, t, 0)
    run(thr, hy, 0.01, t, 1)
    check_threshold(plain, thr, [s] * len(plain))
    kept = [int((x.p.t != 0).sum()) for x in thr]
    print("s=%g kept %s of %s" % (s, kept, list(U.SIZES)))
    if s < 1.0:
        assert all(k < n for k, n in zip(kept, U.SIZES) if n > 1)         # something was cut
        assert abs(kept[-1] / U.SIZES[-1] - s) < 0.01
    else:
        assert kept == list(U.SIZES)


@pytest.mark.parametrize("n", (1025, 65536))
@pytest.mark.parametrize("name", U.ADVERSARIAL)
def test_hard_threshold_on_adversarial_magnitudes(name, n):
    """Values whose magnitudes differ in one byte of their bit pattern only (each radix pass decides alone), are all
    equal, take two values, or are half zeros of both signs.  SGD at step 1 with lr = 1 writes exactly these values."""
    target = U.adversarial(name, n)
    p, g = U.adversarial_operands(target)
    hy = _lib.UpdateHyper(_lib.SGD, 0, 0.9, 0.0, 0.0, 0.0)
    plain = [Seg(p, g, np.zeros(n, np.float32), None, optim.keep_rank(n, s)) for s in U.SPARSITIES]
    thr = [x.clone() for x in plain]
    run(plain, hy, 1.0, 1, 0)
    assert np.array_equal(plain[0].p.t.cpu().numpy().view(np.uint32), target.view(np.uint32))   # the construction holds
    run(thr, hy, 1.0, 1, 1)
    check_threshold(plain, thr, U.SPARSITIES)
    for x, s in zip(thr, U.SPARSITIES):
        th, want = U.threshold_oracle(target, s)
        assert np.array_equal(x.p.t.cpu().numpy(), want), (name, s)
    if name == "all_equal":
        assert all(bool((x.p.t != 0).all()) for x in thr)                 # ties with the threshold survive
    if name == "half_zeros":
        assert int((thr[2].p.t != 0).sum()) == n - n // 2                 # s = 0.5: the threshold is the smallest non-zero


# ---- 3. support mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ("adam", "sgd_nesterov"))
def test_support_mode_keeps_zeros_and_updates_survivors(algo):
    sizes, s = (1025, 65536), 0.3
    hy = c_hyper(algo, 1e-5)
    segs = [make_seg(algo, n, 2, optim.keep_rank(n, s)) for n in sizes]
    run(segs, hy, 0.01, 2, 1)
    support = [x.sup.t.clone() for x in segs]
    assert all(0 < int(m.sum()) < m.numel() for m in support)
    for k, t in enumerate((3, 4)):
        for x, n in zip(segs, sizes):
            x.g.t.copy_(torch.from_numpy(np.array(U.segment(n, t, seed=10 + k)[1])))          # fresh gradients
        plain = [x.clone() for x in segs]
        run(plain, hy, 0.01, t, 0)
        run(segs, hy, 0.01, t, 2)
        for x, a, m in zip(segs, plain, support):
            keep = m.bool()
            assert torch.equal(x.sup.t, m)                                # the mask is only read
            assert bool((x.p.t[~keep] == 0).all())                        # zeros stay zero
            assert torch.equal(x.p.t[keep], a.p.t[keep])                  # survivors take the plain update
            assert bool((a.p.t[~keep] != 0).any())                        # (which would have moved the zeros)
            assert torch.equal(x.s0.t, a.s0.t) and (a.s1 is None or torch.equal(x.s1.t, a.s1.t))   # moments: not masked


# ---- 4. a mixed call across the launch split ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ("adam", "sgd"))
def test_33_mixed_segments_equal_each_run_alone(algo):
    sizes = list(range(5, 38))
    assert len(sizes) == 33 > _lib.UPDATE_MAX_SEGS

    def build():
        out = []
        for i, n in enumerate(sizes):
            rank = None if i % 3 == 0 else 0 if i == 7 else optim.keep_rank(n, 0.4)
            out.append(make_seg(algo, n, 2, rank, seed=2))
        return out

    hy = c_hyper(algo, 1e-5)
    together, alone = build(), build()
    assert sum(x.sup is not None for x in together) == 22 and together[7].keep_rank == 0 and together[32].sup is not None
    run(together, hy, 0.01, 2, 1)
    for x in alone:
        run([x], hy, 0.01, 2, 1)
    for i, (a, b) in enumerate(zip(together, alone)):
        assert same_bits(a, b), sizes[i]
        start = U.segment(sizes[i], 2, 2)[0]
        assert not np.array_equal(a.p.t.cpu().numpy(), start)            # every segment was updated, the 33rd included
        if a.sup is not None:
            assert torch.equal(a.sup.t, (a.p.t != 0).to(torch.uint8))
            zeros = int((a.p.t == 0).sum())
            assert zeros == (0 if i == 7 else a.keep_rank), (i, zeros)    # distinct magnitudes: exactly keep_rank go


def test_unknown_mode_values_behave_as_none():
    a, b = make_seg("adam", 1025, 2, 300), make_seg("adam", 1025, 2, 300)
    run([a], c_hyper("adam", 0.0), 0.01, 2, 0)
    run([b], c_hyper("adam", 0.0), 0.01, 2, 3)
    assert same_bits(a, b)


# ---- 5. module level -------------------------------------------------------------------------------------------------
T, B, F, NCLS = 9, 37, 32, 12


def default_model(seed=0):
    torch.manual_seed(seed)
    return RNNClassifierModel("FastGRNNCUDA", F, 2, [256, 128], [None, None], [None, None], [0.3, 0.5], [0.2, 0.5],
                              "sigmoid", "tanh", num_classes=NCLS, device=DEV)


def batch(seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randn(T, B, F, generator=g).to(DEV), torch.randint(0, NCLS, (B,), generator=g).to(DEV)


def within_bound(model, start, grads, algo, h, t=1):
    """every parameter of `model` against the fp64 oracle of one step from `start` with `grads`; -> worst error / bound"""
    worst = 0.0
    for (name, p), p0, g in zip(model.named_parameters(), start, grads):
        z = np.zeros(p0.numel(), np.float32)
        a = (p0.cpu().numpy().reshape(-1), g.cpu().numpy().reshape(-1))
        if algo == "adam":
            ref, bound = U.adam_oracle(*a, z, z, U.lr32(h["lr"]), h["betas"], h["eps"], h["weight_decay"], t)[::3]
        else:
            ref, _, bound, _ = U.sgd_oracle(*a, z, U.lr32(h["lr"]), h["momentum"], 0.0, h["weight_decay"], h["nesterov"], t)
        err = np.abs(p.detach().cpu().numpy().reshape(-1) - ref)
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("algo", ("adam", "sgd"))
def test_train_step_against_torch_optim(algo):
    h = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5) if algo == "adam" else \
        dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-5)
    model = default_model()
    twin = copy.deepcopy(model)
    start = [p.detach().clone() for p in model.parameters()]
    x, y = batch()
    opt = (FusedAdam if algo == "adam" else FusedSGD)(model.parameters(), **h)
    assert opt.register_iht(model) == 4
    ref_opt = (torch.optim.Adam if algo == "adam" else torch.optim.SGD)(twin.parameters(), foreach=False, **h)
    loss = model.train_step(x, y, opt, iht="none")
    ref_loss = twin.loss(x, y)
    ref_loss.backward()
    ref_opt.step()
    assert not loss.requires_grad and torch.equal(loss, ref_loss.detach())
    grads = [p.grad.detach().clone() for p in model.parameters()]
    assert all(torch.equal(g, q.grad) for g, q in zip(grads, twin.parameters()))              # same gradients
    w_torch = within_bound(twin, start, grads, algo, h)                   # the bound holds for torch's fp32 step ...
    w = within_bound(model, start, grads, algo, h)                        # ... and then for the kernel
    print("%s module step: error / bound %.3f (torch.optim fp32: %.3f)" % (algo, w, w_torch))
    assert int(opt.step_t) == 1 and all(not torch.equal(p, p0) for p, p0 in zip(model.parameters(), start))
    for rnn in model.rnn_list:
        assert rnn.oldmats == []                                           # the layers' own IHT state is not touched


def test_threshold_step_is_hard_threshold_of_the_plain_step():
    model = default_model(1)
    twin = copy.deepcopy(model)
    x, y = batch(1)
    opts = [FusedAdam(m.parameters(), lr=0.01, weight_decay=1e-5) for m in (model, twin)]
    for o, m in zip(opts, (model, twin)):
        o.register_iht(m)
    model.train_step(x, y, opts[0], iht="none")
    twin.train_step(x, y, opts[1], iht="threshold")
    mats = {id(p): s for rnn in twin.rnn_list for p, s in ((rnn.W, rnn._wSparsity), (rnn.U, rnn._uSparsity))}
    assert len(mats) == 4
    for p, q in zip(model.parameters(), twin.parameters()):
        if id(q) in mats:
            assert torch.equal(q.detach(), utils.hardThreshold(p.detach().clone(), mats[id(q)]))
            assert torch.equal(opts[1].support(q), (q != 0).to(torch.uint8))
            assert abs(float((q != 0).float().mean()) - mats[id(q)]) < 0.01
        else:
            assert torch.equal(p, q)
        assert torch.equal(opts[0].state[p]["exp_avg"], opts[1].state[q]["exp_avg"])
    # the next "support" step keeps exactly that support
    before = {id(q): (q != 0) for q in twin.parameters() if id(q) in mats}
    twin.train_step(*batch(2), opts[1], iht="support")
    for q in twin.parameters():
        if id(q) in mats:
            assert bool((q[~before[id(q)]] == 0).all()) and bool((q[before[id(q)]] != 0).all())


def test_a_factorised_layer_registers_four_matrices():
    torch.manual_seed(2)
    layer = FastGRNNCUDA(F, 256, wRank=16, uRank=16, wSparsity=0.5, uSparsity=0.25, device=DEV)
    twin = copy.deepcopy(layer)
    opts = [FusedAdam(m.parameters(), lr=0.01) for m in (layer, twin)]
    assert [o.register_iht(m) for o, m in zip(opts, (layer, twin))] == [4, 4]
    x = batch(3)[0]
    for m, o, iht in ((layer, opts[0], "none"), (twin, opts[1], "threshold")):
        m(x).square().mean().backward()
        o.step(iht)
    for name, s in (("W1", 0.5), ("W2", 0.5), ("U1", 0.25), ("U2", 0.25)):
        p, q = getattr(layer, name), getattr(twin, name)
        assert torch.equal(q.detach(), utils.hardThreshold(p.detach().clone(), s)), name
        assert abs(float((q != 0).float().mean()) - s) < 0.01
    assert torch.equal(layer.bias_gate, twin.bias_gate) and torch.equal(layer.zeta, twin.zeta)


class TriangularLike:
    """writes param_groups[0]['lr'] each step, as the reference's utils.TriangularLR and torch's schedulers do"""

    def __init__(self, optimizer, lrs):
        self.optimizer, self.lrs, self.k = optimizer, lrs, 0

    def step(self):
        self.optimizer.param_groups[0]["lr"] = self.lrs[self.k]
        self.k += 1


def test_a_scheduler_that_writes_the_param_group_is_honoured():
    model = default_model(3)
    x, y = batch(4)
    h = dict(lr=0.05, momentum=0.0, nesterov=False, weight_decay=0.0)
    opt = FusedSGD(model.parameters(), **h)
    sched = TriangularLike(opt, [0.02, 0.007])
    for lr in (0.02, 0.007):
        start = [p.detach().clone() for p in model.parameters()]
        sched.step()                                                       # trainClassifier.py:244-249: before optimizer.step()
        model.train_step(x, y, opt)
        assert float(opt.lr_t) == np.float32(lr)
        grads = [p.grad.detach().clone() for p in model.parameters()]
        within_bound(model, start, grads, "sgd", dict(h, lr=lr))           # p - lr g with the NEW lr (no momentum: any t)
        big = max(range(len(start)), key=lambda i: float(grads[i].abs().max()))
        moved = (list(model.parameters())[big].detach() - start[big]).abs().max()
        assert abs(float(moved) / (lr * float(grads[big].abs().max())) - 1.0) < 1e-3
    torch_sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)               # torch's own, unchanged
    model.train_step(x, y, opt)
    torch_sched.step()
    model.train_step(x, y, opt)
    assert float(opt.lr_t) == np.float32(0.007 * 0.5)


# ---- 6. one graph for the run -------------------------------------------------------------------------------------------
def test_one_captured_graph_serves_changing_lr_and_iht_phase():
    plan = [("none", 0.01), ("threshold", 0.004), ("support", 0.02)]
    model = default_model(5)
    eager = copy.deepcopy(model)
    x, y = batch(5)

    # three eager steps
    e_opt = FusedAdam(eager.parameters(), lr=0.01, weight_decay=1e-5)
    e_opt.register_iht(eager)
    for iht, lr in plan:
        e_opt.param_groups[0]["lr"] = lr
        eager.init_hidden()
        eager.train_step(x, y, e_opt, iht=iht)

    # one capture; its warm-up steps are undone before the first replay
    opt = FusedAdam(model.parameters(), lr=0.01, weight_decay=1e-5, capturable=True)
    opt.register_iht(model)

    def fn():
        model.init_hidden()
        return model.train_step(x, y, opt, iht=None)

    step = GraphedStep(fn, undo=(model, opt))
    for iht, lr in plan:
        opt.lr_t.fill_(lr)
        opt.iht_t.fill_(optim.IHT_MODES[iht])
        step()
    torch.cuda.synchronize()
    assert int(opt.step_t) == 3 == int(e_opt.step_t)
    for (name, p), q in zip(model.named_parameters(), eager.parameters()):
        assert torch.equal(p, q), name
        assert torch.equal(opt.state[p]["exp_avg"], e_opt.state[q]["exp_avg"]), name
        assert torch.equal(opt.state[p]["exp_avg_sq"], e_opt.state[q]["exp_avg_sq"]), name
    for a, b in zip(model.rnn_list, eager.rnn_list):
        for pa, pb in ((a.W, b.W), (a.U, b.U)):
            assert torch.equal(opt.support(pa), e_opt.support(pb))
            assert 0 < int(opt.support(pa).sum()) < pa.numel() and bool((pa[opt.support(pa) == 0] == 0).all())


# ---- 7. the flows of tools/update_bench.py: fixed gradients, a phase that persists over many steps -------------------
def bench_model(kind="default"):
    """the models of tools/update_bench.py (sparsity 0.3 everywhere) with fixed gradients on every parameter"""
    torch.manual_seed(0)
    if kind == "default":
        m = RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None] * 2, [None] * 2, [0.3] * 2, [0.3] * 2,
                               "sigmoid", "tanh", num_classes=NCLS, device=DEV)
    else:
        m = RNNClassifierModel("FastGRNNBatchNormCUDA", 64, 3, [256, 128, 128], [None] * 3, [None] * 3, [0.3] * 3,
                               [0.3] * 3, "sigmoid", "tanh", num_classes=NCLS, device=DEV)
    for p in m.parameters():
        p.grad = 0.01 * torch.randn_like(p)
    return m


def iht_mats(model):
    return [p for rnn in model.rnn_list for p in getattr(rnn, "cell", rnn).getVars()[:2]]


def kept_counts(model):
    return [int((p != 0).sum()) for p in iht_mats(model)]


def sparse_counts(model):
    """what a threshold at sparsity 0.3 leaves of each W/U matrix when no two magnitudes tie"""
    return [p.numel() - optim.keep_rank(p.numel(), 0.3) for p in iht_mats(model)]


def dense_counts(model):
    return [p.numel() for p in iht_mats(model)]


@pytest.mark.parametrize("kind", ("default", "batchnorm3"))
def test_eager_threshold_step_then_many_support_steps(kind):
    """One "threshold" step right after construction, then 25 "support" steps on unchanged gradients: the support of
    the first step holds to the end, and a run of "none" steps after it fills the matrices again."""
    m = bench_model(kind)
    o = FusedAdam(m.parameters(), lr=0.01, weight_decay=1e-5)
    o.register_iht(m)
    o.step("threshold")
    print(kind, "after the threshold step: iht_t", int(o.iht_t), "kept", kept_counts(m), "of", dense_counts(m),
          "support", [int(o.support(p).sum()) for p in iht_mats(m)])
    assert kept_counts(m) == sparse_counts(m)
    assert [int(o.support(p).sum()) for p in iht_mats(m)] == sparse_counts(m)
    for _ in range(25):
        o.step("support")
    print(kind, "after 25 support steps: iht_t", int(o.iht_t), "kept", kept_counts(m))
    assert int(o.iht_t) == 2 and int(o.step_t) == 26
    assert kept_counts(m) == sparse_counts(m)
    for _ in range(3):
        o.step("none")
    assert kept_counts(m) == dense_counts(m)


@pytest.mark.parametrize("mode", ("threshold", "support", "none"))
@pytest.mark.parametrize("kind", ("default", "batchnorm3"))
def test_capture_with_the_iht_phase_already_set(kind, mode):
    """iht_t holds the phase BEFORE GraphedStep's warm-up and capture and is never written again: every replay runs
    that phase, bit for bit what the same number of eager steps gives.  (On unchanged gradients Adam's steps take few
    distinct magnitudes, so repeated thresholds meet ties, which survive: the eager twin is the reference, not a count.)"""
    m = bench_model(kind)
    twin = copy.deepcopy(m)
    for p, q in zip(m.parameters(), twin.parameters()):
        q.grad = p.grad.clone()
    o = FusedAdam(m.parameters(), lr=0.01, weight_decay=1e-5, capturable=True)
    e = FusedAdam(twin.parameters(), lr=0.01, weight_decay=1e-5)
    for opt, model in ((o, m), (e, twin)):
        opt.register_iht(model)
        opt.step("threshold")
    assert kept_counts(m) == sparse_counts(m)
    o.iht_t.fill_(optim.IHT_MODES[mode])
    step = GraphedStep(lambda: o.step(None))               # three warm-up steps, then the capture (which runs nothing)
    for _ in range(10):
        step()
    for _ in range(13):
        e.step(mode)
    torch.cuda.synchronize()
    print(kind, mode, "after 3 + 10 steps: iht_t", int(o.iht_t), "step_t", int(o.step_t), "kept", kept_counts(m))
    assert int(o.iht_t) == optim.IHT_MODES[mode] and int(o.step_t) == 14 == int(e.step_t)
    for (name, p), q in zip(m.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
    for p, q in zip(iht_mats(m), iht_mats(twin)):
        assert torch.equal(o.support(p), e.support(q))
    if mode == "none":
        assert kept_counts(m) == dense_counts(m)
    elif mode == "support":
        assert kept_counts(m) == sparse_counts(m)                          # the mask of the first step, exactly
    else:                                                                  # ties survive: never fewer, and not dense
        assert all(s <= k < n for k, s, n in zip(kept_counts(m), sparse_counts(m), dense_counts(m)))


def test_a_fused_step_moves_the_parameters_versions():
    """The library writes through raw pointers; step() tells torch, so that what is keyed on a tensor's version (the
    eval-mode BatchNorm fold cache, autograd's check of saved tensors) sees the update."""
    model = default_model(7)
    opt = FusedAdam(model.parameters(), lr=0.01)
    x, y = batch(7)
    before = [p._version for p in model.parameters()]
    model.train_step(x, y, opt)
    assert all(p._version > v for p, v in zip(model.parameters(), before))
