"""The gradient guard on the GPU: fastgrnn_hip_grad_guard against the restatement of tests/guard_cases.py (norm and coef
within one fp32 ulp, between canaries, the same bits twice), the eight rules under it (fastgrnn_hip_train_update_guarded,
fastgrnn_hip_optim_update_guarded) -- bit-equal to the unguarded calls at max_norm = inf, inside the existing derived
bounds of tests/update_cases.py / tests/optim_cases.py when they clip, the identity on a rejected step -- and what is
built on them: ``guard()`` on the fused optimizers, one captured ``train_step`` that meets a NaN batch, a guarded
``fit_audio``.  No test provokes a fault: NaN arithmetic is ordinary arithmetic."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import guard_cases as G
from tests import mfcc_cases as M
from tests import optim_cases as OC
from tests import support as S
from tests import update_cases as U

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import (AudioAugment, FusedAdam, GraphedStep, MFCCFrontend, RNNClassifierModel, TrainSchedule, _lib,
                         optim, utils)
DEV = torch.device("cuda:0")
PAD = 256                          # sentinel floats on each side of every buffer
SENTINEL = -7.25e11
UNWRITTEN = 123.0

# the eight rules, by the names tests/update_cases.py and tests/optim_cases.py give their settings
RULES = ("adam", "sgd", "rmsprop_centered_mom", "adagrad_decay", "adadelta", "adamax", "asgd_avg", "rprop")
KEYS = {"adam": ("exp_avg", "exp_avg_sq", None), "sgd": ("momentum_buffer", None, None)}


def is_update(rule):
    return rule in KEYS                                    # fastgrnn_hip_train_update's two rules


def keys_of(rule):
    return KEYS[rule] if is_update(rule) else OC.RULES[rule][2]


def wd_of(rule):
    return 0.0 if rule == "rprop" else 1e-5


def lr_of(rule):
    return U.hyper(rule, 0.0)["lr"] if is_update(rule) else OC.RULES[rule][1]["lr"]


def operands(rule, n, t, seed=1):
    """dict with p, g and the rule's state tensors by torch's keys (ASGD: eta and mu too)"""
    if not is_update(rule):
        return OC.segment(rule, n, t, seed)
    p, g, m, v, b = U.segment(n, t, seed)
    return {"p": p, "g": g, "exp_avg": m, "exp_avg_sq": v} if rule == "adam" else {"p": p, "g": g, "momentum_buffer": b}


def oracle(rule, wd, t, ops):
    """-> dict of (value64, bound) per output, by torch's keys"""
    if not is_update(rule):
        return OC.oracle(rule, wd, t, ops)
    z = np.zeros_like(ops["p"])
    o = U.oracle(rule, wd, t, ops["p"], ops["g"], ops.get("exp_avg", z), ops.get("exp_avg_sq", z),
                 ops.get("momentum_buffer", z))
    names = {"p": "p", "m": "exp_avg", "v": "exp_avg_sq", "b": "momentum_buffer"}
    return {names[k]: v for k, v in o.items()}


def torch_step(rule, wd, t, ops):
    if not is_update(rule):
        return OC.torch_cpu_step(rule, wd, t, ops)
    z = np.zeros_like(ops["p"])
    o = U.torch_cpu_step(rule, wd, t, ops["p"], ops["g"], ops.get("exp_avg", z), ops.get("exp_avg_sq", z),
                         ops.get("momentum_buffer", z))
    names = {"p": "p", "m": "exp_avg", "v": "exp_avg_sq", "b": "momentum_buffer"}
    return {names[k]: v for k, v in o.items()}


class Buf:
    """A device buffer of n elements with PAD sentinel floats (4 * PAD bytes for masks) on each side."""

    def __init__(self, values, dtype=torch.float32):
        values = torch.as_tensor(np.array(values)).to(dtype).reshape(-1)
        self.pad = PAD if dtype == torch.float32 else 4 * PAD
        self.fill = SENTINEL if dtype == torch.float32 else 0xA5
        self.whole = torch.full((values.numel() + 2 * self.pad,), self.fill, dtype=dtype, device=DEV)
        self.t = self.whole[self.pad:self.pad + values.numel()]
        self.t.copy_(values)

    def guards_intact(self):
        return bool((self.whole[:self.pad] == self.fill).all()) and bool((self.whole[-self.pad:] == self.fill).all())

    def bits(self):
        return self.t.view(torch.int32).clone() if self.t.dtype == torch.float32 else self.t.clone()

    def numpy(self):
        return self.t.cpu().numpy()


class Seg:
    """One segment's device state: p, g, the rule's state tensors in their slots and (IHT segments) the support mask."""

    def __init__(self, rule, ops, keep_rank=None, mask=None):
        self.rule = rule
        self.p, self.g = Buf(ops["p"]), Buf(ops["g"])
        self.keys = keys_of(rule)
        self.state = [Buf(ops[k]) if k else None for k in self.keys]
        self.keep_rank = keep_rank
        self.sup = None
        if keep_rank is not None:
            self.sup = Buf(np.full(len(ops["p"]), 9) if mask is None else mask, torch.uint8)

    def written(self):
        """every buffer a step may write"""
        return [b for b in [self.p, self.sup] + self.state if b is not None]

    def bufs(self):
        return self.written() + [self.g]

    def snapshot(self):
        return [b.bits() for b in self.written()]

    def c_seg(self):
        ptr = [b.t.data_ptr() if b else None for b in self.state]
        sup = self.sup.t.data_ptr() if self.sup else None
        tail = (sup, self.p.t.numel(), self.keep_rank or 0, 1 if self.sup else 0, 0)
        if is_update(self.rule):
            return _lib.UpdateSeg(self.p.t.data_ptr(), self.g.t.data_ptr(), ptr[0], ptr[1], *tail)
        return _lib.OptimSeg(self.p.t.data_ptr(), self.g.t.data_ptr(), tuple(ptr), *tail)

    def got(self):
        out = {"p": self.p.numpy()}
        out.update({k: b.numpy() for k, b in zip(self.keys, self.state) if k})
        return out


def c_hyper(rule, wd):
    if not is_update(rule):
        return OC.c_hyper(rule, wd)
    h = U.hyper(rule, wd)
    if rule == "adam":
        return _lib.UpdateHyper(_lib.ADAM, 0, h["betas"][0], h["betas"][1], h["eps"], wd)
    return _lib.UpdateHyper(_lib.SGD, int(h["nesterov"]), h["momentum"], h["dampening"], 0.0, wd)


class Guard:
    """The 32-byte state and the workspace of a guard, both between canaries."""

    def __init__(self, n_segs, applied=0, skipped=0):
        self.state = Buf(np.zeros(8, np.float32))
        nbytes = _lib.load().fastgrnn_hip_grad_guard_workspace_bytes(n_segs)
        self.ws = Buf(np.full(nbytes // 4, UNWRITTEN, np.float32))
        self.nbytes = nbytes
        self.state.t.view(torch.int64)[2:] = torch.tensor([applied, skipped], device=DEV)

    def read(self):
        f, i, q = self.state.t.cpu(), self.state.t.view(torch.int32).cpu(), self.state.t.view(torch.int64).cpu()
        return {"norm": f[0].numpy()[()], "coef": f[1].numpy()[()], "skip": int(i[2]), "reserved": int(i[3]),
                "applied": int(q[2]), "skipped": int(q[3])}

    def call(self, grads, max_norm=math.inf, flags=1):
        """grads: Bufs.  One fastgrnn_hip_grad_guard on the current stream."""
        arr = (_lib.GuardSeg * len(grads))(*[_lib.GuardSeg(b.t.data_ptr(), b.t.numel()) for b in grads])
        st = _lib.load().fastgrnn_hip_grad_guard(arr, len(grads), max_norm, flags, self.state.t.data_ptr(),
                                                 self.ws.t.data_ptr(), self.nbytes, torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "grad_guard")
        torch.cuda.synchronize()
        assert self.state.guards_intact() and self.ws.guards_intact(), "a sentinel next to the state or the workspace changed"
        assert all(b.guards_intact() for b in grads)
        return self.read()


def update(rule, wd, segs, mode, scalars=None, *, step=None, guard=None, lr=None):
    """One update call on the current stream: unguarded at ``step``, or under ``guard`` (a Guard already called)."""
    lib = _lib.load()
    lr_t = torch.tensor([lr_of(rule) if lr is None else lr], dtype=torch.float32, device=DEV)
    mode_t = torch.tensor([mode], dtype=torch.int32, device=DEV)
    cls = _lib.UpdateSeg if is_update(rule) else _lib.OptimSeg
    arr = (cls * len(segs))(*[s.c_seg() for s in segs])
    hy = c_hyper(rule, wd)
    if guard is None:
        count = torch.tensor([step], dtype=torch.int64, device=DEV)
        fn = lib.fastgrnn_hip_train_update if is_update(rule) else lib.fastgrnn_hip_optim_update
        count_ptr = count.data_ptr()
    else:
        fn = lib.fastgrnn_hip_train_update_guarded if is_update(rule) else lib.fastgrnn_hip_optim_update_guarded
        count_ptr = guard.state.t.data_ptr()
    extra = () if is_update(rule) else (scalars.t.data_ptr() if scalars else None,)
    st = fn(C.byref(hy), arr, len(segs), lr_t.data_ptr(), count_ptr, mode_t.data_ptr(), *extra,
            torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "update")
    torch.cuda.synchronize()
    for s in segs:
        assert all(b.guards_intact() for b in s.bufs()), "a sentinel next to a buffer of %d elements changed" % s.p.t.numel()
    assert scalars is None or scalars.guards_intact()
    assert guard is None or guard.state.guards_intact()


def guarded_step(rule, wd, segs, guard, mode=0, scalars=None, max_norm=math.inf, flags=1):
    verdict = guard.call([s.g for s in segs], max_norm, flags)
    update(rule, wd, segs, mode, scalars, guard=guard)
    return verdict


def scalars_for(rule, t, ops):
    """ASGD's double buffer before step t: what step t-1 left in its pair, a marker in the pair step t writes"""
    if rule not in ("asgd", "asgd_avg"):
        return None
    vals = [UNWRITTEN] * 4
    vals[2 * ((t - 1) & 1):2 * ((t - 1) & 1) + 2] = [ops["eta"], ops["mu"]]
    return Buf(np.array(vals, np.float32))


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.snapshot(), b.snapshot()))


def set_grad(seg, g):
    seg.g.t.copy_(torch.from_numpy(np.array(g)))


# ---- 1. the sum of squares -------------------------------------------------------------------------------------------------
SUMSQ_CASES = [((n,), 1.0) for n in G.SEG_SIZES] + [(G.SEG_SIZES, 30.0), (G.MIXED_SIZES, 1e-3), ((1 << 16,) * 2, 1.0)]


@pytest.mark.parametrize("sizes,scale", SUMSQ_CASES, ids=["%dx%d" % (len(s), s[0]) for s, _ in SUMSQ_CASES])
def test_norm_and_coef_against_the_restatement(sizes, scale):
    grads = [G.gradient(n, 10 + i, scale) for i, n in enumerate(sizes)]
    bufs = [Buf(g) for g in grads]
    root = math.sqrt(G.sumsq(grads))
    for max_norm in (0.37 * root, 3.0 * root, math.inf):
        want = G.restate(grads, max_norm)
        guard = Guard(len(sizes))
        got = guard.call(bufs, max_norm)
        print("n_segs %d, max_norm %g: norm %r (restated %r), coef %r (restated %r)"
              % (len(sizes), max_norm, got["norm"], want["norm"], got["coef"], want["coef"]))
        assert G.ulps_apart(got["norm"], want["norm"]) <= 1 and G.ulps_apart(got["coef"], want["coef"]) <= 1
        assert (got["skip"], got["reserved"], got["applied"], got["skipped"]) == (0, 0, 1, 0)
        assert (want["coef"] < 1.0) == (max_norm < root) and (max_norm < root or got["coef"] == 1.0)
        assert all(np.array_equal(b.numpy(), g) for b, g in zip(bufs, grads))           # the gradients are only read
        assert bool((guard.ws.t[2 * len(sizes):] == UNWRITTEN).all())                    # one double per segment, no more
        again = guard.call(bufs, max_norm)                                               # the same bits, counted once more
        assert again["norm"].tobytes() == got["norm"].tobytes() and again["coef"].tobytes() == got["coef"].tobytes()
        assert (again["applied"], again["skipped"]) == (2, 0)


# ---- 2. max_norm = inf, finite gradients: the unguarded call, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_without_clipping_the_guarded_call_is_the_unguarded_call(rule):
    sizes, wd = (1, 1023, 1025, 4097), wd_of(rule)
    ops = [operands(rule, n, 1) for n in sizes]
    plain = [Seg(rule, o) for o in ops]
    guarded = [Seg(rule, o) for o in ops]
    sc = [Buf(np.full(4, UNWRITTEN, np.float32)) if rule == "asgd_avg" else None for _ in range(2)]
    guard = Guard(len(sizes))
    for t in (1, 2, 3):
        for n, a, b in zip(sizes, plain, guarded):
            g = operands(rule, n, t, seed=20 + t)["g"]                   # fresh gradients every step
            set_grad(a, g)
            set_grad(b, g)
        update(rule, wd, plain, 0, sc[0], step=t)
        verdict = guarded_step(rule, wd, guarded, guard, 0, sc[1])
        assert (verdict["coef"], verdict["skip"], verdict["applied"], verdict["skipped"]) == (1.0, 0, t, 0)
        for n, a, b in zip(sizes, plain, guarded):
            assert same_bits(a, b), (rule, t, n)
        assert sc[0] is None or torch.equal(sc[0].bits(), sc[1].bits())
    assert not np.array_equal(guarded[1].p.numpy(), ops[1]["p"])         # (something happened)


# ---- 3. clipping: the existing oracles on the fp32 product g coef ------------------------------------------------------------
@pytest.mark.parametrize("t", U.STEPS)
@pytest.mark.parametrize("rule", RULES)
def test_a_clipped_step_meets_the_existing_bound(rule, t):
    sizes, wd = (1, 1025, 3079), wd_of(rule)
    ops = [operands(rule, n, t) for n in sizes]
    segs = [Seg(rule, o) for o in ops]
    sc = scalars_for(rule, t, ops[0])
    guard = Guard(len(sizes), applied=t - 1)                             # the rules count the steps taken: this is step t
    max_norm = 0.1 * math.sqrt(G.sumsq([o["g"] for o in ops]))
    verdict = guarded_step(rule, wd, segs, guard, 0, sc, max_norm)
    coef = verdict["coef"]
    assert abs(float(coef) - 0.1) < 1e-4 and verdict["applied"] == t and verdict["skip"] == 0
    for n, o, s in zip(sizes, ops, segs):
        clipped = dict(o, g=(o["g"] * coef).astype(np.float32))          # the one fp32 multiply, with the kernel's own coef
        ref = oracle(rule, wd, t, clipped)
        w_torch = OC.worst(torch_step(rule, wd, t, clipped), ref)
        assert max(w_torch.values()) <= 1.0, ("the bound is wrong: torch's fp32 step misses it", n, w_torch)
        got = s.got()
        if sc is not None:
            written = sc.numpy()[2 * (t & 1):][:2]
            got.update(eta=np.float64(written[0]), mu=np.float64(written[1]))
        w = OC.worst(got, ref)
        print("%s t=%d n=%d coef=%r: error / bound %s (torch fp32: %s)" % (rule, t, n, coef, w, w_torch))
        assert max(w.values()) <= 1.0, (n, w)
        assert np.array_equal(s.g.numpy(), o["g"])                       # the gradient tensor itself is not scaled


# ---- 4. a rejected step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ("first", "last"))
@pytest.mark.parametrize("bad", G.BAD_VALUES, ids=("nan", "inf", "-inf"))
@pytest.mark.parametrize("rule", RULES)
def test_a_nonfinite_gradient_is_skipped_and_the_run_goes_on_as_if_it_never_came(rule, bad, where):
    sizes, wd, t = G.MIXED_SIZES, wd_of(rule), 2
    assert len(sizes) == 33 > _lib.UPDATE_MAX_SEGS
    ops = [operands(rule, n, t, seed=2) for n in sizes]
    segs, twin = [Seg(rule, o) for o in ops], [Seg(rule, o) for o in ops]
    sc, sc_twin = scalars_for(rule, t, ops[0]), scalars_for(rule, t, ops[0])
    before = [s.snapshot() for s in segs]
    if where == "first":
        segs[0].g.t[0] = bad
    else:
        segs[32].g.t[-1] = bad
    guard = Guard(33, applied=t - 1)
    verdict = guarded_step(rule, wd, segs, guard, 0, sc)
    assert (verdict["skip"], verdict["coef"], verdict["applied"], verdict["skipped"]) == (1, 0.0, t - 1, 1)
    assert not np.isfinite(verdict["norm"])
    for s, snap in zip(segs, before):
        assert all(torch.equal(x, y) for x, y in zip(s.snapshot(), snap)), (rule, s.p.t.numel())
    assert sc is None or torch.equal(sc.bits(), sc_twin.bits())          # ASGD's scalars: neither pair was written
    # the next, finite step: the bits of an unguarded run that never saw the bad one
    for s, o in zip(segs, ops):
        set_grad(s, o["g"])
    verdict = guarded_step(rule, wd, segs, guard, 0, sc)
    assert (verdict["skip"], verdict["coef"], verdict["applied"], verdict["skipped"]) == (0, 1.0, t, 1)
    update(rule, wd, twin, 0, sc_twin, step=t)
    for n, a, b in zip(sizes, segs, twin):
        assert same_bits(a, b), (rule, n)
        assert not np.array_equal(a.p.numpy(), operands(rule, n, t, seed=2)["p"])
    assert sc is None or torch.equal(sc.bits(), sc_twin.bits())


@pytest.mark.parametrize("rule", ("adam", "asgd_avg"))
def test_the_iht_phase_still_runs_on_a_skipped_step(rule):
    n, t, s, wd = 3079, 2, 0.3, wd_of(rule)
    o = operands(rule, n, t)
    mask = (np.random.default_rng(5).random(n) < 0.6).astype(np.uint8)
    small = operands(rule, 37, t)

    def build():
        return [Seg(rule, o, optim.keep_rank(n, s), mask), Seg(rule, small, 0, np.ones(37, np.uint8)), Seg(rule, small)]

    for mode in (1, 2):
        segs = build()
        before = [x.snapshot() for x in segs]
        segs[2].g.t[3] = float("nan")
        sc = scalars_for(rule, t, o)
        sc_before = sc.bits() if sc else None
        verdict = guarded_step(rule, wd, segs, Guard(3, applied=t - 1), mode, sc)
        assert (verdict["skip"], verdict["applied"], verdict["skipped"]) == (1, t - 1, 1)
        p0 = torch.from_numpy(np.array(o["p"])).to(DEV)
        if mode == 1:                                                    # threshold p as it stands, record the support
            assert torch.equal(segs[0].p.t, utils.hardThreshold(p0.clone(), s))
            assert torch.equal(segs[0].sup.t, (segs[0].p.t != 0).to(torch.uint8)) and 0 < int(segs[0].sup.t.sum()) < n
            assert torch.equal(segs[1].p.bits(), before[1][0])           # keep_rank 0: everything survives ...
            assert torch.equal(segs[1].sup.t, (segs[1].p.t != 0).to(torch.uint8))          # ... and the support says so
        else:                                                            # mask with the recorded support, which is only read
            keep = torch.from_numpy(mask).to(DEV).bool()
            assert bool((segs[0].p.t[~keep] == 0).all()) and torch.equal(segs[0].p.t[keep], p0[keep])
            assert torch.equal(segs[0].sup.t, torch.from_numpy(mask).to(DEV))
            assert torch.equal(segs[1].p.bits(), before[1][0])
        for x, snap in zip(segs, before):                                # no state tensor moved, nor the plain segment
            for b, was in list(zip(x.written(), snap))[2 if x.sup else 1:]:
                assert torch.equal(b.bits(), was)
        assert torch.equal(segs[2].p.bits(), before[2][0])
        assert sc is None or torch.equal(sc.bits(), sc_before)


def test_without_skip_nonfinite_a_nan_gradient_propagates_as_it_does_today():
    rule, wd, t, sizes = "adam", 1e-5, 2, (37, 1025)
    ops = [operands(rule, n, t) for n in sizes]
    segs, twin = [Seg(rule, o) for o in ops], [Seg(rule, o) for o in ops]
    for x in (segs, twin):
        x[1].g.t[7] = float("nan")
    verdict = guarded_step(rule, wd, segs, Guard(2, applied=t - 1), flags=0)              # max_norm = inf: coef 1
    assert (verdict["skip"], verdict["coef"], verdict["applied"], verdict["skipped"]) == (0, 1.0, t, 0)
    assert np.isnan(verdict["norm"])
    update(rule, wd, twin, 0, step=t)
    for a, b in zip(segs, twin):
        assert same_bits(a, b)
    assert bool(torch.isnan(segs[1].p.t[7])) and int(torch.isnan(segs[1].p.t).sum()) == 1
    # with a finite max_norm the coefficient is clip_grad_norm_'s NaN, which reaches every element
    segs = [Seg(rule, o) for o in ops]
    segs[1].g.t[7] = float("nan")
    verdict = guarded_step(rule, wd, segs, Guard(2, applied=t - 1), max_norm=1.0, flags=0)
    assert verdict["skip"] == 0 and np.isnan(verdict["coef"]) and verdict["applied"] == t
    assert all(bool(torch.isnan(x.p.t).all()) for x in segs)


# ---- 5. module level: one captured train_step meets a NaN batch --------------------------------------------------------------
T, B, F, NCLS = 4, 16, 32, 12


def small_model(seed=0):
    torch.manual_seed(seed)
    return RNNClassifierModel("FastGRNNCUDA", F, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                              num_classes=NCLS, device=DEV)


def batch(k):
    g = torch.Generator().manual_seed(900 + k)
    x = torch.randn(T, B, F, generator=g)
    if k == 3:
        x[1, 5, 7] = float("nan")                                          # the third replay's batch, and only it
    return x.to(DEV), torch.randint(0, NCLS, (B,), generator=g).to(DEV)


def test_one_captured_train_step_rejects_a_nan_batch_and_goes_on():
    model = small_model()
    eager = copy.deepcopy(model)
    opt = FusedAdam(model.parameters(), lr=0.01, weight_decay=1e-5, capturable=True).guard(max_grad_norm=5.0)
    e_opt = FusedAdam(eager.parameters(), lr=0.01, weight_decay=1e-5).guard(max_grad_norm=5.0)
    x, y = (t.clone() for t in batch(0))

    def fn():
        model.init_hidden()
        return model.train_step(x, y, opt, iht=None)

    step = GraphedStep(fn, undo=(model, opt))
    for k in range(1, 7):
        xb, yb = batch(k)
        x.copy_(xb)
        y.copy_(yb)
        loss = step()
        eager.init_hidden()
        e_loss = eager.train_step(xb, yb, e_opt)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters()), k
        assert int(opt.skip_t) == (1 if k == 3 else 0), k
        if k >= 4:
            for (name, p), q in zip(model.named_parameters(), eager.parameters()):
                S.assert_same_bits(p.detach(), q.detach(), "replay %d: %s" % (k, name))
                for key in ("exp_avg", "exp_avg_sq"):
                    S.assert_same_bits(opt.state[p][key], e_opt.state[q][key], "replay %d: %s of %s" % (k, key, name))
            S.assert_same_bits(loss, e_loss, "replay %d: the loss" % k)
    assert (int(opt.skipped_t), int(opt.applied_t), int(opt.step_t)) == (1, 5, 6)
    assert (int(e_opt.skipped_t), int(e_opt.applied_t), int(e_opt.step_t)) == (1, 5, 6)
    assert 0.0 < float(opt.grad_norm_t) < math.inf and 0.0 < float(opt.clip_coef_t) <= 1.0
    sd = opt.state_dict()
    assert sd["guard"] == {"applied": 5, "skipped": 1} and sd["fused_step"] == 6 and float(sd["state"][0]["step"]) == 5.0


# ---- 6. a guarded fit_audio: every iteration clips, graph and eager give the same bits ------------------------------------------
MAX_GRAD_NORM = 1e-3
SEED = (0xC0FFEE << 32) | 0x1234
N_CLIPS, L_MAX, BATCH, NUM_EPOCHS, TRIM, LR = 50, 4000, 8, 3, 2, 0.01       # the run of tests/test_hip_schedule.py


def audio_bank():
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


def test_a_guarded_fit_audio_clips_every_iteration_the_same_from_a_graph_and_eagerly():
    bank, lengths, labels, aug, fe = audio_bank()
    torch.manual_seed(5)
    start = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [0.5], [0.5], "sigmoid", "tanh",
                               num_classes=12, device=DEV)

    def trainer():
        model = copy.deepcopy(start)
        opt = FusedAdam(model.parameters(), lr=LR, capturable=True).guard(max_grad_norm=MAX_GRAD_NORM)
        assert opt.register_iht(model) == 2
        sched = TrainSchedule(opt, N_CLIPS, BATCH, NUM_EPOCHS, seed=SEED, lr_scheduler="StepLR", gamma=0.5,
                              lr_step_size=6, sparsify=True, trim_level=TRIM)
        return model, opt, sched

    graphed, eager = trainer(), trainer()
    coefs, eager_step = [], eager[1].step

    def logging_step(*args, **kw):                         # the kernel's own coefficient after every eager iteration
        out = eager_step(*args, **kw)
        coefs.append(eager[1].clip_coef_t.clone())
        return out

    eager[1].step = logging_step
    log = graphed[0].fit_audio(bank, lengths, labels, fe, aug, graphed[1], graphed[2], graph=True)
    e_log = eager[0].fit_audio(bank, lengths, labels, fe, aug, eager[1], eager[2], graph=False)
    assert graphed[2].total_iterations == 18 == int(graphed[1].step_t) == int(eager[1].step_t)
    for (name, p), q in zip(graphed[0].named_parameters(), eager[0].parameters()):
        S.assert_same_bits(p.detach(), q.detach(), "graph against eager: %s" % name)
        for k in ("exp_avg", "exp_avg_sq"):
            S.assert_same_bits(graphed[1].state[p][k], eager[1].state[q][k], "graph against eager: %s of %s" % (k, name))
    for pa, pb in ((graphed[0].rnn_list[0].W, eager[0].rnn_list[0].W), (graphed[0].rnn_list[0].U, eager[0].rnn_list[0].U)):
        S.assert_same_bits(graphed[1].support(pa), eager[1].support(pb), "graph against eager: a support mask")
    for name in ("loss_log", "lr_log", "norm_log", "skip_log"):
        S.assert_same_bits(getattr(graphed[2], name), getattr(eager[2], name), name + ", graph against eager")
    norms = graphed[2].norm_log.tolist()
    assert len(norms) == 18 and all(math.isfinite(v) for v in norms)
    coefs = torch.cat(coefs).tolist()                      # (the eager run is the graphed one bit for bit, logs included)
    assert len(coefs) == 18 and all(0.0 < c < 1.0 for c in coefs), coefs                   # every coef < 1
    # ... and it is the logged norm's: norm_log holds sqrt(S) rounded to fp32 (2^-24 relative), the coefficient is one
    # more rounding of the quotient, so the two agree to 2^-23 relative: two ulps at the most
    assert all(G.ulps_apart(c, np.float32(MAX_GRAD_NORM / (v + 1e-6))) <= 2 for c, v in zip(coefs, norms))
    assert 0.0 < float(graphed[1].clip_coef_t) < 1.0
    assert graphed[2].skip_log.tolist() == [0] * 18
    assert (int(graphed[1].applied_t), int(graphed[1].skipped_t)) == (18, 0)               # (the warm-up was undone)
    assert [e["skipped"] for e in log] == [0, 0, 0] and [e["grad_norm"] for e in log] == [norms[i] for i in (5, 11, 17)]
    assert [(e["loss"], e["skipped"], e["grad_norm"]) for e in e_log] == [(e["loss"], e["skipped"], e["grad_norm"]) for e in log]
