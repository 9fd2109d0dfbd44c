"""CPU-side checks of the six further fused optimizers (fastgrnn_hip_optim_update, kws_amd/optim.py): the fp64 oracles
the GPU tests compare against, held to torch.optim in fp64; torch's own fp32 step inside the derived bounds on the GPU
tests' operands; the entry point's argument checks without a launch; construction, limits and checkpoints to and from
torch.optim on CPU tensors; configure_optimizer; and that the radix select exists once (the static scans of the kernel
source, which all eight rules share, are tests/test_update_cpu.py's)."""
import copy
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from kws_amd import _lib, optim
from tests import optim_cases as OC
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, ONE = None, 256                                   # (a fake non-NULL pointer: nothing is launched)
OK, NULLP, SHAPE, UNSUP = 0, 1, 2, 7
FUSED = {"RMSprop": optim.FusedRMSprop, "Adagrad": optim.FusedAdagrad, "Adadelta": optim.FusedAdadelta,
         "Adamax": optim.FusedAdamax, "ASGD": optim.FusedASGD, "Rprop": optim.FusedRprop}


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


# ---- the oracles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,t,wd", OC.CASES)
def test_oracle_is_torch_optim_in_fp64(rule, t, wd):
    ops = OC.segment(rule, 1025, t, seed=3)
    ref = OC.torch_cpu_step(rule, wd, t, ops, dtype=torch.float64)
    for name, (val, _) in OC.oracle(rule, wd, t, ops).items():
        # (torch rounds ASGD's eta and mu to fp32 whatever the parameters' dtype: one rounding)
        rtol = OC.u if name in ("eta", "mu") else 1e-11
        np.testing.assert_allclose(val, ref[name], rtol=rtol, atol=0, err_msg=name)


def test_two_consecutive_asgd_steps_carry_eta_and_mu():
    """the scalars one step leaves are the ones the next reads: the oracle chained twice is torch stepping twice"""
    rule, wd, t = "asgd_avg", 1e-5, 7
    ops = dict(OC.segment(rule, 1025, t, seed=4))
    h = dict(OC.hyper(rule, wd), lr=OC.f32(0.01))
    q = torch.nn.Parameter(torch.from_numpy(np.array(ops["p"])).double())
    opt = torch.optim.ASGD([q], foreach=False, **h)
    opt.state[q] = OC.torch_state(rule, t, ops, torch.float64)
    for k in range(2):
        q.grad = torch.from_numpy(np.array(ops["g"])).double()
        opt.step()
        out = {n: v for n, (v, _) in OC.oracle(rule, wd, t + k, ops).items()}
        np.testing.assert_allclose(out["p"], q.detach().numpy(), rtol=1e-11)
        np.testing.assert_allclose(out["ax"], opt.state[q]["ax"].numpy(), rtol=1e-11)
        assert OC.f32(out["eta"]) == float(opt.state[q]["eta"]) and OC.f32(out["mu"]) == float(opt.state[q]["mu"])
        ops.update(p=out["p"], ax=out["ax"], eta=OC.f32(out["eta"]), mu=OC.f32(out["mu"]))      # (stored as fp32)
    assert ops["mu"] < 1.0


@pytest.mark.parametrize("rule,t,wd", OC.CASES)
def test_torch_fp32_meets_the_bound_on_the_gpu_tests_operands(rule, t, wd):
    """The bounds are not tighter than a faithful fp32 implementation needs: torch's own fp32 step, on the operands of
    tests/test_hip_optim.py, stays inside them."""
    for n in OC.SIZES:
        ops = OC.segment(rule, n, t, seed=1)
        w = OC.worst(OC.torch_cpu_step(rule, wd, t, ops), OC.oracle(rule, wd, t, ops))
        assert max(w.values()) <= 1.0, (n, w)


def test_the_operands_are_what_the_bounds_assume():
    for t in (2, 1000):
        o = OC.segment("rmsprop_centered_mom", 65536, t, seed=1)
        assert (np.abs(o["grad_avg"]) <= 0.5 * np.sqrt(o["square_avg"]) * (1 + 1e-6)).all()
        ref = OC.oracle("rmsprop_centered_mom", 1e-5, t, o)
        assert np.isfinite(ref["p"][0]).all() and np.isfinite(ref["p"][1]).all()
        r = OC.segment("rprop", 65536, t, seed=1)
        for a in (r["g"], r["prev"]):
            assert (a == 0).any() and (np.abs(a[a != 0]) > 1e-6).all()
        ref = OC.oracle("rprop", 0.0, t, r)
        assert (ref["step_size"][0] == 1e-6).any() and (ref["step_size"][0] == 50.0).any()       # both clamps
        assert (ref["prev"][0][r["g"] * r["prev"] < 0] == 0).all() and (r["g"] * r["prev"] < 0).any()
    first = OC.segment("rprop", 1025, 1, seed=1)
    assert not first["prev"].any() and (first["step_size"] == np.float32(0.01)).all()
    a = OC.segment("asgd_avg", 1025, 1000, seed=1)
    assert a["mu"] == np.float32(1 / 998) and a["eta"] != np.float32(0.01)
    assert OC.segment("asgd", 1025, 1000, seed=1)["mu"] == 1.0 != OC.segment("asgd", 1025, 1000, seed=1)["eta"]


# ---- argument checks of the entry point, no launch ---------------------------------------------------------------------
def _seg(**kw):
    d = dict(param=ONE, grad=ONE, state=(ONE, ONE, ONE), support=NULL, n=100, keep_rank=0, iht=0, reserved=0)
    d.update(kw)
    return _lib.OptimSeg(**d)


GOOD = {2: (0.99, 1e-8, 0.9), 3: (0.0, 1e-10), 4: (0.9, 1e-6), 5: (0.9, 0.999, 1e-8), 6: (1e-4, 0.75, 1e6),
        7: (0.5, 1.2, 1e-6, 50.0)}


def _hyper(algo=2, flags=0, h=None, wd=0.0):
    return _lib.OptimHyper(algo, flags, tuple(GOOD.get(algo, ()) if h is None else h), wd)


def _update(lib, segs=None, h=None, n_segs=None, lr=ONE, step=ONE, mode=ONE, scalars=ONE, no_h=False, no_segs=False):
    segs = [_seg()] if segs is None else segs
    arr = (_lib.OptimSeg * len(segs))(*segs)
    h = _hyper() if h is None else h
    return lib.fastgrnn_hip_optim_update(None if no_h else C.byref(h), None if no_segs else arr,
                                         len(segs) if n_segs is None else n_segs, lr, step, mode, scalars, None)


def test_symbol_and_structures(lib):
    assert hasattr(lib, "fastgrnn_hip_optim_update") and "fastgrnn_hip_optim_update" in _lib.EXPORTS
    assert lib.fastgrnn_hip_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    assert "fastgrnn_hip_optim_update(" in header
    # void* x 2, void*[3], uint8_t*, int64 x 2, int32 x 2;  int32 x 2, double[6], double
    assert C.sizeof(_lib.OptimSeg) == 72 and C.sizeof(_lib.OptimHyper) == 64
    assert _lib.OptimSeg.n.offset == 48 and _lib.OptimSeg.iht.offset == 64 and _lib.OptimHyper.weight_decay.offset == 56
    assert C.sizeof(_lib.UpdateSeg) == 64 and C.sizeof(_lib.UpdateHyper) == 40            # the first call's: untouched


def test_null_pointers(lib):
    assert _update(lib, no_h=True) == NULLP
    assert _update(lib, no_segs=True) == NULLP
    assert _update(lib, lr=NULL) == NULLP
    assert _update(lib, step=NULL) == NULLP
    for algo in GOOD:
        h = _hyper(algo, 1 if algo == 2 else 0)
        assert _update(lib, [_seg(n=0)], h) == SHAPE                                       # (every pointer check passes)
        for name in ("param", "grad"):
            assert _update(lib, [_seg(**{name: NULL})], h) == NULLP, (algo, name)
        assert _update(lib, [_seg(), _seg(), _seg(grad=NULL)], h) == NULLP                 # every segment is looked at
        assert _update(lib, [_seg(iht=1, support=NULL)], h) == NULLP
        assert _update(lib, [_seg(iht=1, support=ONE)], h, mode=NULL) == NULLP             # an IHT segment needs the mode
        assert _update(lib, [_seg(n=0)], h, mode=NULL) == SHAPE                            # ... no other segment does
    # the state tensors a rule needs, and only those: (algo, flags, h) -> the slots that must not be NULL
    needs = [((2, 0, (0.99, 1e-8, 0.0)), (0,)), ((2, 0, (0.99, 1e-8, 0.9)), (0, 1)), ((2, 1, (0.99, 1e-8, 0.0)), (0, 2)),
             ((2, 1, (0.99, 1e-8, 0.9)), (0, 1, 2)), ((3, 0, None), (0,)), ((4, 0, None), (0, 1)), ((5, 0, None), (0, 1)),
             ((6, 0, None), (0,)), ((7, 0, None), (0, 1))]
    for (algo, flags, h), slots in needs:
        hy = _hyper(algo, flags, h)
        for j in range(3):
            state = tuple(NULL if i == j else ONE for i in range(3))
            want = NULLP if j in slots else SHAPE
            assert _update(lib, [_seg(state=state, n=0)], hy) == want, (algo, flags, j)
    # ASGD's scalars, and nobody else's
    assert _update(lib, h=_hyper(6), scalars=NULL) == NULLP
    for algo in (2, 3, 4, 5, 7):
        assert _update(lib, [_seg(n=0)], _hyper(algo), scalars=NULL) == SHAPE


def test_bad_shapes(lib):
    assert _update(lib, n_segs=0) == SHAPE
    assert _update(lib, n_segs=-1) == SHAPE
    for n in (0, -5, (1 << 22) + 1):
        assert _update(lib, [_seg(n=n)]) == SHAPE, n
    assert _update(lib, [_seg(n=10, keep_rank=10)]) == SHAPE
    assert _update(lib, [_seg(n=10, keep_rank=-1)]) == SHAPE
    nan = float("nan")
    bad = [(2, (-0.1, 1e-8, 0.0)), (2, (0.99, 0.0, 0.0)), (2, (0.99, -1e-8, 0.0)), (2, (0.99, 1e-8, -0.1)), (2, (nan, 1e-8, 0.0)),
           (3, (-1e-3, 1e-10)), (3, (0.0, 0.0)), (3, (nan, 1e-10)),
           (4, (-0.1, 1e-6)), (4, (1.1, 1e-6)), (4, (0.9, 0.0)), (4, (0.9, nan)),
           (5, (1.0, 0.999, 1e-8)), (5, (-0.1, 0.999, 1e-8)), (5, (0.9, 1.0, 1e-8)), (5, (0.9, -0.5, 1e-8)), (5, (0.9, 0.999, 0.0)),
           (6, (nan, 0.75, 1e6)), (6, (1e-4, nan, 1e6)), (6, (1e-4, 0.75, nan)),
           (7, (0.0, 1.2, 1e-6, 50.0)), (7, (1.0, 1.2, 1e-6, 50.0)), (7, (0.5, 1.0, 1e-6, 50.0)), (7, (0.5, 0.9, 1e-6, 50.0)),
           (7, (0.5, 1.2, 51.0, 50.0)), (7, (0.5, nan, 1e-6, 50.0))]
    for algo, h in bad:
        assert _update(lib, h=_hyper(algo, 0, h)) == SHAPE, (algo, h)
    for algo in (2, 3, 4, 5, 6):
        assert _update(lib, h=_hyper(algo, wd=-1e-5)) == SHAPE, algo
        assert _update(lib, h=_hyper(algo, wd=nan)) == SHAPE, algo
    for wd in (1e-5, -1e-5, nan):
        assert _update(lib, h=_hyper(7, wd=wd)) == SHAPE                                    # Rprop takes no weight decay
    # what torch's constructors accept stays legal: rho = 0 and 1, alpha = 0 and above 1, a large momentum
    for algo, h in ((4, (0.0, 1e-8)), (4, (1.0, 1e-6)), (2, (0.0, 1e-8, 0.9)), (2, (1.5, 1e-8, 2.0)), (7, (0.5, 1.2, 1.0, 1.0))):
        assert _update(lib, [_seg(param=NULL)], _hyper(algo, 0, h)) == NULLP, (algo, h)     # (the next refusal in line)


def test_algo_codes(lib):
    for algo in (0, 1, -1, 8, 100):                       # Adam and SGD belong to the first call
        assert _update(lib, h=_hyper(algo, 0, (0.9, 0.999, 1e-8))) == UNSUP, algo
    upd = lambda algo: lib.fastgrnn_hip_train_update(
        C.byref(_lib.UpdateHyper(algo, 0, 0.9, 0.999, 1e-8, 0.0)),
        (_lib.UpdateSeg * 1)(_lib.UpdateSeg(ONE, ONE, ONE, ONE, NULL, 0, 0, 0, 0)), 1, ONE, ONE, ONE, None)
    assert upd(0) == SHAPE and upd(1) == SHAPE            # (n = 0: their next refusal)
    for algo in range(2, 8):                              # ... and the first call still refuses the new codes
        assert upd(algo) == UNSUP, algo


# ---- the optimizers on CPU tensors: construction, limits, checkpoints ------------------------------------------------
def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(5, 7, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g)),
            torch.nn.Parameter(torch.randn(1, 1, generator=g))]


CLASS_RULES = ("rmsprop_centered_mom", "rmsprop", "adagrad_decay", "adadelta", "adamax", "asgd_avg", "rprop")


@pytest.mark.parametrize("rule", CLASS_RULES)
def test_construction_needs_no_gpu_and_step_does(rule):
    ps = _params()
    k, h = OC.kind(rule), OC.hyper(rule, 1e-5)
    opt = FUSED[k](ps, **h)
    ref = getattr(torch.optim, k)(_params(), **h)
    assert set(ref.param_groups[0]) <= set(opt.param_groups[0]) <= set(ref.param_groups[0]) | {"capturable"}
    assert all(opt.param_groups[0][key] == v for key, v in ref.param_groups[0].items() if key != "params")
    assert isinstance(opt, optim._FusedOptimizer) and opt.param_groups[0]["capturable"] is False
    assert opt.lr_t.dtype == torch.float32 and opt.step_t.dtype == torch.int64 and opt.iht_t.dtype == torch.int32
    assert float(opt.lr_t) == np.float32(h["lr"]) and int(opt.step_t) == 0 and int(opt.iht_t) == 0
    # state exists where torch's does: Adagrad creates it when constructed, the others at the first step
    assert {p: set(st) for p, st in opt.state.items()} == {p: set(st) for p, st in zip(ps, ref.state.values())} \
        or (k != "Adagrad" and not opt.state and not ref.state)
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    segs, n = opt._segments()                             # the table, on CPU tensors: slots as the library reads them
    assert n == 3 and isinstance(segs[0], _lib.OptimSeg)
    for slot, key in enumerate(OC.RULES[rule][2]):
        assert segs[1].state[slot] == (opt.state[ps[1]][key].data_ptr() if key else None), (slot, key)
    assert set(opt.state[ps[0]]) - {"step"} == set(OC.keys(rule))
    if k == "Rprop":
        assert bool((opt.state[ps[0]]["step_size"] == h["lr"]).all()) and not opt.state[ps[0]]["prev"].any()
    if k == "ASGD":
        assert opt.scalars.dtype == torch.float32 and opt.scalars.tolist() == [np.float32(h["lr"]), 1.0] * 2


def test_adagrad_fills_the_accumulator_when_constructed():
    ps = _params()
    opt = optim.FusedAdagrad(ps, initial_accumulator_value=0.25)
    assert all(bool((opt.state[p]["sum"] == 0.25).all()) and float(opt.state[p]["step"]) == 0.0 for p in ps)


def test_limits_are_named():
    ps = _params()
    for k, cls in FUSED.items():
        with pytest.raises(ValueError, match="one param group"):
            cls([{"params": ps[:1]}, {"params": ps[1:]}])
        with pytest.raises(ValueError, match="float32"):
            cls([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
        with pytest.raises(ValueError, match="contiguous"):
            cls([torch.nn.Parameter(torch.zeros(4, 6).t())])
        with pytest.raises(ValueError, match="maximize"):
            cls(ps, maximize=True)
        with pytest.raises(ValueError, match="differentiable"):
            cls(ps, differentiable=True)
        with pytest.raises(ValueError, match="float lr"):
            cls(ps, lr=torch.tensor(0.01))
        with pytest.raises(ValueError, match="one param group"):
            cls(ps).add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})
    with pytest.raises(ValueError, match="eps > 0"):
        optim.FusedRMSprop(ps, eps=0.0)
    with pytest.raises(ValueError, match="momentum >= 0"):
        optim.FusedRMSprop(ps, momentum=-0.5)
    with pytest.raises(ValueError, match="lr_decay >= 0"):
        optim.FusedAdagrad(ps, lr_decay=-1.0)
    with pytest.raises(ValueError, match=r"rho in \[0,1\]"):
        optim.FusedAdadelta(ps, rho=1.5)
    with pytest.raises(ValueError, match="betas"):
        optim.FusedAdamax(ps, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="weight_decay >= 0"):
        optim.FusedASGD(ps, weight_decay=-1.0)
    with pytest.raises(ValueError, match="etaminus"):
        optim.FusedRprop(ps, etas=(1.5, 1.2))
    with pytest.raises(ValueError, match="step_min <= step_max"):
        optim.FusedRprop(ps, step_sizes=(1.0, 0.5))
    assert optim.FusedAdadelta(ps, rho=0.0).param_groups[0]["rho"] == 0.0                  # the reference's default is legal


@pytest.mark.parametrize("rule", CLASS_RULES)
def test_state_dict_round_trip_with_torch_optim(rule):
    """torch steps three times; the fused class loads its checkpoint; torch loads what the fused class saves and goes on
    exactly as the original does."""
    k, h = OC.kind(rule), OC.hyper(rule, 1e-4)
    ps = _params()
    ref = getattr(torch.optim, k)(ps, foreach=False, **h)
    for n in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (n + 1)) * (-1) ** n
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    fused = FUSED[k](ps)
    fused.load_state_dict(sd)
    assert int(fused.step_t) == 3 and float(fused.lr_t) == np.float32(h["lr"])
    assert all(fused.param_groups[0][key] == v for key, v in ref.param_groups[0].items() if key != "params")
    for p in ps:
        for key in OC.keys(rule):
            assert torch.equal(fused.state[p][key], ref.state[p][key]), key
    if k == "ASGD":
        assert fused.scalars[2:].tolist() == [float(ref.state[ps[0]]["eta"]), float(ref.state[ps[0]]["mu"])]   # pair 3 & 1
    out = fused.state_dict()
    extra = {"eta", "mu"} if k == "ASGD" else set()
    assert set(out["state"][0]) == set(OC.keys(rule)) | {"step"} | extra and float(out["state"][0]["step"]) == 3.0
    assert "iht_support" in out                                            # (the extra key torch ignores)
    if k == "ASGD":
        assert float(out["state"][2]["eta"]) == float(ref.state[ps[2]]["eta"])
        assert float(out["state"][2]["mu"]) == float(ref.state[ps[2]]["mu"])
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = getattr(torch.optim, k)(ps2, foreach=False)
    back.load_state_dict(out)
    for p, q in zip(ps, ps2):
        p.grad = torch.full_like(p, -0.3)
        q.grad = torch.full_like(q, -0.3)
    ref.step()
    back.step()
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
        for key in OC.keys(rule):
            assert torch.equal(ref.state[p][key], back.state[q][key]), key
    # a checkpoint whose parameters disagree about the step count has no single device counter
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="one step count"):
        FUSED[k](ps).load_state_dict(sd)
    # what the class cannot run is refused at load time too
    sd = copy.deepcopy(ref.state_dict())
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        FUSED[k](ps).load_state_dict(sd)


def test_a_fresh_checkpoint_and_the_masks():
    from kws_amd import FastGRNNCUDA
    layer = FastGRNNCUDA(8, 16, wSparsity=0.3, uSparsity=0.5, device=torch.device("cpu"))
    ps = list(layer.parameters())
    fused = optim.FusedRMSprop(ps, momentum=0.9)
    assert fused.register_iht(layer) == 2
    fused.load_state_dict(torch.optim.RMSprop(ps, momentum=0.9).state_dict())
    assert int(fused.step_t) == 0 and not fused.state                      # no state yet: the next step is the first
    fused.support(layer.W).view(-1)[::3] = 0
    again = optim.FusedRMSprop(ps, momentum=0.9)
    again.register_iht(layer)
    again.load_state_dict(fused.state_dict())
    assert torch.equal(again.support(layer.W), fused.support(layer.W)) and int(again.support(layer.W).sum()) < layer.W.numel()
    for p in ps:
        p.grad = torch.ones_like(p)
    segs, _ = again._segments()
    assert segs[0].iht == 1 and segs[0].support == again.support(layer.W).data_ptr()
    assert segs[0].keep_rank == optim.keep_rank(layer.W.numel(), 0.3) and segs[2].iht == 0
    assert segs[0].state[1] == again.state[layer.W]["momentum_buffer"].data_ptr() and segs[0].state[2] is None


# ---- configure_optimizer ---------------------------------------------------------------------------------------------
def reference_options(name, lr=1e-2):
    """TrainingOptions / OptimizerOptions with the reference's defaults (trainingConfig.py:43-58, 61-64)"""
    oo = types.SimpleNamespace(weight_decay=1e-5, momentum=0.9, centered=False, alpha=0, eps=1e-8, rho=0, lr_decay=0,
                               betas=(0.9, 0.999), lambd=0.0001, t0=1000000.0, etas=(0.5, 1.2), dampening=0,
                               step_sizes=(1e-06, 50), nesterov=True)
    return types.SimpleNamespace(optimizer=name, learning_rate=lr, optimizer_options=oo)


WANT = {
    "Adadelta": (optim.FusedAdadelta, dict(lr=1e-2, weight_decay=1e-5, rho=0, eps=1e-8)),
    "Adagrad": (optim.FusedAdagrad, dict(lr=1e-2, weight_decay=1e-5, lr_decay=0, eps=1e-10)),
    "Adam": (optim.FusedAdam, dict(lr=1e-2, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8)),
    "Adamax": (optim.FusedAdamax, dict(lr=1e-2, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8)),
    "ASGD": (optim.FusedASGD, dict(lr=1e-2, weight_decay=1e-5, lambd=1e-4, alpha=0, t0=1e6)),
    "RMSprop": (optim.FusedRMSprop, dict(lr=1e-2, weight_decay=1e-5, eps=1e-8, alpha=0, momentum=0.9, centered=False)),
    "Rprop": (optim.FusedRprop, dict(lr=1e-2, etas=(0.5, 1.2), step_sizes=(1e-6, 50))),
    "SGD": (optim.FusedSGD, dict(lr=1e-2, weight_decay=1e-5, momentum=0.9, dampening=0, nesterov=True)),
}


@pytest.mark.parametrize("name", sorted(WANT))
def test_configure_optimizer_maps_the_references_eight_names(name):
    import kws_amd
    cls, want = WANT[name]
    opt = kws_amd.configure_optimizer(_params(), reference_options(name))
    assert type(opt) is cls and isinstance(opt, optim._FusedOptimizer)
    g = opt.param_groups[0]
    assert {k: g[k] for k in want} == want and g["capturable"] is False
    assert kws_amd.configure_optimizer(_params(), reference_options(name), capturable=True).param_groups[0]["capturable"] is True


def test_configure_optimizer_names_what_it_does_not_know():
    with pytest.raises(ValueError, match="SparseAdam"):
        optim.configure_optimizer(_params(), reference_options("SparseAdam"))


def test_train_step_takes_the_new_classes_and_still_names_what_it_needs():
    from kws_amd import RNNClassifierModel, TrainSchedule
    model = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=12, device=torch.device("cpu"))
    x, y = torch.zeros(3, 2, 32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="FusedAdam"):
        model.train_step(x, y, torch.optim.RMSprop(model.parameters()))
    opt = optim.FusedRMSprop(model.parameters(), capturable=True)
    assert TrainSchedule(opt, 64, 8, 3, seed=1).optimizer is opt                   # (the isinstance test lets every fused class in)


# ---- the static scans of kernels_update.hip, all eight rules, are tests/test_update_cpu.py's -------------------------
def test_the_radix_select_exists_once():
    """kernels_update.hip holds the one radix select, and the one kernel template calls it once"""
    csrc = os.path.join(ROOT, "kws_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and "atomicAdd(&hist[" in open(os.path.join(csrc, f)).read()]
    assert holders == ["kernels_update.hip"]
    text = open(os.path.join(csrc, "kernels_update.hip")).read()
    assert text.count("atomicAdd(&hist[") == 1 and text.count("__global__") == 1
    assert text.count("iht_threshold(") == 2                                   # the definition and the kernel's one call
