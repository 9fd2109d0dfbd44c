"""CPU-side checks of the fused optimizer step (fastgrnn_hip_train_update, kws_amd/optim.py): the fp64 oracles the GPU
tests compare against, held to torch.optim in fp64; the threshold rule against numpy's percentile on typed-out cases;
iht_phase against the trainer's branch; the entry point's argument checks without a launch (as tests/test_abi_cpu.py
does for the others); optimizer construction and checkpoints on CPU tensors; and the static scans of the kernel source,
kernels_update.hip, over the kernels of all eight rules (the other scanner tests list their sources by name)."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import _lib, optim
from tests import update_cases as U
from tests import support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_update.hip")
NULL, ONE = None, 256                                   # (a fake non-NULL pointer: nothing is launched)
OK, NULLP, SHAPE, UNSUP = 0, 1, 2, 7


@pytest.fixture(scope="module")
def lib():
    return S.built_library()


# ---- the oracles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", U.WDS)
@pytest.mark.parametrize("t", (1, 2, 1000))
def test_adam_oracle_is_torch_adam_in_fp64(t, wd):
    p, g, m, v, b = U.segment(1025, t, seed=3)
    h = U.hyper("adam", wd)
    for _ in range(2):                                  # two consecutive steps: the outputs of one feed the next
        ref = U.torch_cpu_step("adam", wd, t, p, g, m, v, b, dtype=torch.float64)
        p1, m1, v1, *_ = U.adam_oracle(p, g, m, v, h["lr"], h["betas"], h["eps"], wd, t)
        for got, want in ((p1, ref["p"]), (m1, ref["m"]), (v1, ref["v"])):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        p, m, v, t = p1, m1, v1, t + 1


@pytest.mark.parametrize("wd", U.WDS)
@pytest.mark.parametrize("dampening", (0.0, 0.1))
@pytest.mark.parametrize("nesterov", (False, True))
def test_sgd_oracle_is_torch_sgd_in_fp64(nesterov, dampening, wd):
    if nesterov and dampening:
        with pytest.raises(ValueError):                 # torch's own rule, which the library repeats
            torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9, dampening=dampening, nesterov=True)
        return
    p, g, _, _, _ = U.segment(1025, 1, seed=4)
    g2 = U.segment(1025, 2, seed=5)[1]
    q = torch.nn.Parameter(torch.from_numpy(np.array(p)).double())
    opt = torch.optim.SGD([q], lr=0.05, momentum=0.9, dampening=dampening, weight_decay=wd, nesterov=nesterov,
                          foreach=False)
    p64, b64 = np.asarray(p, dtype=np.float64), np.zeros(1025)
    for t, grad in ((1, g), (2, g2)):                   # step 1: the buffer is the gradient, undamped
        q.grad = torch.from_numpy(np.array(grad)).double()
        opt.step()
        p64, b64, *_ = U.sgd_oracle(p64, grad, b64, 0.05, 0.9, dampening, wd, nesterov, t)
        np.testing.assert_allclose(p64, q.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(b64, opt.state[q]["momentum_buffer"].numpy(), rtol=1e-12, atol=0)
    if dampening:
        first = U.sgd_oracle(p, g, np.zeros(1025), 0.05, 0.9, dampening, wd, nesterov, 1)[1]
        np.testing.assert_array_equal(first, np.asarray(g, np.float64) + wd * np.asarray(p, np.float64))


@pytest.mark.parametrize("algo", U.ALGOS)
@pytest.mark.parametrize("t", U.STEPS)
@pytest.mark.parametrize("wd", U.WDS)
def test_torch_fp32_meets_the_bound_on_the_gpu_tests_operands(algo, t, wd):
    """The bound is not tighter than a faithful fp32 implementation needs: torch's own fp32 step, on the operands of
    tests/test_hip_update.py, stays inside it (with room: 8u against the 4.8u / 3.4u measured)."""
    for n in U.SIZES:
        ops = U.segment(n, t, seed=1)
        w = U.worst(U.torch_cpu_step(algo, wd, t, *ops), U.oracle(algo, wd, t, *ops))
        assert max(w.values()) <= 1.0, (n, w)


# ---- the threshold rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.THRESHOLD_CASES, ids=[c[0] for c in U.THRESHOLD_CASES])
def test_threshold_rule_on_typed_out_cases(case):
    _, vals, s, rank, th, result = case
    a = np.array(vals, dtype=np.float32)
    assert U.keep_rank_oracle(a.size, s) == rank == optim.keep_rank(a.size, s)
    got_th, got = U.threshold_oracle(a, s)
    assert got_th == np.float32(th) == np.percentile(np.abs(a), (1.0 - s) * 100.0, method="higher")
    np.testing.assert_array_equal(got, np.array(result, dtype=np.float32))
    from kws_amd import utils
    np.testing.assert_array_equal(utils.hardThreshold(torch.from_numpy(a.copy()), s).numpy(), got)


@pytest.mark.parametrize("n", U.SIZES + (5, 37))
@pytest.mark.parametrize("s", U.SPARSITIES)
def test_keep_rank_is_numpys_higher_index(n, s):
    a = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    k = optim.keep_rank(n, s)
    assert 0 <= k <= n - 1 and k == U.keep_rank_oracle(n, s)
    assert np.sort(np.abs(a))[k] == np.percentile(np.abs(a), (1.0 - s) * 100.0, method="higher")


def test_adversarial_sets_are_what_they_say():
    for name in U.ADVERSARIAL:
        t = U.adversarial(name, 3079)
        mag = t.view(np.uint32) & np.uint32(0x7FFFFFFF)
        assert np.isfinite(t).all()
        if name == "all_equal":
            assert len(set(mag.tolist())) == 1
        elif name == "two_values":
            assert len(set(mag.tolist())) == 2
        elif name.startswith("byte"):
            k = int(name[4])
            differ = np.bitwise_or.reduce(mag ^ mag[0])
            assert differ & ~np.uint32(0xFF << (8 * k)) == 0 and len(set(mag.tolist())) > 100
        else:
            assert (mag == 0).sum() == 3079 // 2 and (t.view(np.uint32) == 0x80000000).any() and (t.view(np.uint32) == 0).any()
        assert (t < 0).any() and (t > 0).any()
        p, g = U.adversarial_operands(t)
        np.testing.assert_array_equal((p - np.float32(1.0) * g).view(np.uint32) & np.uint32(0x7FFFFFFF), mag)


# ---- iht_phase ---------------------------------------------------------------------------------------------------------
def test_iht_phase_is_the_trainers_branch():
    seen = set()
    for epoch in range(9):
        for i_batch in range(7):
            want = U.iht_phase_reference(True, epoch, 9, i_batch, 3)
            assert optim.iht_phase(epoch, 9, i_batch, 3) == want, (epoch, i_batch)
            seen.add(want)
    assert seen == {"none", "threshold", "support"}
    assert optim.iht_phase(2, 9, 0, 3) == "none" and optim.iht_phase(3, 9, 0, 3) == "threshold"
    assert optim.iht_phase(5, 9, 1, 3) == "support" and optim.iht_phase(6, 9, 0, 3) == "support"
    assert [optim.iht_phase(e, 10, 0, 3) for e in (3, 4, 6, 7)] == ["none", "threshold", "threshold", "support"]


# ---- argument checks of the entry point, no launch ---------------------------------------------------------------------
def _seg(**kw):
    d = dict(param=ONE, grad=ONE, state0=ONE, state1=ONE, support=NULL, n=100, keep_rank=0, iht=0, reserved=0)
    d.update(kw)
    return _lib.UpdateSeg(**d)


def _hyper(algo=_lib.ADAM, nesterov=0, a=0.9, b=0.999, eps=1e-8, wd=0.0):
    return _lib.UpdateHyper(algo, nesterov, a, b, eps, wd)


def _update(lib, segs=None, h=None, n_segs=None, lr=ONE, step=ONE, mode=ONE, no_h=False, no_segs=False):
    segs = [_seg()] if segs is None else segs
    arr = (_lib.UpdateSeg * len(segs))(*segs)
    h = _hyper() if h is None else h
    return lib.fastgrnn_hip_train_update(None if no_h else C.byref(h), None if no_segs else arr,
                                         len(segs) if n_segs is None else n_segs, lr, step, mode, None)


def test_symbol_exists_and_the_abi_version_stays(lib):
    assert hasattr(lib, "fastgrnn_hip_train_update") and "fastgrnn_hip_train_update" in _lib.EXPORTS
    assert lib.fastgrnn_hip_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    assert "fastgrnn_hip_train_update(" in header and "#define FASTGRNN_UPDATE_MAX_SEGS 32" in header
    assert C.sizeof(_lib.UpdateSeg) == 64 and C.sizeof(_lib.UpdateHyper) == 40


def test_null_pointers(lib):
    assert _update(lib, no_h=True) == NULLP
    assert _update(lib, no_segs=True) == NULLP
    assert _update(lib, lr=NULL) == NULLP
    assert _update(lib, step=NULL) == NULLP
    for name in ("param", "grad", "state0", "state1"):
        assert _update(lib, [_seg(**{name: NULL})]) == NULLP, name
    assert _update(lib, [_seg(), _seg(), _seg(grad=NULL)]) == NULLP            # every segment is looked at
    assert _update(lib, [_seg(iht=1, support=NULL)]) == NULLP
    assert _update(lib, [_seg(iht=1, support=ONE)], mode=NULL) == NULLP         # an IHT segment needs the mode scalar
    # SGD has no second moment: state1 may be NULL (the next refusal in line shows the pointer checks passed)
    sgd = _hyper(_lib.SGD, 0, 0.9, 0.0)
    assert _update(lib, [_seg(state1=NULL, n=0)], sgd) == SHAPE
    assert _update(lib, [_seg(state0=NULL)], sgd) == NULLP
    # iht_mode may be NULL when no segment takes part; support is not required then
    assert _update(lib, [_seg(n=0)], mode=NULL) == SHAPE


def test_bad_shapes(lib):
    assert _update(lib, n_segs=0) == SHAPE
    assert _update(lib, n_segs=-1) == SHAPE
    for n in (0, -5, (1 << 22) + 1):
        assert _update(lib, [_seg(n=n)]) == SHAPE, n
    assert _update(lib, [_seg(n=10, keep_rank=10)]) == SHAPE
    assert _update(lib, [_seg(n=10, keep_rank=-1)]) == SHAPE
    for h in (_hyper(a=1.0), _hyper(a=-0.1), _hyper(b=1.0), _hyper(b=-0.5), _hyper(eps=0.0), _hyper(eps=-1e-8),
              _hyper(wd=-1e-5), _hyper(a=float("nan")), _hyper(_lib.SGD, 0, 1.0, 0.0), _hyper(_lib.SGD, 0, -0.1, 0.0),
              _hyper(_lib.SGD, 0, 0.9, 0.0, wd=-1.0),
              _hyper(_lib.SGD, 1, 0.0, 0.0),                  # nesterov without momentum
              _hyper(_lib.SGD, 1, 0.9, 0.1)):                 # nesterov with dampening
        assert _update(lib, h=h) == SHAPE, (h.algo, h.nesterov, h.beta1_or_momentum, h.beta2_or_dampening, h.eps)
    # SGD ignores eps; dampening may be anything finite
    assert _update(lib, [_seg(n=0)], _hyper(_lib.SGD, 0, 0.9, 0.1, eps=0.0)) == SHAPE       # (the segment's n, not eps ...
    assert _update(lib, [_seg(param=NULL)], _hyper(_lib.SGD, 0, 0.9, 0.1, eps=0.0)) == NULLP  # ... as this shows)


def test_unknown_algo(lib):
    for algo in (2, -1, 7):
        assert _update(lib, h=_hyper(algo)) == UNSUP


# ---- the optimizers on CPU tensors: construction, limits, checkpoints ------------------------------------------------
def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(5, 7, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g)),
            torch.nn.Parameter(torch.randn(1, 1, generator=g))]


def test_construction_needs_no_gpu_and_step_does():
    ps = _params()
    opt = optim.FusedAdam(ps, lr=0.01, weight_decay=1e-5)
    assert set(torch.optim.Adam(_params()).param_groups[0]) == set(opt.param_groups[0])
    assert set(torch.optim.SGD(_params(), lr=0.1).param_groups[0]) <= set(optim.FusedSGD(ps, lr=0.1).param_groups[0])
    assert opt.lr_t.dtype == torch.float32 and opt.step_t.dtype == torch.int64 and opt.iht_t.dtype == torch.int32
    assert float(opt.lr_t) == np.float32(0.01) and int(opt.step_t) == 0 and int(opt.iht_t) == 0
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()


def test_limits_are_named():
    ps = _params()
    with pytest.raises(ValueError, match="one param group"):
        optim.FusedAdam([{"params": ps[:1]}, {"params": ps[1:]}])
    with pytest.raises(ValueError, match="float32"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="float32"):
        optim.FusedSGD([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))], lr=0.1)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.FusedAdam(ps, amsgrad=True)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        optim.FusedAdam(ps, decoupled_weight_decay=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.FusedSGD(ps, lr=0.1, maximize=True)
    with pytest.raises(ValueError, match="Nesterov"):
        optim.FusedSGD(ps, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="betas"):
        optim.FusedAdam(ps, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="contiguous"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])


def test_register_iht_marks_the_layers_matrices():
    from kws_amd import FastGRNNCUDA, RNNClassifierModel
    cpu = torch.device("cpu")
    fact = FastGRNNCUDA(32, 256, wRank=16, uRank=16, wSparsity=0.3, uSparsity=0.5, device=cpu)
    opt = optim.FusedAdam(fact.parameters())
    assert opt.register_iht(fact) == 4
    assert opt.support(fact.W1).shape == fact.W1.shape and opt.support(fact.U2).dtype == torch.uint8
    assert bool(opt.support(fact.W2).all())
    assert opt._iht[fact.W1][0] == optim.keep_rank(fact.W1.numel(), 0.3)
    assert opt._iht[fact.U2][0] == optim.keep_rank(fact.U2.numel(), 0.5)
    model = RNNClassifierModel("FastGRNNCUDA", 32, 2, [256, 128], [None, None], [None, None], [0.3, 0.5], [0.2, 1.0],
                               "sigmoid", "tanh", num_classes=12, device=cpu)
    opt = optim.FusedSGD(model.parameters(), lr=0.1, momentum=0.9)
    assert opt.register_iht(model) == 4
    assert opt._iht[model.rnn_list[1].U][0] == 0                          # sparsity 1.0: everything survives
    with pytest.raises(KeyError):
        opt.support(model.hidden2keyword.weight)
    bn = RNNClassifierModel("FastGRNNBatchNormCUDA", 64, 3, [256, 128, 128], [None] * 3, [None] * 3, [0.3] * 3, [0.5] * 3,
                            "sigmoid", "tanh", num_classes=12, device=cpu)
    opt = optim.FusedAdam(bn.parameters())
    assert opt.register_iht(bn) == 6 and len(opt.param_groups[0]["params"]) > _lib.UPDATE_MAX_SEGS   # (two launches)
    assert opt._iht[bn.rnn_list[2].cell.U][0] == optim.keep_rank(128 * 128, 0.5)
    with pytest.raises(ValueError, match="not a parameter"):
        optim.FusedAdam(model.hidden2keyword.parameters()).register_iht(model)


def test_state_dict_round_trip_with_torch_adam():
    ps = _params()
    ref = torch.optim.Adam(ps, lr=0.02, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-4, foreach=False)
    for k in range(3):
        for p in ps:
            p.grad = torch.full_like(p, 0.1 * (k + 1))
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    fused = optim.FusedAdam(ps)
    fused.load_state_dict(sd)
    assert int(fused.step_t) == 3 and float(fused.lr_t) == np.float32(0.02)
    g = fused.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (0.02, (0.8, 0.99), 1e-6, 1e-4)
    for p in ps:
        assert torch.equal(fused.state[p]["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(fused.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    # ... and back: torch.optim.Adam loads what FusedAdam saves, and goes on exactly as the original does
    out = fused.state_dict()
    assert set(out["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(out["state"][0]["step"]) == 3.0
    assert "iht_support" in out                                            # (the extra key torch ignores)
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch.optim.Adam(ps2, foreach=False)
    back.load_state_dict(out)
    for p, q in zip(ps, ps2):
        p.grad = torch.full_like(p, -0.3)
        q.grad = torch.full_like(q, -0.3)
    ref.step()
    back.step()
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
    # a checkpoint whose parameters disagree about the step count has no single device counter
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="one step count"):
        optim.FusedAdam(ps).load_state_dict(sd)
    # what FusedAdam cannot run is refused at load time too
    sd = copy.deepcopy(ref.state_dict())
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        optim.FusedAdam(ps).load_state_dict(sd)


def test_state_dict_round_trip_with_torch_sgd_and_the_masks():
    from kws_amd import FastGRNNCUDA
    layer = FastGRNNCUDA(8, 16, wSparsity=0.3, uSparsity=0.5, device=torch.device("cpu"))
    ps = list(layer.parameters())
    ref = torch.optim.SGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-5, foreach=False)
    for p in ps:
        p.grad = torch.full_like(p, 0.25)
    ref.step()
    fused = optim.FusedSGD(ps, lr=0.1)
    fused.register_iht(layer)
    fused.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert int(fused.step_t) == 1                                          # a buffer: the first step is behind us
    assert fused.param_groups[0]["momentum"] == 0.9 and float(fused.lr_t) == np.float32(0.05)
    assert all(torch.equal(fused.state[p]["momentum_buffer"], ref.state[p]["momentum_buffer"]) for p in ps)
    fused.support(layer.W).view(-1)[::3] = 0
    out = fused.state_dict()
    again = optim.FusedSGD(ps, lr=0.1)
    again.register_iht(layer)
    again.load_state_dict(out)
    assert torch.equal(again.support(layer.W), fused.support(layer.W)) and int(again.support(layer.W).sum()) < layer.W.numel()
    assert int(again.step_t) == 1
    back = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.1)
    back.load_state_dict(out)                                              # torch ignores the extra keys
    assert back.param_groups[0]["momentum"] == 0.9
    fresh = optim.FusedSGD(ps, lr=0.1, momentum=0.9)
    fresh.load_state_dict(torch.optim.SGD(ps, lr=0.1, momentum=0.9).state_dict())
    assert int(fresh.step_t) == 0                                          # no buffer yet: the next step is the first


# ---- static scans of the kernel source, all eight rules --------------------------------------------------------------
@pytest.fixture(scope="module")
def update_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_update.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(update_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), update_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(update_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), update_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_the_kernel_uses_no_scratch_and_one_workgroup_of_1024():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = resource_usage.usage(SRC)
    assert sorted(r["pretty"] for r in rows) == ["void update_k<%d>" % a for a in range(8)]   # one kernel per rule
    for r in rows:
        assert r["scratch"] == 0 and r["lds"] <= 2048 and r["vgpr"] <= 64, r               # (1024 threads: 16 waves, 128 VGPRs at most)


# ---- the segment table and the one-group limit, on CPU tensors (no launch) -------------------------------------------
def test_segment_table_follows_what_it_points_at():
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = optim.FusedAdam(ps)
    segs, n = opt._segments()
    assert n == 3 and opt._segments()[0] is segs                              # nothing moved: the same table
    assert segs[0].state0 == opt.state[ps[0]]["exp_avg"].data_ptr() and segs[0].state1 == opt.state[ps[0]]["exp_avg_sq"].data_ptr()
    opt.state[ps[0]]["exp_avg"] = torch.zeros_like(ps[0])                      # replaced behind the optimizer's back
    segs2, _ = opt._segments()
    assert segs2 is not segs and segs2[0].state0 == opt.state[ps[0]]["exp_avg"].data_ptr()
    ps[1].grad = torch.ones_like(ps[1])                                        # a new gradient tensor
    segs3, _ = opt._segments()
    assert segs3[1].grad == ps[1].grad.data_ptr()
    ps[2].grad = None
    assert opt._segments()[1] == 2                                             # parameters without a gradient are skipped
    ps[0].grad = torch.ones(7, 5).t()                                          # checked on every call, hit or not
    with pytest.raises(RuntimeError, match="contiguous"):
        opt._segments()


def test_a_replaced_mask_and_a_second_group_are_noticed():
    from kws_amd import FastGRNNCUDA
    layer = FastGRNNCUDA(8, 16, wSparsity=0.3, uSparsity=0.5, device=torch.device("cpu"))
    for p in layer.parameters():
        p.grad = torch.ones_like(p)
    opt = optim.FusedSGD(layer.parameters(), lr=0.1, momentum=0.9)
    opt.register_iht(layer)
    segs, _ = opt._segments()
    assert segs[0].iht == 1 and segs[0].support == opt.support(layer.W).data_ptr()
    assert segs[0].keep_rank == optim.keep_rank(layer.W.numel(), 0.3) and segs[2].iht == 0
    opt.register_iht(layer)                                                    # new masks
    assert opt._segments()[0][0].support == opt.support(layer.W).data_ptr()
    with pytest.raises(ValueError, match="one param group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})


def test_train_step_names_the_optimizer_it_needs():
    from kws_amd import RNNClassifierModel
    model = RNNClassifierModel("FastGRNNCUDA", 32, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=12, device=torch.device("cpu"))
    with pytest.raises(TypeError, match="FusedAdam"):
        model.train_step(torch.zeros(3, 2, 32), torch.zeros(2, dtype=torch.int64), torch.optim.Adam(model.parameters()))
