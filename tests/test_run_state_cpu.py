"""What a graph capture's warm-up has to put back, without a GPU: kws_amd.graph.RunSnapshot over the owners' own lists
(the model, the fused optimizers, TrainSchedule, RollingBags).  The warm-up is simulated: no step runs, every tensor an
owner lists, and every state tensor a first step would have created, is overwritten with a marker.
"""
import pytest
import torch

from kws_amd import RNNClassifierModel, RollingBags, RunSnapshot, TrainSchedule, optim
from tests import optim_cases as OC
from tests import update_cases as U

MARK, OLD = 7.0, 3.0
# the eight rules: (class, constructor arguments, what each state tensor is created with)
RULES = {
    "adam": (optim.FusedAdam, dict(U.ADAM), {"exp_avg": 0.0, "exp_avg_sq": 0.0}),
    "sgd": (optim.FusedSGD, dict(U.SGD), {"momentum_buffer": 0.0}),
    "rmsprop": (optim.FusedRMSprop, OC.hyper("rmsprop_centered_mom", 0.0),
                {"square_avg": 0.0, "momentum_buffer": 0.0, "grad_avg": 0.0}),
    "adagrad": (optim.FusedAdagrad, dict(OC.hyper("adagrad_decay", 0.0), initial_accumulator_value=0.5), {"sum": 0.5}),
    "adadelta": (optim.FusedAdadelta, OC.hyper("adadelta", 0.0), {"square_avg": 0.0, "acc_delta": 0.0}),
    "adamax": (optim.FusedAdamax, OC.hyper("adamax", 0.0), {"exp_avg": 0.0, "exp_inf": 0.0}),
    "asgd": (optim.FusedASGD, OC.hyper("asgd_avg", 0.0), {"ax": 0.0}),
    "rprop": (optim.FusedRprop, OC.hyper("rprop", 0.0), {"prev": 0.0, "step_size": OC.RULES["rprop"][1]["lr"]}),
}


def cpu_model(layers=1):
    torch.manual_seed(2)
    return RNNClassifierModel("FastGRNNCUDA", 32, layers, [128] * layers, [None] * layers, [None] * layers, [0.5] * layers,
                              [0.5] * layers, "sigmoid", "tanh", num_classes=12, device=torch.device("cpu"))


def trainer(rule):
    cls, h, created = RULES[rule]
    model = cpu_model()
    opt = cls(model.parameters(), capturable=True, **h)
    assert opt.register_iht(model) == 2
    return model, opt, created


def simulated_warmup(model, opt):
    """what three steps leave behind, as far as an undo can tell: state exists, everything listed has been written"""
    params = opt.param_groups[0]["params"]
    for p in params:
        opt._init_state(p)
    with torch.no_grad():
        for t in model.run_tensors() + opt.run_tensors() + [t for p in params for t in opt.state[p].values()]:
            t.fill_(MARK)
    model.hidden_states = [torch.full((8, 128), MARK)]


def filled(t, value):
    return bool((t == torch.tensor(value, dtype=t.dtype)).all())


@pytest.mark.parametrize("rule", sorted(RULES))
def test_restore_recreates_the_state_a_warmup_created(rule):
    model, opt, created = trainer(rule)
    start = [p.detach().clone() for p in model.parameters()]
    scalars = opt.scalars.clone() if rule == "asgd" else None
    keep = RunSnapshot([model, opt])
    simulated_warmup(model, opt)
    keep.restore()
    group = opt.param_groups[0]
    for p, p0 in zip(model.parameters(), start):
        assert torch.equal(p, p0)
        assert set(created) <= set(opt.state[p])
        for key, value in created.items():
            assert filled(opt.state[p][key], value), (key, value, opt.state[p][key].flatten()[:3])
            assert torch.equal(opt.state[p][key], opt._new_state(p, key, group)), key
    assert int(opt.step_t) == 0
    for rnn in model.rnn_list:
        assert filled(opt.support(rnn.W), 1) and filled(opt.support(rnn.U), 1)
    if rule == "asgd":
        assert torch.equal(opt.scalars, scalars) and not filled(opt.scalars, MARK)
    assert model.hidden_states == [None]


@pytest.mark.parametrize("rule", sorted(RULES))
def test_restore_puts_back_state_that_existed_before(rule):
    model, opt, created = trainer(rule)
    for p in model.parameters():
        for key in opt._init_state(p):
            opt.state[p][key].fill_(OLD)
    opt.step_t.fill_(5)
    keep = RunSnapshot([model, opt])
    simulated_warmup(model, opt)
    keep.restore()
    for p in model.parameters():
        for key in created:
            assert filled(opt.state[p][key], OLD), key
    assert int(opt.step_t) == 5


def test_what_the_owners_list():
    model = cpu_model(2)
    opt = optim.FusedASGD(model.parameters(), capturable=True)
    opt.register_iht(model)
    listed = {id(t) for t in opt.run_tensors()}
    assert id(opt.lr_t) not in listed and id(opt.iht_t) not in listed
    assert {id(opt.step_t), id(opt.scalars)} <= listed and len(listed) == 2 + 4       # no state yet; four masks
    sched = TrainSchedule(opt, 50, 8, 4, seed=1, rolling=True, max_rolling_length=2, bag_count=3)
    assert [id(t) for t in sched.run_tensors()] == [id(sched.loss_log), id(sched.lr_log)]
    bags = RollingBags(model, sched)
    assert len(bags.run_tensors()) == 6 and [id(t) for t in bags.run_tensors()] == [id(t) for t in bags.tensors()]
    guarded = optim.FusedAdam(model.parameters(), capturable=True).guard(1.0)
    g_sched = TrainSchedule(guarded, 50, 8, 4, seed=1)
    assert [id(t) for t in g_sched.run_tensors()] == [id(g_sched.loss_log), id(g_sched.lr_log), id(g_sched.norm_log),
                                                      id(g_sched.skip_log)]
    assert {id(p) for p in model.parameters()} | {id(b) for b in model.buffers()} == {id(t) for t in model.run_tensors()}


def test_a_snapshot_of_nothing_and_an_owner_without_run_reset():
    class Owner:
        def __init__(self):
            self.t = torch.arange(4.0)

        def run_tensors(self):
            return [self.t]

    o = Owner()
    keep = RunSnapshot([o])
    o.t.fill_(MARK)
    keep.restore()
    assert o.t.tolist() == [0.0, 1.0, 2.0, 3.0]
    RunSnapshot([]).restore()
