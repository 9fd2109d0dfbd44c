#!/usr/bin/env python3
"""What the last two lines of a trainer iteration cost -- optimizer.step() and the IHT phase (trainClassifier.py:249-259)
-- with the fused call (kws_amd.FusedAdam on fastgrnn_hip_train_update) and with the torch chain it replaces
(torch.optim.Adam(foreach=True) + model.sparsify() / model.sparsifyWithSupport()).

    python tools/update_bench.py [--iters 15] [--run 200] [--step-run 20] [--warmup 3] [--batches 128,4096] [--steps 99]

Two parts, the routes of each alternating inside every repeat:

  update   the two lines alone, on fixed gradients, for two parameter lists: the default model (dense 64 -> 256 -> 128
           + a 12-class head: 14 tensors) and the 3-layer BatchNorm model (64 -> 256 -> 128 -> 128: 44 tensors, i.e.
           two launches of 32 and 12 segments).  fused none / threshold / support; torch Adam alone; torch Adam +
           sparsify(); torch Adam + sparsifyWithSupport().  Eager, and replayed from a captured graph where the route
           captures (the fused ones with capturable=True, torch's Adam with capturable=True and a tensor lr).
  step     the whole iteration of the default model at T = --steps for every batch size: forward + backward alone,
           model.train_step with the fused optimizer in each IHT phase, and the same iteration with the torch chain;
           eager and graph-replayed.  "share" is the part of the iteration that the two lines take:
           (iteration - forward/backward alone) / iteration, with the forward/backward timed on the route's own model
           instance (instances differ by more than the two lines cost).

Every route is checked before and after it is timed: the W/U matrices must be dense after plain steps and hold the
models' sparsity after a threshold or support phase, else the run ends with an error instead of a number.

A sample is a host clock around --run (--step-run) consecutive calls that end in a device synchronise, per call: what a
training loop pays per iteration, whichever of host and device is the slower.  Medians over --iters samples with the
10th / 90th percentiles as the spread; "device_median_us" is the same window between two device events (it leaves out the
host's lead-in and the final synchronise).  Prints one JSON line; fails without a GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def stats(ts):
    return {"median_us": round(pct(ts, 0.5), 2), "p10_us": round(pct(ts, 0.1), 2), "p90_us": round(pct(ts, 0.9), 2),
            "n": len(ts)}


def sample_us(fn, run):
    """-> (host clock, device events) around `run` calls, each per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(run):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / run, e0.elapsed_time(e1) * 1e3 / run


def interleaved(routes, iters, run):
    ts = {k: ([], []) for k in routes}
    for _ in range(iters):
        for k, fn in routes.items():
            host, device = sample_us(fn, run)
            ts[k][0].append(host)
            ts[k][1].append(device)
    return ts


def measure(routes, checks, a, run):
    """routes: name -> fn; checks: name -> (model, phase, describe()).  Every route is verified after the warm-up and again
    after the timed calls (verify): a route that does not do what it names ends the run."""
    interleaved(routes, a.warmup, 2)
    for k, (model, phase, describe) in checks.items():
        if k in routes:
            verify(k, model, phase, " after the warm-up" + describe())
    ts = interleaved(routes, a.iters, run)
    kept = {k: verify(k, model, phase, " after the timed calls" + describe())
            for k, (model, phase, describe) in checks.items() if k in routes}
    return ({k: dict(stats(h), device_median_us=round(pct(d, 0.5), 2)) for k, (h, d) in ts.items()}, kept)


def fused_state(o):
    return lambda: " (iht_t %d, step_t %d)" % (int(o.iht_t), int(o.step_t))


def try_graph(name, fn, routes, notes):
    """add a graph-replayed twin of `fn` to `routes` if it captures"""
    from kws_amd import GraphedStep
    try:
        routes[name + "_graph"] = GraphedStep(fn)
    except Exception as e:                                  # a route that does not capture is reported, not timed
        notes[name + "_graph"] = "does not capture: %s" % (str(e).splitlines()[0][:160],)
        torch.cuda.synchronize()


def nonzero_fraction(model):
    mats = [p for rnn in model.rnn_list for p in getattr(rnn, "cell", rnn).getVars()[:2]]
    return sum(int((p != 0).sum()) for p in mats) / sum(p.numel() for p in mats)


SPARSITY = 0.3


def verify(name, model, phase, detail=""):
    """A route must do what its name says before its time is worth anything: after a threshold or support phase the W/U
    matrices hold the models' sparsity (a little more where magnitudes tie with the threshold: ties survive), after
    plain steps they are dense.  Anything else ends the run."""
    f = nonzero_fraction(model)
    ok = (f == 1.0) if phase == "none" else (SPARSITY - 1e-3 <= f <= SPARSITY + 0.02)
    if not ok:
        raise SystemExit("update_bench: route %s left %.4f of the W/U entries non-zero, which is not what phase %r "
                         "implies%s -- its time would not measure what it names" % (name, f, phase, detail))
    return round(f, 4)


def build(kind, dev, sparsity=SPARSITY):
    from kws_amd import RNNClassifierModel
    torch.manual_seed(0)
    if kind == "default":
        return RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None] * 2, [None] * 2, [sparsity] * 2,
                                  [sparsity] * 2, "sigmoid", "tanh", num_classes=12, device=dev)
    return RNNClassifierModel("FastGRNNBatchNormCUDA", 64, 3, [256, 128, 128], [None] * 3, [None] * 3, [sparsity] * 3,
                              [sparsity] * 3, "sigmoid", "tanh", num_classes=12, device=dev)


def update_part(kind, a, dev):
    from kws_amd import FusedAdam, optim
    hyper = dict(lr=0.01, weight_decay=1e-5)
    notes, routes, checks = {}, {}, {}
    no_state = lambda: ""

    def with_grads(model):
        for p in model.parameters():
            p.grad = 0.01 * torch.randn_like(p)
        return model

    # fused: one optimizer per mode so that iht_t is written once, outside the timed calls
    for mode in ("none", "threshold", "support"):
        m = with_grads(build(kind, dev))
        o = FusedAdam(m.parameters(), **hyper)
        o.register_iht(m)
        o.step("threshold")                                 # a support to mask with
        routes["fused_" + mode] = (lambda o=o, mode=mode: o.step(mode))
        checks["fused_" + mode] = (m, mode, fused_state(o))
        mg = with_grads(build(kind, dev))
        og = FusedAdam(mg.parameters(), capturable=True, **hyper)
        og.register_iht(mg)
        og.step("threshold")
        og.iht_t.fill_(optim.IHT_MODES[mode])
        try_graph("fused_" + mode, (lambda og=og: og.step(None)), routes, notes)
        checks["fused_" + mode + "_graph"] = (mg, mode, fused_state(og))
    n_tensors = len(list(m.parameters()))

    # torch: the chain the fused call replaces
    m0 = with_grads(build(kind, dev))
    o0 = torch.optim.Adam(m0.parameters(), foreach=True, **hyper)
    routes["torch_adam"] = o0.step
    m1 = with_grads(build(kind, dev))
    o1 = torch.optim.Adam(m1.parameters(), foreach=True, **hyper)
    routes["torch_adam_sparsify"] = (lambda: (o1.step(), m1.sparsify()))
    m2 = with_grads(build(kind, dev))
    o2 = torch.optim.Adam(m2.parameters(), foreach=True, **hyper)
    m2.sparsify()
    routes["torch_adam_support"] = (lambda: (o2.step(), m2.sparsifyWithSupport()))
    checks.update(torch_adam=(m0, "none", no_state), torch_adam_sparsify=(m1, "threshold", no_state),
                  torch_adam_support=(m2, "support", no_state))
    cap = dict(foreach=True, capturable=True, weight_decay=1e-5)
    mg0 = with_grads(build(kind, dev))
    og0 = torch.optim.Adam(mg0.parameters(), lr=torch.tensor(0.01, device=dev), **cap)
    try_graph("torch_adam", og0.step, routes, notes)
    mg2 = with_grads(build(kind, dev))
    og2 = torch.optim.Adam(mg2.parameters(), lr=torch.tensor(0.01, device=dev), **cap)
    mg2.sparsify()
    try_graph("torch_adam_support", (lambda: (og2.step(), mg2.sparsifyWithSupport())), routes, notes)
    mg1 = with_grads(build(kind, dev))
    og1 = torch.optim.Adam(mg1.parameters(), lr=torch.tensor(0.01, device=dev), **cap)
    try_graph("torch_adam_sparsify", (lambda: (og1.step(), mg1.sparsify())), routes, notes)
    checks.update(torch_adam_graph=(mg0, "none", no_state), torch_adam_sparsify_graph=(mg1, "threshold", no_state),
                  torch_adam_support_graph=(mg2, "support", no_state))
    us, kept = measure(routes, checks, a, a.run)
    return {"tensors": n_tensors, "elements": sum(p.numel() for p in m.parameters()), "us": us,
            "nonzero_fraction_of_W_U": kept, "notes": notes}


def step_part(B, a, dev):
    """Every route is paired with a forward + backward alone ON ITS OWN MODEL INSTANCE (name + ":fwd_bwd"): between
    instances of the same model the forward + backward differs by more than the two lines cost."""
    from kws_amd import FusedAdam, optim
    T, F, C = a.steps, 64, 12
    x = torch.randn(T, B, F, device=dev)
    y = torch.randint(0, C, (B,), device=dev)
    hyper = dict(lr=0.01, weight_decay=1e-5)
    notes, routes, checks = {}, {}, {}
    no_state = lambda: ""

    def fwd_bwd_of(model):
        def fwd_bwd():
            for p in model.parameters():
                p.grad = None
            model.init_hidden()
            model.loss(x, y).backward()
        return fwd_bwd

    def add(name, fn, model, phase, describe, graph):
        if graph:
            try_graph(name, fn, routes, notes)
            if name + "_graph" in routes:
                try_graph(name + ":fwd_bwd", fwd_bwd_of(model), routes, notes)     # -> name:fwd_bwd_graph
                checks[name + "_graph"] = (model, phase, describe)
        else:
            routes[name] = fn
            routes[name + ":fwd_bwd"] = fwd_bwd_of(model)
            checks[name] = (model, phase, describe)

    for mode in ("none", "threshold", "support"):
        for graph in (False, True):
            m = build("default", dev)
            o = FusedAdam(m.parameters(), capturable=graph, **hyper)
            o.register_iht(m)
            m.init_hidden()
            m.train_step(x, y, o, iht="threshold")          # a support to mask with
            if graph:
                o.iht_t.fill_(optim.IHT_MODES[mode])

            def fused(m=m, o=o, iht=(None if graph else mode)):
                m.init_hidden()
                m.train_step(x, y, o, iht=iht)

            add("fused_" + mode, fused, m, mode, fused_state(o), graph)

        mt = build("default", dev)
        ot = torch.optim.Adam(mt.parameters(), foreach=True, **hyper)
        mt.sparsify()

        def chain(mt=mt, ot=ot, mode=mode):
            for p in mt.parameters():
                p.grad = None
            mt.init_hidden()
            mt.loss(x, y).backward()
            ot.step()
            if mode == "threshold":
                mt.sparsify()
            elif mode == "support":
                mt.sparsifyWithSupport()

        add("torch_" + mode, chain, mt, mode, no_state, False)
    mtg = build("default", dev)
    otg = torch.optim.Adam(mtg.parameters(), foreach=True, capturable=True, lr=torch.tensor(0.01, device=dev),
                           weight_decay=1e-5)

    def chain_g():
        for p in mtg.parameters():
            p.grad = None
        mtg.init_hidden()
        mtg.loss(x, y).backward()
        otg.step()

    add("torch_none", chain_g, mtg, "none", no_state, True)
    us, kept = measure(routes, checks, a, a.step_run)
    share = {}
    for k, v in us.items():
        if ":fwd_bwd" in k:
            continue
        base = us.get(k[:-6] + ":fwd_bwd_graph" if k.endswith("_graph") else k + ":fwd_bwd")
        if base:
            share[k] = round((v["median_us"] - base["median_us"]) / v["median_us"], 4)
    return {"B": B, "T": T, "us": us, "share_of_iteration": share, "nonzero_fraction_of_W_U": kept, "notes": notes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--run", type=int, default=200, help="calls per sample of the update part (tens of microseconds each)")
    ap.add_argument("--step-run", type=int, default=20, help="calls per sample of the step part (milliseconds each)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--steps", type=int, default=99)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("update_bench needs a GPU: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    res = {"iters": a.iters, "run": a.run, "step_run": a.step_run, "device": torch.cuda.get_device_name(0),
           "update": {kind: update_part(kind, a, dev) for kind in ("default", "batchnorm3")},
           "step": [step_part(int(b), a, dev) for b in a.batches.split(",")]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
