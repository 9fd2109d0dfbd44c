#!/usr/bin/env python3
"""What optimizer.step() costs for the six optimizers of kws_amd.optim beside Adam and SGD -- RMSprop, Adagrad, Adadelta,
Adamax, ASGD, Rprop -- with the fused call (fastgrnn_hip_optim_update: one launch for the default model's 14 tensors) and
with torch.optim.X(foreach=True), each eager and replayed from a captured graph.  The companion of tools/update_bench.py,
which does this for Adam and adds the IHT phases and the whole iteration.

    python tools/optim_bench.py [--iters 15] [--run 200] [--warmup 3] [--timeout 120] [--rules rmsprop,adagrad,...]

The parameter list is the default model's (dense 64 -> 256 -> 128 + a 12-class head: 14 tensors) with fixed gradients and
the reference's OptimizerOptions defaults (through kws_amd.configure_optimizer for the fused routes).  Each rule is one
row, measured in a child process of its own under --timeout seconds (this process never opens the GPU); a child that
runs out of time or dies from a signal ends the run, nothing more is started on the device after it.  Inside a child
the four routes alternate within every repeat.  A sample is a host clock around --run consecutive calls that end in a
device synchronise, per call; medians over --iters samples with the 10th / 90th percentiles, and "device_median_us", the
same window between two device events.  The fused graph route is built with capturable=True; torch's with capturable=True
and a tensor lr where torch.optim has that argument (Adagrad has none: reported under "notes", not timed).

Before and after its timed calls every route must have moved its parameters and kept them finite, else the row ends with
an error instead of a number.  Prints one JSON line; fails without a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RULES = ("RMSprop", "Adagrad", "Adadelta", "Adamax", "ASGD", "Rprop")


def options(name):
    """TrainingOptions with the reference's defaults (trainingConfig.py:43-64)"""
    oo = types.SimpleNamespace(weight_decay=1e-5, momentum=0.9, centered=False, alpha=0, eps=1e-8, rho=0, lr_decay=0,
                               betas=(0.9, 0.999), lambd=0.0001, t0=1000000.0, etas=(0.5, 1.2), dampening=0,
                               step_sizes=(1e-06, 50), nesterov=True)
    return types.SimpleNamespace(optimizer=name, learning_rate=1e-2, optimizer_options=oo)


def torch_kwargs(name):
    """what the reference's configure_optimizer passes to torch.optim (trainClassifier.py:67-95)"""
    oo = options(name).optimizer_options
    return {"RMSprop": dict(weight_decay=oo.weight_decay, eps=oo.eps, alpha=oo.alpha, momentum=oo.momentum, centered=oo.centered),
            "Adagrad": dict(weight_decay=oo.weight_decay, lr_decay=oo.lr_decay),
            "Adadelta": dict(weight_decay=oo.weight_decay, rho=oo.rho, eps=oo.eps),
            "Adamax": dict(weight_decay=oo.weight_decay, betas=oo.betas, eps=oo.eps),
            "ASGD": dict(weight_decay=oo.weight_decay, lambd=oo.lambd, alpha=oo.alpha, t0=oo.t0),
            "Rprop": dict(etas=oo.etas, step_sizes=oo.step_sizes)}[name]


def row(name, a):
    import torch
    import update_bench as UB
    from kws_amd import configure_optimizer
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a GPU: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    notes, routes, models = {}, {}, {}

    def model():
        m = UB.build("default", dev)
        for p in m.parameters():
            p.grad = 0.01 * torch.randn_like(p)
        return m, [p.detach().clone() for p in m.parameters()]

    models["fused"] = model()
    routes["fused"] = configure_optimizer(models["fused"][0].parameters(), options(name)).step
    models["fused_graph"] = model()
    og = configure_optimizer(models["fused_graph"][0].parameters(), options(name), capturable=True)
    UB.try_graph("fused", (lambda: og.step(None)), routes, notes)
    models["torch"] = model()
    routes["torch"] = getattr(torch.optim, name)(models["torch"][0].parameters(), lr=1e-2, foreach=True,
                                                 **torch_kwargs(name)).step
    models["torch_graph"] = model()
    try:
        ot = getattr(torch.optim, name)(models["torch_graph"][0].parameters(), lr=torch.tensor(1e-2, device=dev),
                                        foreach=True, capturable=True, **torch_kwargs(name))
        UB.try_graph("torch", ot.step, routes, notes)
    except TypeError as e:
        notes["torch_graph"] = "does not capture: %s" % (str(e).splitlines()[0][:160],)

    def verify(when):
        for k in routes:
            m, start = models[k]
            for p, p0 in zip(m.parameters(), start):
                if not bool(torch.isfinite(p).all()) or torch.equal(p, p0):
                    raise SystemExit("optim_bench: route %s of %s left a parameter unchanged or not finite %s -- its "
                                     "time would not measure what it names" % (k, name, when))

    UB.interleaved(routes, a.warmup, 2)
    verify("after the warm-up")
    ts = UB.interleaved(routes, a.iters, a.run)
    verify("after the timed calls")
    n = len(list(models["fused"][0].parameters()))
    return {"rule": name, "tensors": n, "elements": sum(p.numel() for p in models["fused"][0].parameters()),
            "device": torch.cuda.get_device_name(0), "notes": notes,
            "us": {k: dict(UB.stats(h), device_median_us=round(UB.pct(d, 0.5), 2)) for k, (h, d) in ts.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--run", type=int, default=200, help="calls per sample (tens of microseconds each)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds a row's child process may take")
    ap.add_argument("--rules", default=",".join(RULES))
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)          # (the child's entry)
    a = ap.parse_args()
    if a.row:
        print(json.dumps(row(a.row, a)))
        return
    rows = []
    for name in a.rules.split(","):
        if name not in RULES:
            raise SystemExit("optim_bench: %r is none of %s" % (name, ", ".join(RULES)))
        cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--iters", str(a.iters), "--run", str(a.run),
               "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"rows": rows}))
            raise SystemExit("optim_bench: the row %s did not finish in %g s; nothing further was started" % (name, a.timeout))
        if r.returncode != 0:
            print(json.dumps({"rows": rows}))
            raise SystemExit("optim_bench: the row %s ended with status %d; nothing further was started\n%s"
                             % (name, r.returncode, (r.stdout + r.stderr)[-2000:]))
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"iters": a.iters, "run": a.run, "rows": rows}))


if __name__ == "__main__":
    main()
