#!/usr/bin/env python3
"""What the gradient guard costs: ``train_step`` of the default 64 -> 256 -> 128 model (FusedAdam, T = 99) unguarded,
guarded (``optimizer.guard(max_grad_norm=1.0)``), and unguarded with ``torch.nn.utils.clip_grad_norm_(foreach=True)``
spliced in by hand between ``backward()`` and ``step()``; and the guard call (fastgrnn_hip_grad_guard) alone.

    python tools/guard_bench.py [--batches 128,4096] [--iters 9] [--run 20] [--warmup 3] [--row eager|graph]
                                [--batch B] [--limit 240]

The protocol of tools/augment_bench.py: device events around --run consecutive calls, per call; the median over
--iters samples with the 10th / 90th percentiles; --run is raised until a sample lasts at least 0.25 s; the routes of
a row are interleaved sample by sample, all in one process, so the comparison is guarded against unguarded of the same
library under the same conditions.  Without --row this process is a driver that never opens the GPU: every row (eager
and graph-replayed, at every batch size) runs in a fresh child process under its own time limit (--limit seconds), the
driver stops at the first row that fails or runs out of time, and prints one JSON line with the rows that finished.
No number is a pass condition.  The guard adds two small launches, so the expectation is a few microseconds per
replayed step.

Fails without a GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROWS = ("eager", "graph")
T, F = 99, 64


def row(a):
    import torch
    from augment_bench import measure
    from kws_amd import FusedAdam, GraphedStep, RNNClassifierModel, _lib
    from kws_amd.fastgrnn_cuda import _get_raw_stream
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, a.batch, F, generator=g).to(dev)
    y = torch.randint(0, 12, (a.batch,), generator=g).to(dev)
    graph = a.row == "graph"

    def make(guard):
        torch.manual_seed(0)
        m = RNNClassifierModel("FastGRNNCUDA", F, 2, [256, 128], [None] * 2, [None] * 2, [1.0] * 2, [1.0] * 2,
                               "sigmoid", "tanh", num_classes=12, device=dev)
        o = FusedAdam(m.parameters(), lr=1e-3, capturable=graph)
        return m, (o.guard(max_grad_norm=1.0) if guard else o)

    (m0, o0), (m1, o1), (m2, o2) = make(False), make(True), make(False)
    params2 = list(m2.parameters())

    def unguarded():
        m0.init_hidden()
        return m0.train_step(x, y, o0, iht=None if graph else "none")

    def guarded():
        m1.init_hidden()
        return m1.train_step(x, y, o1, iht=None if graph else "none")

    def torch_clip():                                     # train_step's body with the foreach chain spliced in
        m2.init_hidden()
        for p in params2:
            p.grad = None
        loss = m2.loss(x, y)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params2, 1.0, error_if_nonfinite=False, foreach=True)
        o2.step(None if graph else "none")
        return loss.detach()

    guarded()
    # the guard call alone, on fixed copies of that step's gradients with a state and a workspace of its own
    lib = _lib.load()
    grads = [p.grad.detach().clone() for p in m1.parameters()]
    n, max_norm, flags = len(grads), 1.0, _lib.GUARD_SKIP_NONFINITE
    gsegs = (_lib.GuardSeg * n)(*[_lib.GuardSeg(t.data_ptr(), t.numel()) for t in grads])
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.fastgrnn_hip_grad_guard_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)

    def guard_alone():
        stream = _get_raw_stream(torch.cuda.current_device())    # (the capture's stream while a GraphedStep records it)
        st = lib.fastgrnn_hip_grad_guard(gsegs, n, max_norm, flags, state.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream)
        assert st == 0, st

    routes = {"unguarded": unguarded, "guarded": guarded, "torch_clip_grad_norm": torch_clip, "guard_alone": guard_alone}
    if graph:
        routes = {k: GraphedStep(fn) for k, fn in routes.items()}
    res = measure(routes, a)
    res["guarded_minus_unguarded_us"] = round(res["guarded"]["median_us"] - res["unguarded"]["median_us"], 2)
    res["torch_minus_unguarded_us"] = round(res["torch_clip_grad_norm"]["median_us"] - res["unguarded"]["median_us"], 2)
    res["segments"] = n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--run", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--row", choices=ROWS, default=None)
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    if a.row:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("guard_bench: needs a GPU")
        print(json.dumps({"%s_B%d" % (a.row, a.batch): row(a)}))
        return
    res = {"metric": "train_step_us", "model": "64->256->128, FusedAdam, T=99, max_grad_norm=1.0"}
    for batch in (int(b) for b in a.batches.split(",")):
        for name in ROWS:
            cmd = [sys.executable, os.path.abspath(__file__), "--row", name, "--batch", str(batch), "--iters", str(a.iters),
                   "--run", str(a.run), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                res["stopped_at"] = {"row": "%s_B%d" % (name, batch), "why": "time limit of %d s" % a.limit}
                break
            if r.returncode != 0:
                res["stopped_at"] = {"row": "%s_B%d" % (name, batch), "why": "exit status %d" % r.returncode,
                                     "stderr": r.stderr[-2000:]}
                break
            res.update(json.loads(r.stdout.strip().splitlines()[-1]))
        if "stopped_at" in res:
            break
    print(json.dumps(res))
    if "stopped_at" in res:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
