#!/usr/bin/env python3
"""Training step of the BatchNorm keyword spotter on the GPU: FastGRNNBatchNormCUDA's fused kernels against the
reference formula per frame in torch ops (the path the reference itself takes on a GPU), same model, same GPU.

    python tools/bn_train_bench.py [--batches 128,4096] [--steps 99] [--iters 10]

Model: RNNClassifierModel("FastGRNNBatchNormCUDA", 64 -> 256 -> 128 -> 128, 12 classes), time-major, training mode.
One step = zero the gradients, loss() (fused head) and backward.  Each configuration is timed eager and replayed from
a HIP graph (kws_amd.GraphedStep); median of --iters steps, CUDA events.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HIDDEN, F_IN, C = [256, 128, 128], 64, 12


def model(dev, torch_ops):
    from kws_amd import RNNClassifierModel
    m = RNNClassifierModel("FastGRNNBatchNormCUDA", F_IN, 3, HIDDEN, [None] * 3, [None] * 3, [1.0] * 3, [1.0] * 3,
                           "sigmoid", "tanh", num_classes=C, device=dev).train()
    if torch_ops:
        for r in m.rnn_list:
            r._fused = lambda *a: False                 # the per-frame torch-op path on the same shapes
    return m


def gpu_time(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)
    from kws_amd import GraphedStep
    dev = torch.device("cuda", 0)
    res = {"metric": "bn_train_step_ms", "T": a.steps}
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(a.steps, B, F_IN, device=dev, generator=g)
        y = torch.randint(0, C, (B,), device=dev, generator=g)
        for tag, torch_ops in (("fused", False), ("torch_ops", True)):
            m = model(dev, torch_ops)

            def step():
                for p in m.parameters():
                    p.grad = None
                m.init_hidden()
                loss = m.loss(x, y)
                loss.backward()
                return loss.detach()

            iters = a.iters if not torch_ops else max(3, a.iters // 3)
            res["%s_B%d_eager_ms" % (tag, B)] = round(gpu_time(step, iters), 3)
            gs = GraphedStep(step, warmup=2)
            res["%s_B%d_graph_ms" % (tag, B)] = round(gpu_time(gs, iters), 3)
            del gs, m
            torch.cuda.empty_cache()
        for mode in ("eager", "graph"):
            res["speedup_B%d_%s" % (B, mode)] = round(res["torch_ops_B%d_%s_ms" % (B, mode)] /
                                                      res["fused_B%d_%s_ms" % (B, mode)], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
