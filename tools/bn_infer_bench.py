#!/usr/bin/env python3
"""Eval-mode FastGRNNBatchNorm inference time against the plain FastGRNNCUDA model of the same shape.

    python tools/bn_infer_bench.py [--batch 4096] [--steps 99] [--iters 20] [--reference DIR]

The trained keyword spotter's shape (64 -> 256 -> 128 -> 128, 12 classes, batch_first) on one GPU, batch-major:
the BatchNorm model's forward, the same-shaped FastGRNNCUDA model's forward under torch.no_grad() in the same
process, and the BatchNorm model at B = 1 (the real-time use of the reference's inference scripts).  With
--reference DIR (a checkout of the reference project) the reference's own FastGRNNBatchNorm stack is timed on the
CPU (--threads, default 16).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HIDDEN, F_IN, C = [256, 128, 128], 64, 12


def model(name, dev):
    from kws_amd import RNNClassifierModel
    m = RNNClassifierModel(name, F_IN, 3, HIDDEN, [None] * 3, [None] * 3, [1.0] * 3, [1.0] * 3, "sigmoid", "tanh",
                           num_classes=C, batch_first=True, device=dev)
    return m.eval()


def gpu_time(fn, iters, warmup=3):
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


def reference_cpu_ms(ref_dir, B, T, threads=16):
    sys.path.insert(0, ref_dir)
    import rnn  # the reference
    torch.set_num_threads(threads)
    layers = [rnn.FastGRNNBatchNorm(f, h, batch_first=False) for f, h in zip([F_IN] + HIDDEN[:-1], HIDDEN)]
    for lay in layers:
        lay.eval()                                  # (the reference's train() returns None)
    fc = torch.nn.Linear(HIDDEN[-1], C)
    x = torch.randn(T, B, F_IN)

    def run():
        with torch.no_grad():
            r = x
            for lay in layers:
                r = lay(r, training=False)
            return torch.log_softmax(fc(r[-1]), dim=1)
    run()
    t0 = time.perf_counter()
    run()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    res = {"B": a.batch, "T": a.steps, "layout": "batch_major"}
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        bn, plain = model("FastGRNNBatchNorm", dev), model("FastGRNNCUDA", dev)
        x = torch.randn(a.batch, a.steps, F_IN, device=dev)
        x1 = torch.randn(1, a.steps, F_IN, device=dev)

        def fwd(m, inp):
            def f():
                m.init_hidden()
                with torch.no_grad():
                    m(inp)
            return f
        res["bn_eval_ms"] = gpu_time(fwd(bn, x), a.iters)
        res["fastgrnncuda_nograd_ms"] = gpu_time(fwd(plain, x), a.iters)
        res["bn_over_plain"] = res["bn_eval_ms"] / res["fastgrnncuda_nograd_ms"]
        res["bn_eval_b1_ms"] = gpu_time(fwd(bn, x1), a.iters)
        res["fastgrnncuda_nograd_b1_ms"] = gpu_time(fwd(plain, x1), a.iters)
    if a.reference:
        res["reference_cpu_ms"] = reference_cpu_ms(a.reference, a.batch, a.steps, a.threads)
        res["reference_cpu_threads"] = a.threads
    print(json.dumps(res))


if __name__ == "__main__":
    main()
