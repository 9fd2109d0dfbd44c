#!/usr/bin/env python3
"""Training step of FastGRNNCUDA at odd hidden sizes on the zero-extended route (FLAG_ZERO_EXTEND), against the same
module at its native padded shape and, once, against the generic scan the odd shape ran on before.

    python tools/zext_bench.py [--batch 4096] [--steps 99] [--iters 10] [--reps 3] [--no-generic]

One step = zero the gradients, forward of the [T,B,F] input, backward of sum(hs * G).  fp32 unless noted.  Median of
--iters steps timed with CUDA events; the configurations are measured round-robin --reps times (interleaved, so that
clock drift hits them alike) and the best median of each is reported.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# (F, H, dtype) on the padded route; each also runs at its native padded shape
CASES = [(32, 100, torch.float32), (100, 100, torch.float32), (64, 200, torch.float32), (32, 64, torch.bfloat16)]


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


def make_step(F, H, dt, B, T, dev, plain=False):
    from kws_amd import FastGRNNCUDA, _route, rnn
    torch.manual_seed(0)
    m = FastGRNNCUDA(F, H, device=dev)
    x = torch.randn(T, B, F, device=dev).to(dt)
    G = torch.randn(T, B, H, device=dev).to(dt)
    params = list(m.parameters())

    def step():
        for p in params:
            p.grad = None
        hs = m(x)
        hs.backward(G)

    if plain:
        # the module as it was before the flag existed: the flag stripped from the one decision that sets it
        key_step = step

        def step():
            saved = rnn._lib.FLAG_ZERO_EXTEND
            rnn._lib.FLAG_ZERO_EXTEND = 0
            _route.route.cache_clear()
            try:
                key_step()
            finally:
                rnn._lib.FLAG_ZERO_EXTEND = saved
                _route.route.cache_clear()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-generic", action="store_true")
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)
    from kws_amd import _lib, fastgrnn_cuda
    dev = torch.device("cuda", 0)
    B, T = a.batch, a.steps
    configs = {}
    res = {"metric": "zext_step_ms", "B": B, "T": T}
    for F, H, dt in CASES:
        tag = "F%dH%d%s" % (F, H, "_bf16" if dt == torch.bfloat16 else "")
        plan = fastgrnn_cuda.zero_extend_plan(T, B, F, H, dtype=dt, flags=_lib.FLAG_SAVE_PREACT)
        assert plan["backward"] == 1, (tag, plan)
        configs[tag + "_zext"] = make_step(F, H, dt, B, T, dev)
        configs[tag + "_native_F%dH%d" % (plan["Fp"], plan["Hp"])] = make_step(plan["Fp"], plan["Hp"], dt, B, T, dev)
    best = {k: float("inf") for k in configs}
    for _ in range(a.reps):
        for k, fn in configs.items():
            best[k] = min(best[k], gpu_time(fn, a.iters))
    res.update({k + "_ms": round(v, 3) for k, v in best.items()})
    for F, H, dt in CASES:
        tag = "F%dH%d%s" % (F, H, "_bf16" if dt == torch.bfloat16 else "")
        z = [v for k, v in best.items() if k.startswith(tag + "_zext")][0]
        n = [v for k, v in best.items() if k.startswith(tag + "_native")][0]
        res[tag + "_zext_over_native"] = round(z / n, 2)
    if not a.no_generic:       # once: the generic scan the (32, 100) step ran on before (path 0)
        fn = make_step(32, 100, torch.float32, B, T, dev, plain=True)
        g = gpu_time(fn, max(2, a.iters // 5), warmup=1)
        res["F32H100_generic_ms"] = round(g, 3)
        res["F32H100_speedup_over_generic"] = round(g / best["F32H100_zext"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
