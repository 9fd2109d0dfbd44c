#!/usr/bin/env python3
"""One training step of layer 0 from a frame pool: gathered windows through the module against unroll_windows.

    python tools/pool_train_bench.py [--batch 4096] [--steps 99] [--iters 30] [--warmup 5]

Layer 0 of a model -- FastGRNNCUDA 32 -> 128, 32 -> 256 and 64 -> 256, time-major -- runs one forward + backward on B
windows of T frames cut from a pool on the device, with the windows at hop 1 and at random starts, two ways in one
process, alternating:
  (a) gather  : x = gather_windows(pool, starts, T) transposed to [T,B,F] with torch, then the module's forward and
                backward -- today's step (autograd keeps the [T,B,F] copy alive until the backward);
  (b) windows : unroll_windows (check=False: no host synchronisation inside the timed region): the forward reads the
                pool in place (H=256; H=128 gathers into its workspace), the backward gathers its own copy of x into
                its workspace.
The loss is sum(hs * G) for a fixed G, so both backwards take a dense gradient.  Times are device events on the stream
the work runs on, after a warm-up of both routes; medians over --iters with the 10th / 90th percentiles as the
run-to-run spread.  Bytes are computed from the shapes and the library's workspace queries: what each route keeps of x
between its forward and its backward, and the workspace of its backward.  Both routes must give the same bits (hs and
every parameter gradient).  Prints one JSON line; fails without a GPU.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_train_bench needs a GPU: a time taken elsewhere says nothing about it")
    from kws_amd import FastGRNNCUDA, _lib, fastgrnn_cuda
    from kws_amd.rnn import gather_windows
    dev = torch.device("cuda:0")
    B, T = a.batch, a.steps
    R = 4 * B + T                                                          # hop 1 uses its first B + T - 1 rows
    res = {"batch": B, "steps": T, "pool_rows": R, "iters": a.iters, "layers": {}}
    ev = lambda: torch.cuda.Event(enable_timing=True)                      # noqa: E731
    stat = lambda ts: {"median": pct(ts, 0.5), "p10": pct(ts, 0.1), "p90": pct(ts, 0.9)}   # noqa: E731
    for F, H in ((32, 128), (32, 256), (64, 256)):
        torch.manual_seed(F + H)
        m = FastGRNNCUDA(F, H, device=dev)
        params = list(m.parameters())
        pool = torch.randn(R, F, device=dev)
        G = torch.randn(T, B, H, device=dev)
        assert fastgrnn_cuda.train_windows_supported(T, B, F, H)
        layer = res["layers"]["%d->%d" % (F, H)] = {}
        for kind in ("hop1", "random"):
            starts = torch.arange(B, device=dev) if kind == "hop1" else \
                torch.randint(0, R - T + 1, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            starts = starts.to(torch.int32)

            def step(route):
                for q in params:
                    q.grad = None
                if route == "gather":
                    hs = m(gather_windows(pool, starts, T, check=False).transpose(0, 1).contiguous())
                else:
                    hs = m.unroll_windows(pool, starts, T, check=False)
                hs.backward(G)
                return hs

            for _ in range(a.warmup):
                ya = step("gather").detach()
                ga = [q.grad for q in params]
                yb = step("windows").detach()
                gb = [q.grad for q in params]
            torch.cuda.synchronize()
            same = bool(torch.equal(ya, yb)) and all(bool(torch.equal(u, v)) for u, v in zip(ga, gb))
            del ya, yb, ga, gb
            ta, tb = [], []
            for _ in range(a.iters):                                       # alternating, same process
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                step("gather")
                e1.record()
                step("windows")
                e2.record()
                e2.synchronize()
                ta.append(e0.elapsed_time(e1)); tb.append(e1.elapsed_time(e2))
            ws_a = fastgrnn_cuda._plan(T, B, F, H, 0, 0, 0, 2, _lib.F32,
                                       _lib.FLAG_SAVE_PREACT | _lib.FLAG_ZERO_EXTEND | _lib.FLAG_NO_INPUT_GRAD).ws[1]
            ws_b = fastgrnn_cuda._pool_plan((T, B, F, H, 0, 0, 0, 2, _lib.F32, 0), "train_windows", R).ws_backward
            layer[kind] = {
                "gather_route_ms": stat(ta), "windows_route_ms": stat(tb),
                "windows_over_gather": pct(tb, 0.5) / pct(ta, 0.5),
                "same_bits": same,
                # x between the two passes: the gathered [T,B,F] tensor autograd keeps / the [B] int32 starts
                "x_bytes_kept_alive": {"gather_route": B * T * F * 4, "windows_route": B * 4},
                "backward_workspace_bytes": {"gather_route": int(ws_a), "windows_route": int(ws_b)},
            }
        layer["pool_bytes"] = R * F * 4
    print(json.dumps(res))


if __name__ == "__main__":
    main()
