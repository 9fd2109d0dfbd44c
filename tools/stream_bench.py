#!/usr/bin/env python3
"""Scoring every window of a stream: gathered windows through the existing forward against forward_windows.

    python tools/stream_bench.py [--windows 4096] [--steps 99] [--hop 1] [--iters 30] [--warmup 5]

One stream of L = (windows - 1) * hop + steps frames, every window of `steps` frames at hop `hop` scored through
layer 0 of the two default models (32 -> 256 and 64 -> 256, FastGRNNCUDA, batch-major), two ways in one process,
alternating:
  (a) gather  : windows = stream[starts[:, None] + arange(T)] with torch, then the module's forward under
                torch.no_grad() -- what the library could do before forward_windows existed (batch-major, so no
                transpose copy on top of the gather);
  (b) windows : forward_windows on the stream in place (check=False: no host synchronisation inside the timed region).
Times are device events on the stream the work runs on, after a warm-up of both routes; medians over --iters with the
10th / 90th percentiles as the run-to-run spread.  The gather's own time inside (a) is taken with a third event.  Bytes
are computed from the shapes and the library's workspace queries: the frames each route keeps in memory (x) and the
frame product it parks (P: layers wider than 32 features).  Both routes must give the same bits.  Prints one JSON line;
fails without a GPU.
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
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--hop", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU: a time taken elsewhere says nothing about it")
    from kws_amd import FastGRNNCUDA, _lib, fastgrnn_cuda
    dev = torch.device("cuda:0")
    B, T, H = a.windows, a.steps, 256
    L = (B - 1) * a.hop + T
    res = {"windows": B, "steps": T, "hop": a.hop, "frames": L, "H": H, "iters": a.iters, "layers": {}}
    ev = lambda: torch.cuda.Event(enable_timing=True)                      # noqa: E731
    for F in (32, 64):
        torch.manual_seed(F)
        m = FastGRNNCUDA(F, H, batch_first=True, device=dev)
        stream = torch.randn(L, F, device=dev)
        starts = (torch.arange(B, device=dev) * a.hop).to(torch.int32)
        index = starts.long()[:, None] + torch.arange(T, device=dev)
        assert fastgrnn_cuda.windows_supported(T, B, F, H, flags=_lib.FLAG_BATCH_MAJOR)

        def gather_route(mid=None):
            x = stream[index]                                              # [B,T,F]
            if mid is not None:
                mid.record()
            with torch.no_grad():
                return m(x)

        def windows_route():
            return m.forward_windows(stream, starts, T, check=False)

        for _ in range(a.warmup):
            ya, yb = gather_route(), windows_route()
        torch.cuda.synchronize()
        same = bool(torch.equal(ya, yb))
        del ya, yb
        ta, tg, tb = [], [], []
        for _ in range(a.iters):                                           # alternating, same process
            e0, em, e1, e2 = ev(), ev(), ev(), ev()
            e0.record()
            gather_route(em)
            e1.record()
            windows_route()
            e2.record()
            e2.synchronize()
            ta.append(e0.elapsed_time(e1)); tg.append(e0.elapsed_time(em)); tb.append(e1.elapsed_time(e2))
        med = lambda ts: pct(ts, 0.5)                                      # noqa: E731
        ws_a = fastgrnn_cuda._plan(T, B, F, H, 0, 0, 0, 2, _lib.F32, _lib.FLAG_BATCH_MAJOR | _lib.FLAG_ZERO_EXTEND).ws[0]
        ws_b = fastgrnn_cuda._pool_plan((T, B, F, H, 0, 0, 0, 2, _lib.F32, _lib.FLAG_BATCH_MAJOR), "windows", L).ws_forward
        res["layers"]["%d->%d" % (F, H)] = {
            "gather_route_ms": {"median": med(ta), "p10": pct(ta, 0.1), "p90": pct(ta, 0.9)},
            "windows_route_ms": {"median": med(tb), "p10": pct(tb, 0.1), "p90": pct(tb, 0.9)},
            "gather_alone_ms": med(tg),
            "gather_share_of_gather_route": med(tg) / med(ta),
            "windows_over_gather": med(tb) / med(ta),
            "same_bits": same,
            "x_bytes": {"gather_route": L * F * 4 + B * T * F * 4, "windows_route": L * F * 4},
            "P_bytes": {"gather_route": B * T * H * 4 if F != 32 else 0, "windows_route": L * H * 4 if F != 32 else 0},
            "workspace_bytes": {"gather_route": int(ws_a), "windows_route": int(ws_b)},
            "hs_bytes": B * T * H * 4,
        }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
