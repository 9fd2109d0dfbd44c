#!/usr/bin/env python3
"""The inference tail: the fused head + vote against what a user of score_stream / forward had to do before.

    python tools/detect_bench.py [--batch 4096] [--windows 4096] [--iters 30] [--loop-iters 3] [--warmup 5]

Two comparisons in one process, the routes of each alternating inside every repeat (H = 128, C = 12):

  detect   one stream of (windows - 1) + 99 frames at hop 1 through a one-layer 32 -> 128 model:
             fused : detect_stream (layers, head_predict, vote_windows), then the events copied to the host
             host  : score_stream, then argmax on the device, the predictions copied to the host and the reference's
                     vote loop in Python (inferencetry.py:217-227)
           plus the two tails alone on the same last states (head_predict + vote_windows against Linear + log_softmax +
           argmax + copy + loop), so that the scan's time does not dilute the difference.
  accuracy the tail of batch_accuracy on one [batch, 128] tensor of last states:
             fused : head_predict with labels, one copy of (count, predictions) to the host
             torch : Linear, log_softmax, argmax, eq, sum, the same copy
             loop  : Linear, log_softmax, then the reference's batch_accuracy (trainClassifier.py:54-65): one
                     comparison and one sync per utterance (--loop-iters repeats: it takes tens of milliseconds)
           and the device time alone of fused and torch (events, no copy).

Every time but the "device" ones is a host clock around work that ends on the host (the copy synchronises); medians
over --iters with the 10th / 90th percentiles as the run-to-run spread.  The routes must agree on every integer.
Prints one JSON line; fails without a GPU.
"""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def stats(ts):
    return {"median": pct(ts, 0.5), "p10": pct(ts, 0.1), "p90": pct(ts, 0.9), "n": len(ts)}


def host_vote(pred, num_windows=10, majority=5):
    """inferencetry.py:217-227 on a list of predictions: the windows at which a keyword is reported."""
    votes, previous, events = [], None, []
    for w, p in enumerate(pred):
        if len(votes) == num_windows:
            votes.pop(0)
        votes.append(p)
        if len(votes) >= majority:
            word, frequency = collections.Counter(votes).most_common(1)[0]
            if word != previous and frequency >= majority:
                events.append((w, word))
                previous = word
    return events


def reference_batch_accuracy(scores, labels):
    """trainClassifier.py:54-65."""
    batch_size = scores.shape[0]
    passed = 0
    results = []
    for i in range(batch_size):
        expected = labels[i]
        actual = scores[i].argmax()
        results += [int(actual)]
        if expected == actual:
            passed += 1
    return (float(passed) * 100.0 / float(batch_size), passed, results)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def interleaved(routes, iters, timer=host_ms):
    """routes: name -> fn; every repeat runs each route once, in turn.  -> name -> list of ms, name -> last output"""
    ts, outs = {k: [] for k in routes}, {}
    for _ in range(iters):
        for k, fn in routes.items():
            t, outs[k] = timer(fn)
            ts[k].append(t)
    return ts, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench needs a GPU: a time taken elsewhere says nothing about it")
    from kws_amd import RNNClassifierModel, head
    dev = torch.device("cuda:0")
    H, C, T = 128, 12, 99
    res = {"H": H, "C": C, "iters": a.iters}
    torch.manual_seed(0)
    model = RNNClassifierModel("FastGRNNCUDA", 32, 1, [H], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                               num_classes=C, device=dev).eval()
    W, b = model.hidden2keyword.weight.detach(), model.hidden2keyword.bias.detach()

    # ---- detect ----------------------------------------------------------------------------------------------------
    L = a.windows - 1 + T
    stream = torch.randn(1, L, 32, device=dev)

    def fused():
        pred, maj, event = model.detect_stream(stream, hop=1, window=T)
        ev = event[0].cpu()
        idx = (ev >= 0).nonzero()[:, 0]
        return list(zip(idx.tolist(), ev[idx].tolist()))

    def host():
        pred = model.score_stream(stream, hop=1, window=T)[0].argmax(-1).cpu().tolist()
        return host_vote(pred)

    with torch.no_grad():                                              # every window's last state, as score_stream gets it
        h_win = model.rnn_list[0].forward_windows(stream[0], torch.arange(a.windows, device=dev), T, last_state=True,
                                                  check=False).float().contiguous()

    def fused_tail():
        pred, _, _ = head.head_predict(h_win, W, b, want_log_probs=False)
        return head.vote_windows(pred.reshape(1, -1))[1][0].cpu()

    def host_tail():
        with torch.no_grad():
            pred = F.log_softmax(F.linear(h_win, W, b), dim=1).argmax(-1).cpu().tolist()
        return host_vote(pred)

    def fused_tail_device():
        pred, _, _ = head.head_predict(h_win, W, b, want_log_probs=False)
        return head.vote_windows(pred.reshape(1, -1))

    routes = {"fused": fused, "host": host, "fused_tail": fused_tail, "host_tail": host_tail}
    interleaved(routes, a.warmup)
    ts, outs = interleaved(routes, a.iters)
    td, _ = interleaved({"fused_tail_device": fused_tail_device}, a.iters, device_ms)
    res["detect"] = {"windows": a.windows, "frames": L, "events": len(outs["fused"]),
                     "same_events": outs["fused"] == outs["host"],
                     "ms": {k: stats(v) for k, v in {**ts, **td}.items()}}

    # ---- accuracy --------------------------------------------------------------------------------------------------
    B = a.batch
    h = torch.randn(B, H, device=dev)
    labels = torch.randint(0, C, (B,), device=dev)

    def acc_fused():
        pred, _, n = head.head_predict(h, W, b, labels, want_log_probs=False)
        out = torch.cat((n, pred)).cpu().tolist()
        return out[0], out[1:]

    def acc_torch():
        with torch.no_grad():
            pred = F.log_softmax(F.linear(h, W, b), dim=1).argmax(1)
            n = (pred == labels).sum()
            out = torch.cat((n[None], pred)).cpu().tolist()
        return out[0], out[1:]

    def acc_loop():
        with torch.no_grad():
            scores = F.log_softmax(F.linear(h, W, b), dim=1)
        _, passed, results = reference_batch_accuracy(scores, labels)
        return passed, results

    def acc_fused_device():
        return head.head_predict(h, W, b, labels, want_log_probs=False)

    def acc_torch_device():
        with torch.no_grad():
            pred = F.log_softmax(F.linear(h, W, b), dim=1).argmax(1)
            return pred, (pred == labels).sum()

    routes = {"fused": acc_fused, "torch": acc_torch}
    interleaved(routes, a.warmup)
    ts, outs = interleaved(routes, a.iters)
    tl, outl = interleaved({"loop": acc_loop}, a.loop_iters)
    dev_routes = {"fused_device": acc_fused_device, "torch_device": acc_torch_device}
    interleaved(dev_routes, a.warmup, device_ms)
    td, _ = interleaved(dev_routes, a.iters, device_ms)
    differ = sum(int(x != y) for x, y in zip(outs["fused"][1], outs["torch"][1]))
    res["accuracy"] = {"batch": B, "passed": outs["fused"][0],
                       # (the torch chain's logits come from another GEMM: rows with a near-tie may differ)
                       "rows_where_fused_and_torch_differ": differ,
                       "torch_and_loop_agree": outs["torch"] == outl["loop"],
                       "ms": {k: stats(v) for k, v in {**ts, **tl, **td}.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
