#!/usr/bin/env python3
"""What feeding the trainer from the device buys: one iteration of RNNClassifierModel.fit_audio's body -- init_hidden,
TrainSchedule.advance, train_step_audio, TrainSchedule.record -- replayed from one graph with nothing written by the host,
beside the same captured step fed by the host, beside the eager loop.

    python tools/fit_bench.py [--batches 128,4096] [--iters 9] [--run 20] [--warmup 3] [--row fit|advance] [--batch B]
                              [--limit 300]

The protocol of tools/augment_bench.py: device events around --run consecutive iterations, per iteration; the median over
--iters samples with the 10th / 90th percentiles; --run is raised until a sample lasts at least 0.25 s; the variants of a
row are interleaved sample by sample.  Without --row this process is a driver that never opens the GPU: every row runs in
a fresh child process under its own time limit (--limit seconds), the driver stops at the first row that fails or runs
out of time, and prints one JSON line with the rows that finished.  Rows, each at every batch size of --batches:

  fit      the default 32 -> 256 -> 128 model (FusedAdam with the IHT phases registered, StepLR), an int16 bank of
           2 B one-second clips, 16 MFCC + delta, T = 99, every iteration in the middle third of the run (threshold and
           support phases alternate):
             device_fed_graph   the captured body of fit_audio(graph=True)
             host_fed_graph     the same body without advance(), and before every replay three host writes:
                                index.copy_ from pinned memory, lr_t.fill_, iht_t.fill_ -- what a host loader and a
                                host scheduler cost at the least (the shuffle itself is prepared outside the timing)
             eager              the body of fit_audio(graph=False)
  advance  TrainSchedule.advance() alone.
  rolling  the fit row's model on a TrainSchedule(rolling=True) (bag_count 100, every iteration in a full epoch: the
           states go into the bags and come out of them), beside the non-rolling iteration in the same process:
             device_fed_graph   the fit row's, for reference
             rolling_graph      the captured rolling body of fit_audio: advance, RollingBags.exchange, the step, commit,
                                record
             host_exchange      the same graph without exchange(), and before every replay the exchange in torch index
                                ops issued by the host, per layer bag[idx] = state and h0 = bag[:B] (the shuffles are
                                prepared on the device outside the timing)
             exchange           RollingBags.exchange() alone (timed by itself, with its own --run)

Fails without a GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = ("fit", "advance", "rolling")
L, NUM_EPOCHS, TRIM = 16000, 300000, 2


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def stats(ts):
    return {"median_us": round(pct(ts, 0.5), 2), "p10_us": round(pct(ts, 0.1), 2), "p90_us": round(pct(ts, 0.9), 2),
            "n": len(ts)}


def device_us(fn, run):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(run):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / run


def measure(routes, a):
    for fn in routes.values():
        for _ in range(a.warmup):
            fn()
    run, first = a.run, next(iter(routes.values()))
    while device_us(first, run) * run < 0.25e6 and run < 100000:
        run *= 2
    ts = {k: [] for k in routes}
    for _ in range(a.iters):
        for k, fn in routes.items():
            ts[k].append(device_us(fn, run))
    return dict({k: stats(v) for k, v in ts.items()}, run=run)


def trainer(a, dev, **rolling):
    import torch
    from kws_amd import FusedAdam, RNNClassifierModel, TrainSchedule
    torch.manual_seed(0)
    m = RNNClassifierModel("FastGRNNCUDA", 32, 2, [256, 128], [None] * 2, [None] * 2, [0.3] * 2, [0.3] * 2, "sigmoid",
                           "tanh", num_classes=12, device=dev)
    o = FusedAdam(m.parameters(), lr=1e-3, capturable=True)
    o.register_iht(m)
    s = TrainSchedule(o, 2 * a.batch, a.batch, NUM_EPOCHS, seed=1, lr_scheduler="StepLR", gamma=0.999, lr_step_size=1000,
                      sparsify=True, trim_level=TRIM, log_len=4096, **rolling)
    return m, o, s


def middle_third(o, s):
    o.step_t.fill_((NUM_EPOCHS // 3 + 1) * s.full_ticks)


def bank(a, dev, g):
    import torch
    from kws_amd import AudioAugment, MFCCFrontend
    n = 2 * a.batch
    pcm = (0.1 * torch.randn(n, L, generator=g) * 32767.0).round().clamp(-32768, 32767).to(torch.int16).to(dev)
    lengths = torch.full((n,), L, dtype=torch.int32, device=dev)
    labels = torch.randint(0, 12, (n,), generator=g).to(dev)
    fe = MFCCFrontend(n_mfcc=16, mean=torch.randn(32, generator=g) * 10, std=torch.rand(32, generator=g) * 20 + 1, device=dev)
    noises = [(0.1 * torch.randn(k, generator=g) * 32767.0).round().to(torch.int16) for k in (16000, 48000, 7000)]
    aug = AudioAugment(p_augment=0.25, max_shift=1600, gain=(0.8, 1.2), noise_gain=0.1, seed=1, noises=noises, device=dev)
    fe(pcm[:2])
    return pcm, lengths, labels, fe, aug


def row_fit(a):
    import torch
    from kws_amd import GraphedStep, iht_phase
    from kws_amd.optim import IHT_MODES
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = 2 * a.batch
    pcm, lengths, labels, fe, aug = bank(a, dev, g)

    def body(m, o, s, fed):
        m.init_hidden()
        if fed:
            s.advance()
        loss = m.train_step_audio(pcm, lengths, labels, s.index, fe, aug, o, iht=None)
        s.record(loss)
        return loss

    (m0, o0, s0), (m1, o1, s1), (m2, o2, s2) = trainer(a, dev), trainer(a, dev), trainer(a, dev)
    device_fed = GraphedStep(lambda: body(m0, o0, s0, True))
    host_graph = GraphedStep(lambda: body(m1, o1, s1, False))
    # the host's side of the host-fed loop: a shuffled epoch in pinned memory, the rate and the phase per iteration
    order = torch.randperm(n, generator=g).to(torch.int32).reshape(s1.ticks, a.batch).pin_memory()
    host = {"s": (NUM_EPOCHS // 3 + 1) * s1.ticks}

    def host_fed():
        s = host["s"]
        epoch, i_batch = divmod(s, s1.ticks)
        s1.index.copy_(order[i_batch], non_blocking=True)
        o1.lr_t.fill_(1e-3 * 0.999 ** ((s + 1) // 1000))
        o1.iht_t.fill_(IHT_MODES[iht_phase(epoch, NUM_EPOCHS, i_batch, TRIM)])
        host_graph()
        host["s"] = s + 1

    for o, s in ((o0, s0), (o1, s1), (o2, s2)):
        middle_third(o, s)
    res = measure({"device_fed_graph": device_fed, "host_fed_graph": host_fed, "eager": lambda: body(m2, o2, s2, True)}, a)
    torch.cuda.synchronize()
    res["phase_at_the_end"] = [int(o.iht_t) for o in (o0, o1, o2)]
    res["finite"] = bool(torch.isfinite(s0.loss_log).all() and torch.isfinite(s1.loss_log).all())
    res["device_over_host_fed"] = round(res["device_fed_graph"]["median_us"] / res["host_fed_graph"]["median_us"], 4)
    res["device_over_eager"] = round(res["device_fed_graph"]["median_us"] / res["eager"]["median_us"], 4)
    res["model"] = "32->256->128, FusedAdam + IHT, int16 bank of %d clips, 16 MFCC + delta, T=99" % n
    return res


def row_rolling(a):
    import torch
    from kws_amd import GraphedStep, RollingBags
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pcm, lengths, labels, fe, aug = bank(a, dev, g)
    B, bag_count, shuffles = a.batch, 100, 64

    def plain(m, o, s):
        m.init_hidden()
        s.advance()
        loss = m.train_step_audio(pcm, lengths, labels, s.index, fe, aug, o, iht=None)
        s.record(loss)
        return loss

    def rolling(m, o, s, bags, exchange):
        s.advance()
        if exchange:
            bags.exchange()
        else:
            m.hidden_states = list(bags.h0)
        loss = m.train_step_audio(pcm, lengths, labels, s.index, fe, aug, o, iht=None)
        bags.commit()
        s.record(loss)
        return loss

    m0, o0, s0 = trainer(a, dev)
    (m1, o1, s1), (m2, o2, s2) = (trainer(a, dev, rolling=True, bag_count=bag_count) for _ in range(2))
    bags1, bags2 = RollingBags(m1, s1), RollingBags(m2, s2)
    plain_graph = GraphedStep(lambda: plain(m0, o0, s0))
    rolling_graph = GraphedStep(lambda: rolling(m1, o1, s1, bags1, True))
    host_graph = GraphedStep(lambda: rolling(m2, o2, s2, bags2, False))
    idx = torch.stack([torch.randperm(B * bag_count, generator=g)[:B] for _ in range(shuffles)]).to(dev)
    host = {"s": 0}

    def host_exchange():
        rows = idx[host["s"] % shuffles]
        for state, bag, h0 in zip(bags2.state, bags2.bag, bags2.h0):
            bag[rows] = state
            h0.copy_(bag[:B])
        host_graph()
        host["s"] += 1

    for o, s in ((o0, s0), (o1, s1), (o2, s2)):
        middle_third(o, s)
    res = measure({"device_fed_graph": plain_graph, "rolling_graph": rolling_graph, "host_exchange": host_exchange}, a)
    res["exchange"] = measure({"exchange": bags1.exchange}, a)
    torch.cuda.synchronize()
    res["where_at_the_end"] = s1.where.tolist()
    res["finite"] = bool(torch.isfinite(s1.loss_log).all() and torch.isfinite(s2.loss_log).all())
    res["carried"] = bool(all(h.any() for h in bags1.h0))
    res["rolling_over_plain"] = round(res["rolling_graph"]["median_us"] / res["device_fed_graph"]["median_us"], 4)
    res["rolling_over_host_exchange"] = round(res["rolling_graph"]["median_us"] / res["host_exchange"]["median_us"], 4)
    res["bytes_moved_per_exchange"] = 2 * B * sum(m1.hidden_units_list) * 4
    res["model"] = "32->256->128, FusedAdam + IHT, bags of %d rows per layer" % (B * bag_count)
    return res


def row_advance(a):
    import torch
    dev = torch.device("cuda:0")
    m, o, s = trainer(a, dev)
    middle_third(o, s)
    return measure({"advance": s.advance}, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--run", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--row", choices=ROWS, default=None)
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    if a.row:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("fit_bench: needs a GPU")
        print(json.dumps({"%s_b%d" % (a.row, a.batch): globals()["row_" + a.row](a)}))
        return
    res = {"metric": "fit_us_per_iteration", "samples": L}
    for batch in (int(b) for b in a.batches.split(",")):
        for row in ROWS:
            cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--batch", str(batch), "--iters", str(a.iters),
                   "--run", str(a.run), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                res["stopped_at"] = {"row": row, "batch": batch, "why": "time limit of %d s" % a.limit}
                break
            if r.returncode != 0:
                res["stopped_at"] = {"row": row, "batch": batch, "why": "exit status %d" % r.returncode,
                                     "stderr": r.stderr[-2000:]}
                break
            res.update(json.loads(r.stdout.strip().splitlines()[-1]))
            print("fit_bench: row %s at B = %d done" % (row, batch), file=sys.stderr, flush=True)
        if "stopped_at" in res:
            break
    print(json.dumps(res))
    if "stopped_at" in res:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
