#!/usr/bin/env python3
"""What featurising costs: kws_amd.mfcc_features (fastgrnn_hip_mfcc) on B one-second clips, beside a host featuriser and
beside the training step those features feed.

    python tools/mfcc_bench.py [--batch 4096] [--iters 9] [--run 40] [--warmup 3] [--host-clips 512] [--steps 99]

Printed, all from this one run:

  mfcc        the call on [B,16000] fp32 and on int16 PCM (n_mfcc 32, delta, width 9, max_len 99, normalised), device
              events around --run consecutive calls, per call; median over --iters samples with the 10th / 90th
              percentiles.  --run is raised until a sample lasts at least 0.25 s.
  model       algorithmic FLOPs and bytes of the call, from the shapes alone (below), and what the measured time makes
              of them against the MI355X's fp32 matrix peak (157.3 TFLOP/s) and HBM bandwidth (8 TB/s).
  host        an fp32 NUMPY RESTATEMENT of the same chain (rfft, mel product, log10, DCT product, FIR) on 16 host
              threads: a stand-in for the reference's librosa call, which is not installed here -- not librosa itself.
  train_step  one iteration of the default 64 -> 256 -> 128 model (FusedAdam, no IHT phase) at the same B and T = --steps
              on [T,B,64] frames: the consumer the front end has to keep up with.

Prints one JSON line; fails without a GPU.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
N_FFT, HOP, BINS, MELS = 400, 160, 201, 128


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def stats(ts):
    return {"median_us": round(pct(ts, 0.5), 2), "p10_us": round(pct(ts, 0.1), 2), "p90_us": round(pct(ts, 0.9), 2),
            "n": len(ts)}


def device_us(fn, run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(run):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / run


def cost_model(B, L, n_mfcc, order, width, max_len, sample_bytes):
    """Algorithmic work of one call: the products as dense matrix products over the n real frames (what an
    implementation without the kernel's padding to 112 x 208 would do), 2 FLOPs per multiply-add."""
    n = 1 + L // HOP
    F = n_mfcc * (order + 1)
    flops = {"dft": 2.0 * n * N_FFT * 2 * BINS, "power": 3.0 * n * BINS, "mel": 2.0 * n * BINS * MELS,
             "dct": 2.0 * n * MELS * n_mfcc, "delta": 2.0 * n * n_mfcc * width * order}
    per_clip = sum(flops.values())
    bytes_per_clip = L * sample_bytes + max_len * F * 4          # samples in, rows out; the tables stay in L2
    return {"frames": n, "flops_per_clip": per_clip, "dft_share": round(flops["dft"] / per_clip, 3),
            "flops": per_clip * B, "bytes": float(bytes_per_clip) * B}


# ---- the host restatement (fp32 numpy; one clip per call) --------------------------------------------------------------
def host_tables():
    f_sp, logstep = 200.0 / 3, np.log(6.4) / 27.0
    mel_max = 15.0 + np.log(8.0) / logstep
    m = np.linspace(0.0, mel_max, MELS + 2)
    hz = np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), f_sp * m)
    f = np.linspace(0.0, 8000.0, BINS)
    lower = (f[None, :] - hz[:-2, None]) / (hz[1:-1] - hz[:-2])[:, None]
    upper = (hz[2:, None] - f[None, :]) / (hz[2:] - hz[1:-1])[:, None]
    mel = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (hz[2:] - hz[:-2]))[:, None]
    k = np.arange(MELS)
    dct = np.sqrt(2.0 / MELS) * np.cos(np.pi * (2 * k[:, None] + 1) * k[None, :] / (2.0 * MELS))
    dct[:, 0] = np.sqrt(1.0 / MELS)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    return win.astype(np.float32), mel.T.astype(np.float32), dct.astype(np.float32)


def host_features(y, tabs, n_mfcc=32, width=9, max_len=99, mean=None, std=None):
    win, mel, dct = tabs
    frames = np.lib.stride_tricks.sliding_window_view(np.pad(y, N_FFT // 2), N_FFT)[::HOP]
    spec = np.fft.rfft(frames * win, axis=1).astype(np.complex64)
    db = 10.0 * np.log10(np.maximum(np.float32(1e-10), (spec.real ** 2 + spec.imag ** 2) @ mel))
    db = np.maximum(db, db.max() - np.float32(80.0))
    mf = db @ dct[:, :n_mfcc]
    h = width // 2
    taps = (np.arange(-h, h + 1) / float(sum(q * q for q in range(-h, h + 1)))).astype(np.float32)
    idx = np.clip(np.arange(len(mf)), h, len(mf) - 1 - h)
    d = sum(taps[q + h] * mf[idx + q] for q in range(-h, h + 1))
    out = np.zeros((max_len, 2 * n_mfcc), dtype=np.float32)
    k = min(max_len, len(mf))
    out[:k, :n_mfcc], out[:k, n_mfcc:] = mf[:k], d[:k]
    return (out - mean) / std if mean is not None else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--run", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-clips", type=int, default=512)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=99)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mfcc_bench: needs a GPU")
    from kws_amd import FusedAdam, MFCCFrontend, RNNClassifierModel
    dev = torch.device("cuda:0")
    B, L = a.batch, 16000
    g = torch.Generator().manual_seed(0)
    y = (0.1 * torch.randn(B, L, generator=g)).to(dev)
    pcm = (y * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    mean = torch.randn(64, generator=g) * 10
    std = torch.rand(64, generator=g) * 20 + 1
    fe = MFCCFrontend(mean=mean, std=std, device=dev)
    res = {"metric": "mfcc_us_per_call", "batch": B, "samples": L, "n_mfcc": 32, "feature_type": "delta", "width": 9,
           "max_len": 99}

    # ---- the call
    routes = {"fp32": lambda: fe(y), "int16": lambda: fe(pcm)}
    for fn in routes.values():
        for _ in range(a.warmup):
            fn()
    run = a.run
    while device_us(routes["fp32"], run) * run < 0.25e6 and run < 100000:
        run *= 2
    ts = {k: [] for k in routes}
    for _ in range(a.iters):
        for k, fn in routes.items():
            ts[k].append(device_us(fn, run))
    res["run"] = run
    res["mfcc"] = {k: stats(v) for k, v in ts.items()}
    for k, sb in (("fp32", 4), ("int16", 2)):
        m = cost_model(B, L, 32, 1, 9, 99, sb)
        t = res["mfcc"][k]["median_us"] * 1e-6
        m.update(clips_per_s=round(B / t), tflops=round(m["flops"] / t / 1e12, 2),
                 share_of_f32_matrix_peak=round(m["flops"] / t / PEAK_F32_MATRIX, 4),
                 gbytes_per_s=round(m["bytes"] / t / 1e9, 1), share_of_hbm_peak=round(m["bytes"] / t / PEAK_HBM, 4),
                 time_at_matrix_peak_us=round(m["flops"] / PEAK_F32_MATRIX * 1e6, 1),
                 time_at_hbm_peak_us=round(m["bytes"] / PEAK_HBM * 1e6, 1))
        res.setdefault("model", {})[k] = m

    # ---- the host restatement, checked against the device before it is timed
    tabs = host_tables()
    hy = y[:a.host_clips].cpu().numpy()
    hm, hs = mean.numpy(), std.numpy()
    got = fe(y[:4]).cpu().numpy()
    want = np.stack([host_features(hy[i], tabs, mean=hm, std=hs) for i in range(4)])
    res["host_restatement_max_abs_diff"] = float(np.abs(got - want).max())
    with ThreadPoolExecutor(a.host_threads) as pool:
        chunks = np.array_split(np.arange(len(hy)), a.host_threads)
        work = lambda idx: [host_features(hy[i], tabs, mean=hm, std=hs) for i in idx]
        list(pool.map(work, chunks))                                   # warm
        t0 = time.perf_counter()
        list(pool.map(work, chunks))
        dt = time.perf_counter() - t0
    res["host"] = {"what": "fp32 numpy restatement (not librosa)", "threads": a.host_threads, "clips": len(hy),
                   "clips_per_s": round(len(hy) / dt), "us_per_%d_clips" % B: round(dt / len(hy) * B * 1e6)}

    # ---- the consumer
    torch.manual_seed(0)
    model = RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None] * 2, [None] * 2, [1.0] * 2, [1.0] * 2,
                               "sigmoid", "tanh", num_classes=12, device=dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    x = torch.randn(a.steps, B, 64, device=dev)
    labels = torch.randint(0, 12, (B,), device=dev)

    def step():
        model.init_hidden()
        model.train_step(x, labels, opt, iht="none")

    for _ in range(a.warmup):
        step()
    res["train_step"] = dict(stats([device_us(step, 20) for _ in range(a.iters)]), T=a.steps, model="64->256->128, FusedAdam")
    res["mfcc_over_train_step"] = round(res["mfcc"]["fp32"]["median_us"] / res["train_step"]["median_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
