#!/usr/bin/env python3
"""What augmenting on the device costs: the featuriser reading an audio bank through augmentation records
(fastgrnn_hip_mfcc_augment) beside the plain call, beside the unfused chain, and inside a training step.

    python tools/augment_bench.py [--batch 4096] [--iters 9] [--run 20] [--warmup 3] [--parent-lib PATH]
                                  [--row plain|fused|draw|train] [--limit 240]

The protocol of tools/mfcc_bench.py: B one-second clips, device events around --run consecutive calls, per call; the
median over --iters samples with the 10th / 90th percentiles; --run is raised until a sample lasts at least 0.25 s;
the routes of a row are interleaved sample by sample.
Without --row this process is a driver that never opens the GPU: every row runs in a fresh child process under its own
time limit (--limit seconds), the driver stops at the first row that fails or runs out of time, and prints one JSON
line with the rows that finished.  Rows:

  plain   fastgrnn_hip_mfcc on [B,16000] fp32 and int16, from this tree's library and -- with --parent-lib, the parent
          commit's libfastgrnn_hip.so -- from that one, called through the same ctypes path in the same process.
  fused   the augmented call on a bank of B clips, fp32 and int16, every clip with a shift and a noise; and the unfused
          chain, AudioAugment.apply followed by the plain call, on the same records.
  draw    AudioAugment.draw alone.
  train   one train_step_audio of the default 64 -> 256 -> 128 model (FusedAdam), eager and replayed from a GraphedStep,
          beside train_step on precomputed [T,B,64] features.

Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = ("plain", "fused", "draw", "train")
L = 16000


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
    """Interleaved samples of every route: {name: stats}.  --run is raised until a sample of the first route lasts at
    least 0.25 s."""
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


def setup(a):
    import torch
    from kws_amd import AudioAugment, MFCCFrontend
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    y = (0.1 * torch.randn(a.batch, L, generator=g)).to(dev)
    pcm = (y * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    fe = MFCCFrontend(mean=torch.randn(64, generator=g) * 10, std=torch.rand(64, generator=g) * 20 + 1, device=dev)
    noises = [0.1 * torch.randn(n, generator=g) for n in (16000, 48000, 7000, 960000)]
    # every clip augmented, every clip with a noise: the most the kernel's second gather stream can cost
    kw = dict(p_augment=1.0, max_shift=1600, gain=(0.8, 1.2), p_noise=1.0, noise_gain=0.1, seed=1)
    aug = AudioAugment(noises=noises, device=dev, **kw)
    aug16 = AudioAugment(noises=[(z * 32767.0).round().to(torch.int16) for z in noises], device=dev, **kw)
    index = torch.randperm(a.batch, generator=g).to(torch.int32).to(dev)
    step_t = torch.tensor([7], dtype=torch.int64, device=dev)
    return dev, y, pcm, fe, aug, aug16, index, step_t


def row_plain(a):
    import torch
    from kws_amd import _lib
    from kws_amd.fastgrnn_cuda import _get_raw_stream
    dev, y, pcm, fe, *_ = setup(a)
    fe(y)
    libs = {"this": _lib.load()}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.fastgrnn_hip_mfcc.restype = C.c_int
        parent.fastgrnn_hip_mfcc.argtypes = libs["this"].fastgrnn_hip_mfcc.argtypes
        libs["parent"] = parent
    feats = torch.empty((a.batch, 99, 64), dtype=torch.float32, device=dev)
    stream = _get_raw_stream(torch.cuda.current_device())
    routes, outs = {}, {}
    for name, lib in libs.items():
        for tag, x, code in (("fp32", y, 0), ("int16", pcm, 1)):
            desc = _lib.MfccDesc(a.batch, L, L, code, 32, 1, 9, 99, 80.0, 0)

            def call(lib=lib, desc=desc, x=x):
                st = lib.fastgrnn_hip_mfcc(C.byref(desc), x.data_ptr(), None, fe.tables.data_ptr(), fe.mean.data_ptr(),
                                           fe.std.data_ptr(), feats.data_ptr(), None, 0, stream)
                assert st == 0, st
            call()
            outs[name, tag] = feats.clone()
            routes["%s_%s" % (name, tag)] = call
    res = measure(routes, a)
    if a.parent_lib:
        res["same_bits_as_parent"] = all(torch.equal(outs["this", t], outs["parent", t]) for t in ("fp32", "int16"))
    return res


def row_fused(a):
    import torch
    dev, y, pcm, fe, aug, aug16, index, step_t = setup(a)
    lengths = torch.full((a.batch,), L, dtype=torch.int32, device=dev)
    routes = {}
    for tag, bank, au in (("fp32", y, aug), ("int16", pcm, aug16)):
        rec = au.draw(index, step_t)
        fused = lambda bank=bank, au=au, rec=rec: fe(bank, lengths, augment=rec, noise=au.noise,
                                                     noise_lengths=au.noise_lengths, check=False)
        unfused = lambda bank=bank, au=au, rec=rec: fe(au.apply(bank, lengths, rec), lengths)
        assert torch.equal(fused(), unfused()), tag
        routes["fused_" + tag], routes["unfused_" + tag] = fused, unfused
        routes["plain_" + tag] = lambda bank=bank: fe(bank, lengths)
    res = measure(routes, a)
    for tag in ("fp32", "int16"):
        res["fused_over_unfused_" + tag] = round(res["fused_" + tag]["median_us"] / res["unfused_" + tag]["median_us"], 4)
        res["fused_over_plain_" + tag] = round(res["fused_" + tag]["median_us"] / res["plain_" + tag]["median_us"], 4)
    return res


def row_draw(a):
    dev, y, pcm, fe, aug, aug16, index, step_t = setup(a)
    return measure({"draw": lambda: aug.draw(index, step_t)}, a)


def row_train(a):
    import torch
    from kws_amd import FusedAdam, GraphedStep, RNNClassifierModel
    dev, y, pcm, fe, aug, aug16, index, step_t = setup(a)
    lengths = torch.full((a.batch,), L, dtype=torch.int32, device=dev)
    labels = torch.randint(0, 12, (a.batch,), device=dev)

    def make(capturable=False):
        torch.manual_seed(0)
        m = RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None] * 2, [None] * 2, [1.0] * 2, [1.0] * 2,
                               "sigmoid", "tanh", num_classes=12, device=dev)
        return m, FusedAdam(m.parameters(), lr=1e-3, capturable=capturable)

    (m0, o0), (m1, o1), (m2, o2) = make(), make(), make(True)
    x = fe(pcm).transpose(0, 1).contiguous()

    def features_step():
        m0.init_hidden()
        m0.train_step(x, labels, o0, iht="none")

    def audio_step(m=m1, o=o1):
        m.init_hidden()
        return m.train_step_audio(pcm, lengths, labels, index, fe, aug16, o)

    graphed = GraphedStep(lambda: audio_step(m2, o2))
    res = measure({"train_step_on_features": features_step, "train_step_audio_eager": audio_step,
                   "train_step_audio_graph": graphed}, a)
    res["model"] = "64->256->128, FusedAdam, int16 bank, T=99"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--run", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--row", choices=ROWS, default=None)
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    if a.row:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("augment_bench: needs a GPU")
        print(json.dumps({a.row: globals()["row_" + a.row](a)}))
        return
    res = {"metric": "augment_us_per_call", "batch": a.batch, "samples": L}
    for row in ROWS:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--batch", str(a.batch), "--iters", str(a.iters),
               "--run", str(a.run), "--warmup", str(a.warmup)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            res["stopped_at"] = {"row": row, "why": "time limit of %d s" % a.limit}
            break
        if r.returncode != 0:
            res["stopped_at"] = {"row": row, "why": "exit status %d" % r.returncode, "stderr": r.stderr[-2000:]}
            break
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(res))
    if "stopped_at" in res:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
