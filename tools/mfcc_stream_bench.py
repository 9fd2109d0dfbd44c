#!/usr/bin/env python3
"""What computing a recording's frames once saves the detector: the streamed front end (fastgrnn_hip_mfcc_stream_frames
+ _clips) beside the per-clip call on the same overlapping clips, alone and inside detect_audio.

    python tools/mfcc_stream_bench.py [--seconds 600] [--hop 800] [--iters 9] [--run 2] [--warmup 2]
                                 [--row frontend|detect] [--limit 300]

The protocol of tools/augment_bench.py: device events around --run consecutive calls, per call; the median over --iters
samples with the 10th / 90th percentiles; --run is raised until a sample lasts at least 0.25 s; the routes of a row are
interleaved sample by sample in one process.  Without --row this process is a driver that never opens the GPU: every row
runs in a fresh child process under its own time limit (--limit seconds), the driver stops at the first row that fails
or runs out of time, and prints one JSON line with the rows that finished.  The input is an int16 recording of
--seconds at --hop (600 s at 800: 11 981 clips).  Before a row times anything it checks the streamed output against the
per-clip one: equal bit for bit without peak normalisation, the same predictions from detect_audio's two routes.  Rows:

  frontend  the per-clip call on MFCCFrontend.clips_of(recording); the frames call alone; the clips call alone on a
            ready workspace; frames + clips back to back (their sum as the shim runs it, its allocations included).
            Each with peak normalisation off and on (the detector's setting).
  detect    RNNClassifierModel.detect_audio of the default 64 -> 256 -> 128 FastGRNNCUDA model, shared_frames False and
            True, and the model + vote alone on a ready pool.

Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = ("frontend", "detect")


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
    from kws_amd import MFCCFrontend
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = int(a.seconds * 16000)
    # noise under a slow envelope: every clip has a peak of its own
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    y = 0.1 * torch.randn(n, generator=g) * (0.55 + 0.45 * torch.sin(2 * torch.pi * 0.37 * t))
    rec = (y * 32767.0).round().clamp(-32768, 32767).to(torch.int16).to(dev)
    fe = MFCCFrontend(mean=torch.randn(64, generator=g) * 10, std=torch.rand(64, generator=g) * 20 + 1, device=dev)
    return dev, rec, fe


def row_frontend(a):
    import torch
    from kws_amd import MFCCFrontend, _lib
    from kws_amd.fastgrnn_cuda import _get_raw_stream
    dev, rec, fe = setup(a)
    lib = _lib.load()
    clips = MFCCFrontend.clips_of(rec, a.hop)
    B, N = clips.shape[0], rec.shape[0]
    stream = _get_raw_stream(torch.cuda.current_device())
    routes, res = {}, {"clips": B}
    for tag, peak in (("", False), ("_peak", True)):
        fe.peak_normalize = peak
        want, got = fe(clips), fe.stream(rec, a.hop)
        if peak:
            res["max_abs_difference_peak"] = float((want - got).abs().max())
        else:
            assert torch.equal(want, got), "the streamed features differ from the per-clip call's"
            res["bit_equal_peak_off"] = True
        del want
        desc = _lib.MfccStreamDesc(N, a.hop, 1, 0, B, 32, 1, 9, 99, 80.0, int(peak))
        nbytes = lib.fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(desc))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        feats = torch.empty_like(got)

        def frames(desc=desc, ws=ws, nbytes=nbytes):
            st = lib.fastgrnn_hip_mfcc_stream_frames(C.byref(desc), rec.data_ptr(), fe.tables.data_ptr(), ws.data_ptr(),
                                                     nbytes, stream)
            assert st == 0, st

        def clips_call(desc=desc, ws=ws, nbytes=nbytes, feats=feats):
            st = lib.fastgrnn_hip_mfcc_stream_clips(C.byref(desc), rec.data_ptr(), fe.tables.data_ptr(), ws.data_ptr(),
                                                    nbytes, fe.mean.data_ptr(), fe.std.data_ptr(), feats.data_ptr(), stream)
            assert st == 0, st

        frames()
        clips_call()
        assert torch.equal(feats, got), "the raw calls differ from the shim's"
        del got
        routes["per_clip" + tag] = lambda peak=peak: (setattr(fe, "peak_normalize", peak), fe(clips))
        if not peak:
            routes["frames"] = frames
        routes["clips" + tag] = clips_call
        routes["streamed" + tag] = lambda peak=peak: (setattr(fe, "peak_normalize", peak), fe.stream(rec, a.hop))
    res.update(measure(routes, a))
    for tag in ("", "_peak"):
        res["frames_plus_clips%s_us" % tag] = round(res["frames"]["median_us"] + res["clips" + tag]["median_us"], 2)
        res["per_clip_over_streamed" + tag] = round(res["per_clip" + tag]["median_us"] / res["streamed" + tag]["median_us"], 3)
    return res


def row_detect(a):
    import torch
    from kws_amd import RNNClassifierModel, head
    dev, rec, fe = setup(a)
    torch.manual_seed(0)
    m = RNNClassifierModel("FastGRNNCUDA", 64, 2, [256, 128], [None] * 2, [None] * 2, [1.0] * 2, [1.0] * 2,
                           "sigmoid", "tanh", num_classes=12, batch_first=True, device=dev)
    m.eval()
    per_clip = lambda: m.detect_audio(rec, fe, a.hop)
    shared = lambda: m.detect_audio(rec, fe, a.hop, shared_frames=True)
    p0, p1 = per_clip()[0], shared()[0]
    agree = float((p0 == p1).float().mean())
    fe.peak_normalize = True
    pool = fe.stream(rec, a.hop)
    fe.peak_normalize = False

    def behind_the_pool():
        m.init_hidden()
        p, _ = m.predict(pool)
        m.init_hidden()
        return head.vote_windows(p.reshape(1, -1), 10, 5)

    res = {"clips": int(p0.numel()), "predictions_agree": agree}
    res.update(measure({"detect_per_clip": per_clip, "detect_shared_frames": shared, "model_and_vote": behind_the_pool}, a))
    res["per_clip_over_shared"] = round(res["detect_per_clip"]["median_us"] / res["detect_shared_frames"]["median_us"], 3)
    res["model"] = "64->256->128 FastGRNNCUDA, random weights, T=99"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--hop", type=int, default=800)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--run", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row", choices=ROWS, default=None)
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    if a.row:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("mfcc_stream_bench: needs a GPU")
        print(json.dumps({a.row: globals()["row_" + a.row](a)}))
        return
    res = {"metric": "stream_us_per_call", "seconds": a.seconds, "hop": a.hop}
    for row in ROWS:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--seconds", str(a.seconds), "--hop", str(a.hop),
               "--iters", str(a.iters), "--run", str(a.run), "--warmup", str(a.warmup)]
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
