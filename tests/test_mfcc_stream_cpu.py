"""The streamed MFCC front end without a GPU: the index facts it rests on, its fp32 restatement (tests/stream_cases.py)
against the fp64 oracle, the C ABI's symbols and refusals (all before any launch), the shim's argument errors, and the
static scans of the new kernel file's assembly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import MFCCFrontend, _lib, features, mfcc_stream_features
from tests import mfcc_cases as M
from tests import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_mfcc_stream.hip")
OK, NULLP, SHAPE, DTYPE, WS, UNSUP = 0, 1, 2, 4, 5, 7


# ---- index facts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", (160, 800, 1600, 16000))
def test_a_clips_frame_is_the_recordings_frame(hop):
    k = hop // 160
    for b in (0, 1, 7):
        for r in range(101):
            lo, hi = S.frame_span(r)
            g = k * b + r
            assert (b * hop + lo, b * hop + hi) == (160 * g - 200, 160 * g + 199)


def test_interior_frames_read_no_sample_outside_the_clip():
    inside = [r for r in range(101) if S.frame_span(r)[0] >= 0 and S.frame_span(r)[1] <= S.CLIP - 1]
    assert inside == list(S.INTERIOR) and sorted(set(range(101)) - set(inside)) == list(S.EDGE_FRAMES)
    assert S.frame_span(2) == (120, 519) and S.frame_span(98) == (15480, 15879)


@pytest.mark.parametrize("N", (16000, 16001, 16159, 16160, 32327, 48000))
def test_the_last_clip_stays_inside_the_workspace(N):
    G = S.n_global_frames(N)
    for hop in (160, 800, 1600, 16000):
        last = (S.n_clips(N, hop) - 1) * hop // 160
        assert last + 98 <= G - 1 and last + 99 <= N // 160 - 1       # interior frames; whole blocks of 160 samples


# ---- the restatement against the fp64 oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("peak", (False, True))
@pytest.mark.parametrize("name", ("mixed", "faint", "speech"))
def test_the_streamed_formulation_holds_the_bound(name, peak):
    rec = S.recordings()[name]
    mel, blk = S.global_frames(rec)
    worst = [0.0, 0.0]
    for b in range(S.n_clips(len(rec), 800)):
        raw = S.clip_features(rec, b, 800, mel, blk, peak=peak)
        r64, r32 = M.oracle_pair(rec[800 * b:800 * b + 16000], 99, n_mfcc=32, order=1, width=9, peak=peak)
        r = M.check_clip(M.finish(raw), r64, r32, 32, 1, what="%s clip %d peak %s" % (name, b, peak))
        worst = [max(a, c) for a, c in zip(worst, r)]
    print("%s peak %s: worst error/bound per block %s" % (name, peak, ["%.3f" % w for w in worst]))


def test_a_silent_clip_is_left_unscaled():
    rec = S.with_a_silent_clip()
    mel, blk = S.global_frames(rec)
    assert np.abs(rec[16000:32000]).max() == 0
    a = S.clip_features(rec, 20, 800, mel, blk, peak=True)
    assert np.isfinite(a).all() and np.array_equal(a, S.clip_features(rec, 20, 800, mel, blk, peak=False))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


ONE = C.c_void_p(256)                          # a non-NULL, 256-byte aligned pointer that no refused call may touch
BIG = 1 << 40


def _desc(**kw):
    f = dict(N=32000, hop=800, audio_dtype=0, clip0=0, B=21, n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, flags=0)
    f.update(kw)
    return _lib.MfccStreamDesc(**f)


def _clips(lib, d=None, audio=ONE, tables=ONE, ws=ONE, ws_bytes=BIG, mean=None, std=None, feats=ONE, no_desc=False):
    d = _desc() if d is None else d
    return lib.fastgrnn_hip_mfcc_stream_clips(None if no_desc else C.byref(d), audio, tables, ws, ws_bytes, mean, std,
                                              feats, None)


def _frames(lib, d=None, audio=ONE, tables=ONE, ws=ONE, ws_bytes=BIG, no_desc=False):
    d = _desc() if d is None else d
    return lib.fastgrnn_hip_mfcc_stream_frames(None if no_desc else C.byref(d), audio, tables, ws, ws_bytes, None)


def test_symbols_exist_and_the_abi_version_stays(lib):
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    for name in ("fastgrnn_hip_mfcc_stream_workspace_bytes", "fastgrnn_hip_mfcc_stream_frames",
                 "fastgrnn_hip_mfcc_stream_clips"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header
    assert lib.fastgrnn_hip_abi_version() == 1 and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.MfccStreamDesc) == 48 and C.sizeof(_lib.MfccDesc) == 48
    assert "typedef struct fastgrnn_mfcc_stream_desc {" in header
    # the frames' mel power and the block maxima at the least, and a function of N alone
    for N in (16000, 32327, 9600000):
        n = lib.fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(_desc(N=N)))
        assert n % 256 == 0 and n >= 4 * (N // 160 + 1) * 129
        assert n == lib.fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(_desc(N=N, hop=160, B=1, clip0=3, order=2)))


def test_null_pointers_are_refused(lib):
    assert _clips(lib, no_desc=True) == NULLP and _frames(lib, no_desc=True) == NULLP
    for arg in ("audio", "tables", "ws"):
        assert _clips(lib, **{arg: None}) == NULLP and _frames(lib, **{arg: None}) == NULLP, arg
    assert _clips(lib, feats=None) == NULLP
    assert _clips(lib, mean=ONE) == NULLP and _clips(lib, std=ONE) == NULLP      # exactly one of the pair


def test_bad_shapes_are_refused(lib):
    for kw in (dict(N=0), dict(N=-16000), dict(hop=0), dict(hop=-800), dict(B=0), dict(B=-1), dict(max_len=0),
               dict(n_mfcc=0), dict(clip0=-1), dict(top_db=float("nan")),
               dict(B=22), dict(clip0=1), dict(clip0=21, B=1), dict(N=16000, B=2), dict(N=16799, B=2),
               dict(N=(1 << 31) - 1, hop=160, B=1 << 23, max_len=1 << 20)):          # size overflow
        assert _clips(lib, _desc(**kw)) == SHAPE, kw
    for kw in (dict(N=0), dict(hop=0), dict(hop=-160)):
        assert _frames(lib, _desc(**kw)) == SHAPE, kw
    for kw in (dict(audio_dtype=2), dict(audio_dtype=-1)):
        assert _clips(lib, _desc(**kw)) == DTYPE and _frames(lib, _desc(**kw)) == DTYPE, kw


def test_what_lies_outside_the_supported_range_is_refused(lib):
    for kw in (dict(hop=801), dict(hop=80), dict(hop=159), dict(N=15999, B=1), dict(N=1 << 31, B=1)):
        assert _clips(lib, _desc(**kw)) == UNSUP and _frames(lib, _desc(**kw)) == UNSUP, kw
    for kw in (dict(n_mfcc=65), dict(order=3), dict(order=-1), dict(width=1), dict(width=4), dict(width=17),
               dict(flags=2), dict(flags=1 | 4)):
        assert _clips(lib, _desc(**kw)) == UNSUP, kw
    # the edges of the range pass the descriptor check (the next refusal in line shows it)
    for kw in (dict(N=16000, B=1), dict(N=(1 << 31) - 1, B=1), dict(hop=160, B=101), dict(hop=16000, B=2),
               dict(clip0=20, B=1), dict(n_mfcc=64, order=2), dict(n_mfcc=1, order=0), dict(width=3), dict(width=15),
               dict(top_db=-1.0), dict(flags=1), dict(audio_dtype=1)):
        assert _clips(lib, _desc(**kw), feats=None) == NULLP, kw
    # the frames call ignores the clips and the feature settings
    for kw in (dict(B=0), dict(clip0=-1), dict(n_mfcc=65), dict(width=4), dict(flags=2), dict(max_len=0)):
        assert _frames(lib, _desc(**kw), tables=None) == NULLP, kw


def test_a_short_or_misaligned_workspace_is_refused(lib):
    need = lib.fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(_desc()))
    assert need > 0
    for fn in (_clips, _frames):
        assert fn(lib, ws_bytes=need - 1) == WS and fn(lib, ws_bytes=0) == WS
        assert fn(lib, ws=C.c_void_p(256 + 64), ws_bytes=need) == WS


# ---- the shim ----------------------------------------------------------------------------------------------------------
def test_the_shims_argument_errors():
    x = torch.zeros(32000)
    with pytest.raises(RuntimeError, match="CUDA"):
        mfcc_stream_features(x)
    with pytest.raises(TypeError):
        mfcc_stream_features(x.numpy())
    with pytest.raises(ValueError, match="feature type"):
        mfcc_stream_features(x, feature_type="delta2")
    assert features._check_stream_geometry(32000, 800, 16000) == 21
    assert features._check_stream_geometry(16000, 160, 16000) == 1
    with pytest.raises(ValueError, match="multiple of 160"):
        features._check_stream_geometry(32000, 801, 16000)
    with pytest.raises(ValueError, match="multiple of 160"):
        features._check_stream_geometry(32000, 0, 16000)
    with pytest.raises(ValueError, match="exactly 16000"):
        features._check_stream_geometry(32000, 800, 8000)
    with pytest.raises(ValueError, match="shorter"):
        features._check_stream_geometry(15999, 800, 16000)
    with pytest.raises(ValueError, match="2\\^31"):
        features._check_stream_geometry(1 << 31, 800, 16000)


def test_frontend_construction_needs_no_gpu():
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"], std=fx["std"], peak_normalize=True)
    assert callable(fe.stream) and fe.peak_normalize and fe.tables is None
    with pytest.raises(RuntimeError, match="GPU|CUDA"):
        fe.stream(torch.zeros(32000))


# ---- static scans of the new kernel source -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_mfcc_stream.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(stream_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), stream_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(stream_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), stream_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_no_branch_between_the_mfmas_of_a_loop(stream_asm):
    """DESIGN 4.0, as tests/test_mfcc_cpu.py checks it for the per-clip kernels: every stretch of MFMAs without a label
    or a branch is whole batches of four k-steps.  The frames kernels run two products (7 x 2 and 4 MFMAs per k-step),
    the clips kernels three (2, 1 and 2).  No new kernel's name contains ``mfcc_k``: the per-clip files' own tests
    count those."""
    kernels, cur = {}, None
    for line in open(stream_asm):
        s = line.split(";")[0].strip()
        if s.endswith(":") and s.startswith("_Z"):
            cur = kernels.setdefault(s[:-1], [])
        elif cur is not None and s and (s.endswith(":") or not s.startswith(".")):
            cur.append(s)
    assert not any("mfcc_k" in k for k in kernels)
    want = {"stream_frames_k": (56, 16), "stream_clips_k": (8, 4, 8)}
    seen = {k: 0 for k in want}
    for name, ins in kernels.items():
        blocks, run = [], 0
        for s in ins:
            if s.startswith("v_mfma"):
                run += 1
            elif s.endswith(":") or s.startswith(("s_cbranch", "s_branch")):
                if run:
                    blocks.append(run)
                run = 0
        if run:
            blocks.append(run)
        for key, per in want.items():
            if key in name:
                seen[key] += 1
                assert len(blocks) == len(per) and [b % q for b, q in zip(blocks, per)] == [0] * len(per), (name, blocks)
    assert seen == {"stream_frames_k": 2, "stream_clips_k": 2}                    # fp32 and int16 audio


def test_the_kernels_use_no_scratch_and_fit_sixteen_waves():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = [r for r in resource_usage.usage(SRC) if "stream_" in r["pretty"]]
    assert len(rows) == 4
    for r in rows:
        # 1024 threads: 4 waves per SIMD, 128 registers each; one workgroup's LDS is the CU's 160 KiB at most
        assert r["scratch"] == 0 and r["vgpr"] + r.get("agpr", 0) <= 128 and r["lds"] <= 163840
