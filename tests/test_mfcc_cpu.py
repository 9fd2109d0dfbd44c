"""The MFCC front end without a GPU: the oracle of tests/mfcc_cases.py against independent facts, the C ABI's symbols and
refusals (all before any launch), the shim's argument errors, the module's host-side arithmetic, and the static scans of
the kernel's assembly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from kws_amd import MFCCFrontend, _lib, features, mfcc_features
from tests import batchnorm_golden as G
from tests import mfcc_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_mfcc.hip")
OK, NULLP, SHAPE, DTYPE, WS, UNSUP = 0, 1, 2, 4, 5, 7


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", (3, 5, 9, 15))
@pytest.mark.parametrize("order", (1, 2))
def test_taps_are_scipys_savgol_coefficients(width, order):
    want = scipy.signal.savgol_coeffs(width, order, deriv=order, use="dot")
    assert np.abs(M.delta_taps(width, order) - want).max() < 1e-15


@pytest.mark.parametrize("width", (3, 9))
@pytest.mark.parametrize("order", (1, 2))
def test_interp_edges_are_constant(width, order):
    x = np.random.default_rng(3).standard_normal((40, 5))
    y = scipy.signal.savgol_filter(x, width, polyorder=order, deriv=order, axis=0, mode="interp")
    h = width // 2
    taps = M.delta_taps(width, order)
    fir = np.stack([(taps[:, None] * x[t - h:t + h + 1]).sum(0) for t in range(h, 40 - h)])
    assert np.abs(y[h:40 - h] - fir).max() < 1e-13
    assert np.abs(y[:h] - y[h]).max() < 1e-13 and np.abs(y[40 - h:] - y[39 - h]).max() < 1e-13


@pytest.mark.parametrize("length,frames", ((1280, 9), (1439, 9), (1440, 10), (16000, 101)))
def test_frame_counts(length, frames):
    assert M.n_frames(length) == frames
    assert M.features(M.noise(1, length)).shape == (frames, 64)


def test_a_gain_of_ten_moves_c0_alone():
    y = M.noise(5, 16000, 0.01).astype(np.float64)
    a = M.features(y.astype(np.float32), order=2)
    # (the gain applied in fp64 to the fp32 samples: the oracle takes fp32 input, so scale what it computes from)
    b = M.features((10.0 * y).astype(np.float32), order=2)
    d = b - a
    assert np.abs(d[:, 0] - 20.0 * np.sqrt(128.0)).max() < 1e-3          # (fp32 rounding of the scaled samples)
    assert np.abs(d[:, 1:]).max() < 1e-3


def test_silence_is_the_floor():
    f = M.features(M.silence(), order=2)
    assert np.abs(f[:, 0] + 100.0 * np.sqrt(128.0)).max() < 1e-9
    assert np.abs(f[:, 1:]).max() < 1e-9


def test_mel_weights_are_slaney():
    w = M.mel_weights()
    assert w.shape == (128, 201) and w.dtype == np.float32 and (w >= 0).all()
    # 1 kHz is where the scale turns logarithmic: 15 mel of 200/3 Hz
    assert abs(float(M._hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(M._mel_to_hz(15.0)) - 1000.0) < 1e-9
    # bin k is k * 40 Hz; every filter peaks below its Slaney height 2 / (f[i+2] - f[i]) and has bounded support
    mel_f = M._mel_to_hz(np.linspace(0.0, float(M._hz_to_mel(8000.0)), 130))
    assert (w.max(axis=1) <= 2.0 / (mel_f[2:] - mel_f[:-2]) + 1e-9).all()
    for i in (0, 64, 127):
        nz = np.nonzero(w[i])[0] * 40.0
        assert len(nz) == 0 or (nz.min() > mel_f[i] and nz.max() < mel_f[i + 2])


def test_the_trained_model_hears_down():
    fx = M.fixture()
    assert fx["pcm"].shape == (16000,) and fx["pcm"].dtype == np.int16 and fx["classes"][0] == "down" and len(fx["classes"]) == 12
    raw = M.features(fx["pcm"], n_mfcc=32, order=1, width=9, peak=True)
    x = M.finish(raw, 99, fx["mean"], fx["std"])
    _, sd = G.load("trained")
    _, logp = G.model_oracle(sd, torch.from_numpy(x)[:, None, :])
    logp = logp[0].numpy()
    order = np.argsort(-logp)
    assert order[0] == 0 and logp[0] > -1e-2 and logp[order[0]] - logp[order[1]] > 5.0, logp


def test_the_fp32_oracle_is_close_but_not_equal():
    for y in (M.speech_like(1), M.fixture()["pcm"]):
        r64, r32 = M.oracle_pair(y, order=2)
        e = np.abs(r64 - r32).max()
        assert 0 < e < 1e-2


# ---- the C ABI -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


ONE = C.c_void_p(256)                          # a non-NULL pointer that no refused call may touch


def _desc(**kw):
    f = dict(B=2, L=16000, clip_stride=16000, audio_dtype=0, n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, flags=0)
    f.update(kw)
    return _lib.MfccDesc(**f)


def _run(lib, d=None, audio=ONE, lengths=None, tables=ONE, mean=None, std=None, feats=ONE, ws=None, ws_bytes=0, no_desc=False):
    d = _desc() if d is None else d
    return lib.fastgrnn_hip_mfcc(None if no_desc else C.byref(d), audio, lengths, tables, mean, std, feats, ws, ws_bytes, None)


def test_symbols_exist_and_the_abi_version_stays(lib):
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    for name in ("fastgrnn_hip_mfcc_tables_bytes", "fastgrnn_hip_mfcc_init_tables", "fastgrnn_hip_mfcc_workspace_bytes",
                 "fastgrnn_hip_mfcc"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header
    assert lib.fastgrnn_hip_abi_version() == 1
    assert C.sizeof(_lib.MfccDesc) == 48 and "#define FASTGRNN_MFCC_PEAK_NORMALIZE 1u" in header
    n = lib.fastgrnn_hip_mfcc_tables_bytes()
    assert n % 256 == 0 and n >= 4 * (2 * 400 * 208 + 208 * 128 + 128 * 64 + 7 * 2 * 16)
    assert lib.fastgrnn_hip_mfcc_workspace_bytes(C.byref(_desc())) == 0


def test_null_pointers_are_refused(lib):
    assert _run(lib, no_desc=True) == NULLP
    assert _run(lib, audio=None) == NULLP
    assert _run(lib, tables=None) == NULLP
    assert _run(lib, feats=None) == NULLP
    assert _run(lib, mean=ONE) == NULLP and _run(lib, std=ONE) == NULLP          # exactly one of the pair
    assert lib.fastgrnn_hip_mfcc_init_tables(None, None) == NULLP


def test_bad_shapes_are_refused(lib):
    for kw in (dict(B=0), dict(B=-3), dict(L=0), dict(clip_stride=0), dict(clip_stride=-16000), dict(max_len=0),
               dict(n_mfcc=0), dict(top_db=float("nan")), dict(B=1 << 30, max_len=1 << 20)):
        assert _run(lib, _desc(**kw)) == SHAPE, kw
    assert _run(lib, _desc(audio_dtype=2)) == DTYPE and _run(lib, _desc(audio_dtype=-1)) == DTYPE


def test_what_lies_outside_the_supported_range_is_refused(lib):
    for kw in (dict(L=1279), dict(L=16001), dict(n_mfcc=65), dict(order=3), dict(order=-1), dict(width=1), dict(width=4),
               dict(width=17), dict(width=-9), dict(L=1280, width=11),       # 160 * 10 = 1600 samples for eleven frames
               dict(flags=2), dict(flags=1 | 4)):
        assert _run(lib, _desc(**kw)) == UNSUP, kw
    # the edges of the range pass the descriptor check (the next refusal in line shows it)
    for kw in (dict(L=1280, width=9), dict(L=16000, width=15), dict(n_mfcc=64, order=2), dict(n_mfcc=1, order=0),
               dict(width=3), dict(top_db=-1.0), dict(top_db=0.0), dict(flags=1), dict(audio_dtype=1), dict(clip_stride=1),
               dict(L=1600, width=11)):
        assert _run(lib, _desc(**kw), feats=None) == NULLP, kw


# ---- the shim --------------------------------------------------------------------------------------------------------
def test_the_shims_argument_errors():
    x = torch.zeros(2, 16000)
    with pytest.raises(RuntimeError, match="CUDA"):
        mfcc_features(x)
    with pytest.raises(TypeError):
        mfcc_features(x.numpy())
    with pytest.raises(ValueError, match="feature type"):
        mfcc_features(x, feature_type="delta2")
    for bad in (dict(n_mfcc=0), dict(n_mfcc=65), dict(width=4), dict(width=17), dict(max_len=0)):
        with pytest.raises(ValueError):
            features._check_settings(bad.get("n_mfcc", 32), 1, bad.get("width", 9), bad.get("max_len", 99), 16000)
    with pytest.raises(ValueError, match="samples"):
        features._check_settings(32, 1, 9, 99, 16001)
    with pytest.raises(ValueError, match="samples"):
        features._check_settings(32, 1, 9, 99, 1279)
    with pytest.raises(ValueError, match="width 11"):
        features._check_settings(32, 1, 11, 99, 1280)
    with pytest.raises(RuntimeError, match="GPU"):
        features.mfcc_tables("cpu")
    with pytest.raises(ValueError):
        MFCCFrontend(feature_type="energy")
    with pytest.raises(ValueError):
        MFCCFrontend(mean=np.zeros(64))
    with pytest.raises(ValueError, match="64 values"):
        MFCCFrontend(mean=np.zeros(32), std=np.ones(32))


def test_frontend_construction_needs_no_gpu():
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"][None, :, None], std=fx["std"][None, :, None])      # the reference's [1,F,1] files
    assert fe.num_features == 64 and fe.max_len == 99 and fe.width == 9 and fe.order == 1
    assert fe.mean.shape == (64,) and fe.mean.dtype == torch.float32 and torch.equal(fe.std, torch.from_numpy(fx["std"]))
    assert set(fe.state_dict()) == {"mean", "std"}                # the tables are rebuilt, not stored
    assert MFCCFrontend(n_mfcc=13, feature_type="delta_delta").num_features == 39
    assert MFCCFrontend(feature_type="mfcc").num_features == 32


def test_clips_of_is_a_view_with_the_detectors_stride():
    rec = torch.arange(32000, dtype=torch.int16)
    v = MFCCFrontend.clips_of(rec)
    assert v.shape == (21, 16000) and v.stride() == (800, 1) and v.data_ptr() == rec.data_ptr()
    assert int(v[20, -1]) == 31999 and int(v[3, 0]) == 2400                     # the last clip ends the buffer
    v = MFCCFrontend.clips_of(rec[1:], hop_samples=160, clip=1280)
    assert v.shape == ((31999 - 1280) // 160 + 1, 1280) and int(v[2, 5]) == 1 + 320 + 5
    assert MFCCFrontend.clips_of(rec[:16000]).shape == (1, 16000)
    assert MFCCFrontend.clips_of(rec[::2], 400, 8000).stride() == (800, 2)      # (a strided recording keeps its step)
    for bad in (lambda: MFCCFrontend.clips_of(rec[:15999]), lambda: MFCCFrontend.clips_of(rec[None]),
                lambda: MFCCFrontend.clips_of(rec, hop_samples=0)):
        with pytest.raises(ValueError):
            bad()


def test_fit_normalization_is_the_datasets_statistics():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((7, 99, 64)) * 30 + 500).astype(np.float32)
    b = (rng.standard_normal((3, 99, 64)) * 5 - 200).astype(np.float32)
    a[..., 5] = 2.5
    b[..., 5] = 2.5                                                              # a constant feature: std 0 -> 1e-6
    fe = MFCCFrontend()
    mean, std = fe.fit_normalization([torch.from_numpy(a), torch.from_numpy(b)])
    both = np.concatenate([a, b]).astype(np.float64)                             # preprocessing.py:60-66 on [N,T,F]
    want_std = both.std(axis=(0, 1))
    want_std[want_std == 0] = 1e-6
    assert np.abs(mean.numpy() - both.mean(axis=(0, 1))).max() <= 2.0 ** -23 * 600
    assert np.abs(std.numpy() - want_std).max() <= 2.0 ** -23 * 400 and float(std[5]) == np.float32(1e-6)
    assert fe.mean is mean and fe.std.dtype == torch.float32
    with pytest.raises(ValueError):
        fe.fit_normalization([])
    with pytest.raises(ValueError):
        fe.fit_normalization([torch.zeros(2, 99, 32)])


# ---- static scans of the new kernel source ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mfcc_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_mfcc.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(mfcc_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), mfcc_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(mfcc_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), mfcc_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_no_branch_between_the_mfmas_of_a_loop(mfcc_asm):
    """between the first and the last MFMA of a basic-block run, the only conditional branch is a back edge
    that follows the last one -- i.e. no label and no branch sits between two MFMAs of one kernel phase's loop body."""
    kernels, cur = {}, None
    for line in open(mfcc_asm):
        s = line.split(";")[0].strip()
        if s.endswith(":") and s.startswith("_Z"):
            cur = kernels.setdefault(s[:-1], [])
        elif cur is not None and s and (s.endswith(":") or not s.startswith(".")):
            cur.append(s)
    assert any("mfcc_k" in k for k in kernels)
    for name, ins in kernels.items():
        if "mfcc_k" not in name:
            continue
        blocks, run = [], 0                        # MFMAs per maximal stretch without a label or a branch
        for s in ins:
            if s.startswith("v_mfma"):
                run += 1
            elif s.endswith(":") or s.startswith(("s_cbranch", "s_branch")):
                if run:
                    blocks.append(run)
                run = 0
        if run:
            blocks.append(run)
        # the three products in program order, each one stretch per loop body: whole batches of 4 k-steps x
        # (7 x 2 | 4 | 2) MFMAs, however far the compiler unrolled the loop around them
        assert len(blocks) == 3 and [b % q for b, q in zip(blocks, (56, 16, 8))] == [0, 0, 0], (name, blocks)


def test_the_kernels_use_no_scratch_and_fit_sixteen_waves():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = {r["pretty"]: r for r in resource_usage.usage(SRC)}
    main = [r for n, r in rows.items() if "mfcc_k" in n]
    assert len(main) == 2                                                        # fp32 and int16 audio
    for r in main:
        # 1024 threads: 4 waves per SIMD, 128 registers each; one workgroup's LDS is the CU's 160 KiB at most
        assert r["scratch"] == 0 and r["vgpr"] + r.get("agpr", 0) <= 128 and r["lds"] <= 163840
