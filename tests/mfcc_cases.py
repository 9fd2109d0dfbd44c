"""Oracle, signals and bound of the MFCC front end's tests (tests/test_mfcc_cpu.py, tests/test_hip_mfcc.py).

The oracle restates librosa 0.10.2's defaults as the reference calls them (data_pipeline/mfccProcessor.py:43-58:
``librosa.feature.mfcc(y, sr=16000, n_mfcc, n_fft=400, hop_length=160)`` + ``librosa.feature.delta(width, order)``) with
scipy's own transforms -- ``scipy.fft.rfft``, ``scipy.fft.dct``, ``scipy.signal.savgol_filter`` -- and shares nothing
with the product code.  It runs in fp64 (the truth) and in fp32 with a complex64 FFT (what the reference's own float32
pipeline loses: the yardstick of the bound).  librosa itself is not installed where this suite runs, so bit-level
agreement with it is not verified; every formula below is from its source.
"""
import os

import numpy as np
import scipy.fft
import scipy.signal

SR, N_FFT, HOP, N_MELS = 16000, 400, 160, 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mfcc", "reference_clip.npz")


def fixture():
    d = np.load(GOLDEN)
    return {"pcm": d["pcm"], "mean": d["mean"], "std": d["std"], "classes": [str(c) for c in d["classes"]]}


# ---- librosa.filters.mel(sr=16000, n_fft=400, n_mels=128, fmin=0, fmax=8000, htk=False, norm="slaney") -------------
def _hz_to_mel(f):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_weights():
    """[128, 201] float32 (computed in fp64, rounded once: librosa's ``dtype=np.float32``)."""
    fftfreqs = np.linspace(0.0, SR / 2.0, 1 + N_FFT // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SR / 2.0), N_MELS + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((N_MELS, 1 + N_FFT // 2))
    for i in range(N_MELS):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return w.astype(np.float32)


_MEL = mel_weights()


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)           # scipy get_window("hann", 400, fftbins=True)


def n_frames(length):
    return 1 + length // HOP


def as_samples(y):
    """What ``librosa.load`` hands on: fp32 samples; int16 PCM times 2^-15."""
    y = np.asarray(y)
    if y.dtype == np.int16:
        return y.astype(np.float32) / np.float32(32768.0)
    return y.astype(np.float32)


def features(y, n_mfcc=32, order=1, width=9, top_db=80.0, peak=False, dtype=np.float64):
    """The raw features ``[n, n_mfcc * (order + 1)]`` of one clip, every intermediate in ``dtype``."""
    y = as_samples(y)
    if peak:                                                       # inferencetry.py:172-175, in fp32
        m = np.max(np.abs(y))
        if m > 0:
            y = y / m
    y = y.astype(dtype)
    frames = np.lib.stride_tricks.sliding_window_view(np.pad(y, N_FFT // 2), N_FFT)[::HOP]    # center=True, zeros
    assert frames.shape[0] == n_frames(len(y))
    spec = scipy.fft.rfft(frames * hann().astype(dtype), axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    power = np.abs(spec) ** 2
    mel = power @ _MEL.astype(dtype).T
    db = 10.0 * np.log10(np.maximum(dtype(1e-10), mel))
    if top_db is not None and top_db >= 0:
        db = np.maximum(db, db.max() - dtype(top_db))
    db = db.astype(dtype)
    mf = scipy.fft.dct(db, axis=1, type=2, norm="ortho")[:, :n_mfcc]
    blocks = [mf]
    for o in range(1, order + 1):
        blocks.append(scipy.signal.savgol_filter(mf, width, polyorder=o, deriv=o, axis=0, mode="interp"))
    out = np.concatenate(blocks, axis=1)
    assert out.dtype == dtype
    return out


def finish(raw, max_len=99, mean=None, std=None):
    """Pad with zeros or cut to ``max_len`` frames, then normalise (preprocessing.py:76-88), in fp64."""
    raw = np.asarray(raw, dtype=np.float64)
    out = np.zeros((max_len, raw.shape[1]))
    k = min(max_len, raw.shape[0])
    out[:k] = raw[:k]
    if mean is not None:
        out = (out - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return out


def oracle_pair(y, max_len=99, **kw):
    """(fp64, fp32) oracle outputs ``[max_len, F]`` of one clip, unnormalised."""
    return finish(features(y, dtype=np.float64, **kw), max_len), finish(features(y, dtype=np.float32, **kw), max_len)


def check_clip(got, ref64, ref32, n_mfcc, order, mean=None, std=None, what=""):
    """The bound, per block (mfcc, delta, delta2) of one clip's ``[max_len, F]``:

        max|got - fp64| <= max(4 e32, 2e-6 max|mfcc block|),   e32 = max|fp32 oracle - fp64| on that block.

    ``ref64`` / ``ref32`` are unnormalised.  With ``mean`` / ``std``, ``got`` is compared with ``(ref64 - mean) / std``
    and feature ``f``'s share of the bound is divided by ``|std[f]|`` -- the same error seen through the division -- plus
    two fp32 roundings (the subtraction and the quotient) of the normalised value.  Returns the worst
    error / bound ratio per block."""
    got = np.asarray(got, dtype=np.float64)
    ratios = []
    scale = max(np.abs(ref64[:, :n_mfcc]).max(), 1e-30)
    for o in range(order + 1):
        sl = slice(o * n_mfcc, (o + 1) * n_mfcc)
        e32 = np.abs(ref32[:, sl] - ref64[:, sl]).max()
        tol = max(4.0 * e32, 2e-6 * scale)
        if mean is None:
            err, bound = np.abs(got[:, sl] - ref64[:, sl]), tol
        else:
            s = np.asarray(std, dtype=np.float64)[sl]
            want = (ref64[:, sl] - np.asarray(mean, dtype=np.float64)[sl]) / s
            err = np.abs(got[:, sl] - want)
            bound = tol / np.abs(s) + 2.0 * 2.0 ** -23 * (np.abs(want) + np.abs(np.asarray(mean, dtype=np.float64)[sl] / s))
        ratio = float((err / bound).max())
        ratios.append(ratio)
        assert np.isfinite(got[:, sl]).all(), what
        assert ratio <= 1.0, "%s block %d: error/bound %.3f (e32 %.3g, scale %.3g)" % (what, o, ratio, e32, scale)
    return ratios


# ---- the tables fastgrnn_hip_mfcc_init_tables writes, from the oracle's ingredients ------------------------------------
TAB_BINS = 208                                                    # 201 bins padded to 13 tiles of 16


def tables():
    """The table image as a dict of float32 arrays: ``cos`` / ``sin`` [400, 208] (window folded in, zero columns from
    201 on), ``mel`` [208, 128], ``dct`` [128, 64], ``taps`` [7, 2, 16] (width 3..15, order 1..2, tap)."""
    j = np.arange(N_FFT)[:, None]
    k = np.arange(1 + N_FFT // 2)[None, :]
    ang = 2.0 * np.pi * ((j * k) % N_FFT) / N_FFT
    cos = np.zeros((N_FFT, TAB_BINS))
    sin = np.zeros((N_FFT, TAB_BINS))
    cos[:, :201] = hann()[:, None] * np.cos(ang)
    sin[:, :201] = hann()[:, None] * np.sin(ang)
    mel = np.zeros((TAB_BINS, N_MELS), dtype=np.float32)
    mel[:201] = _MEL.T
    dct = scipy.fft.dct(np.eye(N_MELS), axis=1, type=2, norm="ortho")[:, :64]       # row m: the transform of e_m
    taps = np.zeros((7, 2, 16))
    for wi in range(7):
        w = 3 + 2 * wi
        for o in (1, 2):
            taps[wi, o - 1, :w] = scipy.signal.savgol_coeffs(w, o, deriv=o, use="dot")
    return {"cos": cos.astype(np.float32), "sin": sin.astype(np.float32), "mel": mel, "dct": dct.astype(np.float32),
            "taps": taps.astype(np.float32)}


def split_tables(flat):
    """The device's flat float32 image -> the dict of ``tables()``."""
    flat = np.asarray(flat)
    out, at = {}, 0
    for name, shape in (("cos", (N_FFT, TAB_BINS)), ("sin", (N_FFT, TAB_BINS)), ("mel", (TAB_BINS, N_MELS)),
                        ("dct", (N_MELS, 64)), ("taps", (7, 2, 16))):
        n = int(np.prod(shape))
        out[name] = flat[at:at + n].reshape(shape)
        at += n
    return out


def delta_taps(width, order):
    """The issue's closed forms: y[t] = sum_k tap[k] x[t + k], k = -h..h."""
    h = width // 2
    k = np.arange(-h, h + 1, dtype=np.float64)
    s2, s4 = (k ** 2).sum(), (k ** 4).sum()
    return k / s2 if order == 1 else 2.0 * (width * k ** 2 - s2) / (width * s4 - s2 ** 2)


# ---- signals -----------------------------------------------------------------------------------------------------------
def speech_like(seed, n=16000):
    """Seeded chirps with slow amplitude envelopes over noise, and a silent (exactly zero) gap: fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = np.zeros(n)
    for _ in range(4):
        f0, f1 = rng.uniform(100, 3500, 2)
        phase = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t ** 2 / t[-1])
        env = np.maximum(0.0, np.sin(2 * np.pi * (rng.uniform(1, 4) * t + rng.uniform())))
        y += rng.uniform(0.05, 0.3) * env * np.sin(phase + rng.uniform(0, 6.28))
    y += 0.003 * rng.standard_normal(n)
    a = int(rng.integers(n // 8, n // 2))
    y[a:a + n // 10] = 0.0
    return y.astype(np.float32)


def noise(seed, n=16000, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def silence(n=16000):
    return np.zeros(n, dtype=np.float32)


def dc(n=16000, level=0.25):
    return np.full(n, level, dtype=np.float32)


def impulse(at, n=16000):
    y = np.zeros(n, dtype=np.float32)
    y[at] = 1.0
    return y


def tone_then_silence(n=16000):
    """Full-scale 1 kHz tone for the first half, digital silence after: the top_db floor and the 1e-10 floor both act."""
    y = np.zeros(n, dtype=np.float32)
    half = n // 2
    y[:half] = np.sin(2 * np.pi * 1000.0 * np.arange(half) / SR).astype(np.float32)
    return y


def recording(seed, seconds=2.0, pcm=None, at=0):
    """Faint noise of ``seconds`` with ``pcm`` (int16) mixed in from sample ``at``: int16."""
    n = int(seconds * SR)
    y = np.round(40.0 * np.random.default_rng(seed).standard_normal(n))
    if pcm is not None:
        y[at:at + len(pcm)] += pcm
    return np.clip(y, -32768, 32767).astype(np.int16)
