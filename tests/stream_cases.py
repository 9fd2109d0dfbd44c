"""The streamed MFCC front end's formulation restated in fp32 numpy, and the recordings of its tests
(tests/test_mfcc_stream_cpu.py, tests/test_hip_mfcc_stream.py).

``fastgrnn_hip_mfcc_stream_frames`` / ``_clips`` (include/fastgrnn_hip.h) featurise the overlapping clips of one
recording with every global frame taken through the DFT and the mel projection once.  The restatement follows that
definition operation by operation where the definition says so -- global frames from the zero-padded recording, the
block maxima, interior rows scaled ``(M s) s`` with ``s = 1 / m``, edge rows from the normalised clip -- on the table
image of ``mfcc_cases.tables()``; from the dB on it is ``mfcc_cases.features``'s code path in fp32.  It shares nothing
with the product code and shows, without a GPU, that the formulation itself stays inside the suite's bound.
"""
import functools

import numpy as np
import scipy.fft
import scipy.signal

from tests import mfcc_cases as M

CLIP, HOP, N_FFT = 16000, M.HOP, M.N_FFT
EDGE_FRAMES = (0, 1, 99, 100)
INTERIOR = range(2, 99)


# ---- index facts -------------------------------------------------------------------------------------------------------
def frame_span(r):
    """First and last CLIP sample under frame ``r`` of a clip (center=True: frame r is centred on sample 160 r)."""
    return HOP * r - N_FFT // 2, HOP * r + N_FFT // 2 - 1


def n_clips(N, hop):
    return (N - CLIP) // hop + 1


def n_global_frames(N):
    return N // HOP + 1


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _mel_power(frames, tabs):
    """[n, 400] fp32 frames -> [n, 128] fp32 mel power through the window-folded bases."""
    re = frames @ tabs["cos"]
    im = frames @ tabs["sin"]
    power = re * re + im * im
    assert power.dtype == np.float32
    return power @ tabs["mel"]


def global_frames(rec):
    """``(mel [G, 128], blk [G])`` of a recording: the mel power of every frame g = 0 .. N / 160 with zeros standing in
    for samples outside the recording, and max|y| of every block of 160 samples (the last one may be ragged)."""
    y = M.as_samples(rec)
    G = n_global_frames(len(y))
    padded = np.zeros(HOP * (G - 1) + N_FFT, dtype=np.float32)
    padded[N_FFT // 2:N_FFT // 2 + len(y)] = y
    frames = np.lib.stride_tricks.sliding_window_view(padded, N_FFT)[::HOP]
    assert frames.shape[0] == G
    blocks = np.zeros(G * HOP, dtype=np.float32)
    blocks[:len(y)] = np.abs(y)
    return _mel_power(frames, M.tables()), blocks.reshape(G, HOP).max(axis=1)


def clip_features(rec, b, hop, mel, blk, n_mfcc=32, order=1, width=9, top_db=80.0, peak=False):
    """The raw features ``[101, F]`` fp32 of clip ``b`` from the recording's ``global_frames``."""
    assert hop % HOP == 0
    kb = b * hop // HOP
    y = M.as_samples(rec)[b * hop:b * hop + CLIP]
    m = blk[kb:kb + CLIP // HOP].max()
    assert m == np.abs(y).max()                                    # exact, whatever the order
    scale = peak and m > 0
    if scale:
        y = y / m
    edge = np.lib.stride_tricks.sliding_window_view(np.pad(y, N_FFT // 2), N_FFT)[::HOP][list(EDGE_FRAMES)]
    rows = np.empty((101, M.N_MELS), dtype=np.float32)
    rows[list(EDGE_FRAMES)] = _mel_power(edge, M.tables())
    inner = mel[kb + 2:kb + 99]
    if scale:
        s = np.float32(1.0) / m
        inner = (inner * s) * s
    rows[2:99] = inner
    db = (np.float32(10.0) * np.log10(np.maximum(np.float32(1e-10), rows))).astype(np.float32)
    if top_db is not None and top_db >= 0:
        db = np.maximum(db, db.max() - np.float32(top_db))
    mf = scipy.fft.dct(db, axis=1, type=2, norm="ortho")[:, :n_mfcc]
    out = [mf]
    for o in range(1, order + 1):
        out.append(scipy.signal.savgol_filter(mf, width, polyorder=o, deriv=o, axis=0, mode="interp"))
    out = np.concatenate(out, axis=1)
    assert out.dtype == np.float32
    return out


# ---- recordings --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recordings():
    """The recordings held to the fp64 oracle with peak normalisation on (name -> 1-D array, int16 or fp32)."""
    pcm = M.fixture()["pcm"]
    return {"mixed": M.recording(1, 3.0, pcm, 9000), "faint": M.recording(2, 2.0),
            "speech": np.concatenate([M.speech_like(20), M.speech_like(21), M.speech_like(22)])}


@functools.lru_cache(maxsize=None)
def hostile():
    """Three seconds of the content edges, fp32: a full-scale tone cut to digital silence, a lone impulse at the last
    sample of a silent second, half a second of silence, half a second of DC.  At 0.94-0.98 of the bound for any fp32
    formulation, so they are compared bit for bit (peak off) and not against the oracle."""
    return np.concatenate([M.tone_then_silence(), M.impulse(15999), M.silence(8000), M.dc(8000)])


@functools.lru_cache(maxsize=None)
def with_a_silent_clip():
    """A loud second, exactly one second of digital silence, a loud second: at hop 800 clip 20 is silent (m == 0)."""
    return np.concatenate([M.speech_like(30), M.silence(), M.speech_like(31)])
