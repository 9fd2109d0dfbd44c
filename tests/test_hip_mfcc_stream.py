"""The streamed MFCC front end on the GPU: ``mfcc_stream_features`` (a recording's frames computed once, then its
overlapping clips) against the per-clip call it is defined by.

Without peak normalisation the two are equal bit for bit, for any signal.  With it the streamed call scales the
recording's mel power where the per-clip call scales the samples, so it is held to the fp64 oracle by the suite's bound
(``mfcc_cases.check_clip``: max|gpu - fp64| <= max(4 e32, 2e-6 max|mfcc block|) per clip and block; the worst
error/bound ratio per block is printed before it is asserted).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import batchnorm_golden as G
from tests import mfcc_cases as M
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import MFCCFrontend, _lib, features, head, mfcc_features, mfcc_stream_features
    from kws_amd.fastgrnn_cuda import _get_raw_stream
DEV = torch.device("cuda:0")
TYPES = {0: "mfcc", 1: "delta", 2: "delta_delta"}
CANARY = -7.25e11


def _dev(rec, dtype=None):
    """A recording on the device one element into a larger buffer (no alignment beyond the element's)."""
    rec = np.asarray(rec)
    if dtype == torch.float32:
        rec = M.as_samples(rec)
    buf = torch.from_numpy(np.concatenate([rec[:1], rec, rec[:3]])).to(DEV)
    return buf[1:1 + len(rec)]


def _settings(n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, mean=None, std=None, peak=False):
    return dict(n_mfcc=n_mfcc, feature_type=TYPES[order], width=width, max_len=max_len, top_db=top_db, mean=mean, std=std,
                peak_normalize=peak)


def _both(rec, hop, **kw):
    got = mfcc_stream_features(rec, hop, **_settings(**kw))
    want = mfcc_features(MFCCFrontend.clips_of(rec, hop), **_settings(**kw))
    torch.cuda.synchronize()
    return got, want


# ---- 1. peak off: bit-equal to the per-clip call -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.int16, torch.float32))
@pytest.mark.parametrize("hop", (160, 800, 1600, 16000))
def test_bit_equal_to_the_per_clip_call(hop, dtype):
    rec = _dev(S.recordings()["mixed"], dtype)
    got, want = _both(rec, hop)
    assert got.shape == want.shape == ((48000 - 16000) // hop + 1, 99, 64)
    assert torch.equal(got, want)


@pytest.mark.parametrize("N", (16000, 16001, 16159, 16160, 32327, 48000))
def test_bit_equal_at_every_recording_length(N):
    """At hop 160 the clips consume every global frame from 2 to N / 160 - 2: every seam between the frames kernel's
    segments is crossed, wherever they lie, and the last clip ends in the recording's last whole hop."""
    rec = _dev(S.recordings()["mixed"][:N])
    for hop in (160, 800):
        got, want = _both(rec, hop, order=2)
        assert got.shape[0] == (N - 16000) // hop + 1 and torch.equal(got, want), hop


@pytest.mark.parametrize("kw", (
    dict(order=0, n_mfcc=13, width=3), dict(order=1, n_mfcc=64, width=15), dict(order=2, n_mfcc=32, width=9),
    dict(order=2, n_mfcc=13, width=15, top_db=-1.0), dict(order=1, n_mfcc=32, width=3, max_len=101),
    dict(order=0, n_mfcc=64, width=9, max_len=7), dict(order=2, n_mfcc=64, width=3, max_len=130, top_db=-1.0)),
    ids=lambda kw: "-".join("%s%s" % (k[0], v) for k, v in kw.items()))
@pytest.mark.parametrize("norm", (False, True))
def test_bit_equal_for_every_setting(kw, norm):
    F = kw["n_mfcc"] * (kw["order"] + 1)
    mean = std = None
    if norm:
        rng = np.random.default_rng(5)
        mean = torch.from_numpy((rng.standard_normal(F) * 20).astype(np.float32)).to(DEV)
        std = torch.from_numpy(rng.uniform(0.5, 30.0, F).astype(np.float32)).to(DEV)
    got, want = _both(_dev(S.recordings()["speech"]), 800, mean=mean, std=std, **kw)
    assert got.shape == (41, kw.get("max_len", 99), F) and torch.equal(got, want)


@pytest.mark.parametrize("hop", (160, 800))
def test_bit_equal_on_the_content_edges(hop):
    """A tone cut to digital silence, a lone impulse in the last sample of a silent second, silence, DC: the top_db
    floor and the 1e-10 floor both act, and whole clips are silent.  Bit-equality needs no bound."""
    rec = _dev(S.hostile())
    for top_db in (80.0, -1.0):
        got, want = _both(rec, hop, order=2, top_db=top_db)
        assert torch.isfinite(got).all() and torch.equal(got, want), top_db


# ---- 2. peak on: the fp64 oracle ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(name, b, order, width):
    rec = S.recordings()[name]
    return M.oracle_pair(rec[800 * b:800 * b + 16000], 99, n_mfcc=32, order=order, width=width, peak=True)


@pytest.mark.parametrize("order,width", ((1, 9), (2, 3)))
@pytest.mark.parametrize("name", ("mixed", "faint", "speech"))
def test_peak_normalised_clips_hold_the_oracles_bound(name, order, width):
    rec = S.recordings()[name]
    got = mfcc_stream_features(_dev(rec), 800, **_settings(order=order, width=width, peak=True)).cpu().numpy()
    worst = [0.0] * (order + 1)
    assert got.shape[0] == S.n_clips(len(rec), 800)
    for b in range(got.shape[0]):
        r64, r32 = _oracle(name, b, order, width)
        r = M.check_clip(got[b], r64, r32, 32, order, what="%s clip %d" % (name, b))
        worst = [max(a, c) for a, c in zip(worst, r)]
    print("streamed, peak on, %s o%d w%d: worst error/bound per block %s" % (name, order, width, ["%.3f" % w for w in worst]))


def test_a_silent_clip_between_loud_ones_is_the_per_clip_calls():
    rec = _dev(S.with_a_silent_clip())
    got, want = _both(rec, 800, peak=True)
    assert float(rec[16000:32000].abs().max()) == 0.0
    assert torch.isfinite(got).all() and torch.equal(got[20], want[20])            # m == 0: unscaled, as the per-clip call
    assert not torch.equal(got[19], got[20]) and not torch.equal(got[21], got[20])


# ---- 3. a clip's rows depend on its own samples only -------------------------------------------------------------------------
@pytest.mark.parametrize("peak", (False, True))
def test_nothing_outside_a_clip_reaches_its_rows(peak):
    clean = M.as_samples(S.recordings()["mixed"])
    for hop, b in ((800, 7), (800, 0), (800, 40), (160, 101)):
        dirty = np.full_like(clean, np.nan)
        dirty[hop * b:hop * b + 16000] = clean[hop * b:hop * b + 16000]
        want = mfcc_stream_features(_dev(clean), hop, **_settings(peak=peak))[b]
        got = mfcc_stream_features(_dev(dirty), hop, clip0=b, num_clips=1, **_settings(peak=peak))[0]
        assert torch.isfinite(got).all() and torch.equal(got, want), (hop, b)


# ---- 4. clip0 / B, the buffers' edges ----------------------------------------------------------------------------------------
def _raw_frames(desc, rec, ws, nbytes):
    st = _lib.load().fastgrnn_hip_mfcc_stream_frames(C.byref(desc), rec.data_ptr(), features.mfcc_tables(DEV).data_ptr(),
                                                     ws.data_ptr(), nbytes, _get_raw_stream(torch.cuda.current_device()))
    assert st == 0


def _raw_clips(desc, rec, ws, nbytes, out):
    st = _lib.load().fastgrnn_hip_mfcc_stream_clips(C.byref(desc), rec.data_ptr(), features.mfcc_tables(DEV).data_ptr(),
                                                    ws.data_ptr(), nbytes, None, None, out.data_ptr(),
                                                    _get_raw_stream(torch.cuda.current_device()))
    assert st == 0


@pytest.mark.parametrize("peak", (0, 1))
def test_chunks_concatenate_and_every_buffer_keeps_its_edges(peak):
    rec = _dev(S.recordings()["faint"])
    N, B, T, F = 32000, 21, 99, 96
    whole = mfcc_stream_features(rec, 800, **_settings(order=2, peak=bool(peak)))
    desc = lambda clip0, n: _lib.MfccStreamDesc(N, 800, 1, clip0, n, 32, 2, 9, T, 80.0, peak)
    nbytes = _lib.load().fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(desc(0, B)))
    assert nbytes % 4 == 0
    ws_big = torch.full((nbytes // 4 + 2 * 4096,), CANARY, device=DEV)
    ws = ws_big[4096:4096 + nbytes // 4]
    assert ws.data_ptr() % 256 == 0
    _raw_frames(desc(0, B), rec, ws, nbytes)
    torch.cuda.synchronize()
    assert (ws_big[:4096] == CANARY).all() and (ws_big[-4096:] == CANARY).all()
    frames = ws.clone()
    out_big = torch.full(((B + 2) * T * F,), float("nan"), device=DEV)
    out_big[:T * F] = CANARY
    out_big[-T * F:] = CANARY
    body = out_big[T * F:-T * F].view(B, T, F)
    for clip0, n in ((0, 1), (1, 7), (8, B - 8)):
        assert torch.isnan(body[clip0:]).all()                                   # rows of the clips to come: untouched
        _raw_clips(desc(clip0, n), rec, ws, nbytes, body[clip0])
        torch.cuda.synchronize()
        assert not torch.isnan(body[:clip0 + n]).any()                           # every element of the chunk is written
    assert (out_big[:T * F] == CANARY).all() and (out_big[-T * F:] == CANARY).all()
    assert torch.equal(body, whole)
    assert torch.equal(ws, frames)                                               # the clips call only reads the workspace
    # the shim's chunks: the frames of the first call serve the later ones
    first, fr = mfcc_stream_features(rec, 800, num_clips=1, return_frames=True, **_settings(order=2, peak=bool(peak)))
    rest = mfcc_stream_features(rec, 800, clip0=1, frames=fr, **_settings(order=2, peak=bool(peak)))
    assert torch.equal(torch.cat([first, rest]), whole)


# ---- 5. many clips -----------------------------------------------------------------------------------------------------------
def test_many_clips_in_one_call():
    rec = _dev(np.tile(S.recordings()["mixed"], 20))                              # 60 s: 1181 clips at hop 800
    got, want = _both(rec, 800)
    assert got.shape[0] == 1181 and torch.equal(got, want)
    # (period 48 000 samples = 60 hops: clip b + 60 reads the same samples as clip b)
    assert torch.equal(got[60:1140], got[:1080])


# ---- 6. repeatability and capture --------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_and_a_graph_replays_on_a_new_recording():
    r0 = torch.from_numpy(S.recordings()["mixed"]).to(DEV)
    r1 = torch.from_numpy(np.ascontiguousarray(S.recordings()["mixed"][::-1])).to(DEV)
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"], std=fx["std"], peak_normalize=True, device=DEV)
    want0, again, want1 = fe.stream(r0), fe.stream(r0), fe.stream(r1)
    assert torch.equal(want0, again) and not torch.equal(want0, want1)
    buf = r0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fe.stream(buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe.stream(buf)                                                     # both calls, one graph
    for r, want in ((r1, want1), (r0, want0)):
        buf.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_stream_is_forward_of_the_clips():
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"], std=fx["std"], device=DEV)
    rec = _dev(S.recordings()["mixed"])
    assert torch.equal(fe.stream(rec), fe(MFCCFrontend.clips_of(rec)))
    assert torch.equal(fe.stream(rec, 1600, normalize=False), fe(MFCCFrontend.clips_of(rec, 1600), normalize=False))
    for bad in (dict(hop_samples=801), dict(hop_samples=400), dict(clip=8000)):
        with pytest.raises(ValueError):
            fe.stream(rec, **bad)


# ---- 7. the live loop --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter():
    d, full = G.trained_state_dict()
    m = G.build_model(DEV, batch_first=True)
    m.load_state_dict(full)
    m.eval()
    fx = M.fixture()
    return m, MFCCFrontend(mean=fx["mean"], std=fx["std"], device=DEV), fx


def test_detect_audio_with_shared_frames_is_the_composition(spotter):
    m, fe, fx = spotter
    rec = torch.from_numpy(M.recording(33, 3.0, fx["pcm"], 20000)).to(DEV)
    pred, maj, event = m.detect_audio(rec, fe, num_windows=10, majority=5, shared_frames=True)
    B = (48000 - 16000) // 800 + 1
    assert pred.shape == maj.shape == event.shape == (1, B)
    assert not fe.peak_normalize                                   # (left as it was)
    fe.peak_normalize = True
    try:
        feats = fe.stream(rec)
    finally:
        fe.peak_normalize = False
    assert feats.shape == (B, 99, 64)
    m.init_hidden()
    p2, _ = m.predict(feats)
    m.init_hidden()
    maj2, ev2 = head.vote_windows(p2.reshape(1, B), 10, 5)
    assert torch.equal(pred.reshape(-1), p2) and torch.equal(maj, maj2) and torch.equal(event, ev2)
    assert (pred == 0).any() and (event == 0).any()                # "down" is in there and gets reported
    assert m.hidden_states == [None] * 3


def test_detect_audio_without_shared_frames_is_unchanged_and_nothing_falls_back(spotter):
    m, fe, fx = spotter
    rec = torch.from_numpy(M.recording(33, 3.0, fx["pcm"], 20000)).to(DEV)
    a = m.detect_audio(rec, fe, num_windows=10, majority=5)
    b = m.detect_audio(rec, fe, num_windows=10, majority=5, shared_frames=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for bad in (dict(hop_samples=400), dict(hop_samples=801), dict(clip=8000)):
        with pytest.raises(ValueError, match="streamed front end"):
            m.detect_audio(rec, fe, shared_frames=True, **bad)
        assert not fe.peak_normalize
        m.detect_audio(rec, fe, **bad)                             # (the per-clip path takes them)
