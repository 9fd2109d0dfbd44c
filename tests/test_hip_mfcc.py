"""The MFCC front end on the GPU against the fp64 oracle of tests/mfcc_cases.py.

Bound, for every clip and block (mfcc, delta, delta2):  max|gpu - fp64| <= max(4 e32, 2e-6 max|mfcc block|), e32 the
fp32 oracle's own error on that clip and block (``mfcc_cases.check_clip``; every test prints its worst error/bound
ratio per block before it asserts).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import batchnorm_golden as G
from tests import mfcc_cases as M

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import MFCCFrontend, _lib, fastgrnn_cuda, features, head, mfcc_features
    from kws_amd.fastgrnn_cuda import _get_raw_stream
DEV = torch.device("cuda:0")
TYPES = {0: "mfcc", 1: "delta", 2: "delta_delta"}


@functools.lru_cache(maxsize=None)
def _signals():
    fx = M.fixture()
    return {"s0": M.speech_like(10), "s1": M.speech_like(11), "s2": M.speech_like(12), "wav": fx["pcm"],
            "noise": M.noise(3), "silence": M.silence(), "dc": M.dc(), "imp0": M.impulse(0), "imp_last": M.impulse(15999),
            "tone_sil": M.tone_then_silence(), "wav_half": fx["pcm"][:8000].copy()}


@functools.lru_cache(maxsize=None)
def _oracle(name, length, n_mfcc, order, width, max_len, top_db, peak):
    y = _signals()[name][:length]
    return M.oracle_pair(y, max_len, n_mfcc=n_mfcc, order=order, width=width, top_db=top_db, peak=peak)


def _gpu(audio, lengths=None, *, n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, mean=None, std=None, peak=False):
    lengths = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    mean = None if mean is None else torch.as_tensor(mean, dtype=torch.float32, device=DEV)
    std = None if std is None else torch.as_tensor(std, dtype=torch.float32, device=DEV)
    out = mfcc_features(audio, lengths, n_mfcc=n_mfcc, feature_type=TYPES[order], width=width, max_len=max_len,
                        top_db=top_db, mean=mean, std=std, peak_normalize=peak)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, names, lengths=None, *, n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, mean=None, std=None,
           peak=False, what=""):
    worst = [0.0] * (order + 1)
    assert got.shape == (len(names), max_len, n_mfcc * (order + 1))
    for b, name in enumerate(names):
        length = len(_signals()[name]) if lengths is None else lengths[b]
        r64, r32 = _oracle(name, length, n_mfcc, order, width, max_len, top_db, peak)
        r = M.check_clip(got[b], r64, r32, n_mfcc, order, mean, std, "%s clip %d (%s, len %d)" % (what, b, name, length))
        worst = [max(a, c) for a, c in zip(worst, r)]
    print("%s: worst error/bound per block %s" % (what, ["%.3f" % w for w in worst]))
    return worst


def _raw(desc, audio, lengths, out, out_offset):
    """The C entry point itself, writing at element ``out_offset`` of the float32 tensor ``out``."""
    st = _lib.load().fastgrnn_hip_mfcc(C.byref(desc), audio.data_ptr(), lengths.data_ptr(),
                                       features.mfcc_tables(DEV).data_ptr(), None, None, out.data_ptr() + 4 * out_offset,
                                       None, 0, _get_raw_stream(torch.cuda.current_device()))
    assert st == 0
    torch.cuda.synchronize()


def _batch(names, dtype=torch.float32):
    return torch.from_numpy(np.stack([M.as_samples(_signals()[n]) if dtype == torch.float32 else _signals()[n]
                                      for n in names])).to(DEV)


# ---- 1. tables -------------------------------------------------------------------------------------------------------
def test_tables_match_the_oracles_to_one_ulp():
    got = M.split_tables(features.mfcc_tables(DEV).cpu().numpy())
    want = M.tables()
    for name in ("cos", "sin", "mel", "dct", "taps"):
        g, w = got[name], want[name]
        assert g.shape == w.shape
        ulp = np.spacing(np.abs(w).astype(np.float32))
        # (an entry that is an exact zero in one and 1e-17 in the other rounds to different tiny floats: below
        # 2^-24 of the table's largest entry the comparison is absolute)
        ok = (np.abs(g - w) <= ulp) | (np.abs(g - w) <= 2.0 ** -24 * np.abs(w).max() * 2.0 ** -23)
        assert ok.all(), (name, int((~ok).sum()), float(np.abs(g - w).max()))
    assert (got["cos"][:, 201:] == 0).all() and (got["sin"][:, 201:] == 0).all() and (got["mel"][201:] == 0).all()


# ---- 2. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (0, 1, 2))
@pytest.mark.parametrize("n_mfcc,width", ((32, 9), (13, 3)))
def test_parity_fp32(order, n_mfcc, width):
    names = ["s0", "s1", "s2"]
    got = _gpu(_batch(names), n_mfcc=n_mfcc, order=order, width=width)
    _check(got, names, n_mfcc=n_mfcc, order=order, width=width, what="parity fp32 o%d c%d w%d" % (order, n_mfcc, width))


@pytest.mark.parametrize("order", (0, 1, 2))
def test_parity_int16_fixture_clip(order):
    got = _gpu(_batch(["wav"], torch.int16), order=order)
    _check(got, ["wav"], order=order, what="parity int16 o%d" % order)


@pytest.mark.parametrize("order,n_mfcc", ((1, 32), (2, 13)))
def test_parity_normalised(order, n_mfcc):
    rng = np.random.default_rng(5)
    F = n_mfcc * (order + 1)
    mean = (rng.standard_normal(F) * 20).astype(np.float32)
    std = rng.uniform(0.5, 30.0, F).astype(np.float32)
    if F == 64:
        fx = M.fixture()
        mean, std = fx["mean"], fx["std"]
    names = ["s0", "wav_half", "s2"]
    a = _batch(["s0", "s2"])
    audio = torch.zeros(3, 16000, device=DEV)
    audio[0], audio[2] = a[0], a[1]
    audio[1, :8000] = torch.from_numpy(M.as_samples(_signals()["wav_half"])).to(DEV)
    lengths = [16000, 8000, 16000]
    got = _gpu(audio, lengths, n_mfcc=n_mfcc, order=order, mean=mean, std=std)
    _check(got, names, lengths, n_mfcc=n_mfcc, order=order, mean=mean, std=std, what="normalised o%d c%d" % (order, n_mfcc))
    # padded frames of the short clip are exactly -mean/std
    pad = got[1, 60:]
    want = (-mean.astype(np.float64) / std.astype(np.float64))[None, :]
    assert np.abs(pad - want).max() <= 2.0 ** -22 * np.abs(want).max()


# ---- 3. lengths ------------------------------------------------------------------------------------------------------
def test_lengths_in_one_call():
    lengths = [1280, 1281, 1439, 1440, 8000, 16000]
    names = ["s0", "s1", "noise", "s2", "wav", "s1"]
    audio = _batch(["s0", "s1", "noise", "s2", "s0", "s1"])
    audio[4] = torch.from_numpy(M.as_samples(_signals()["wav"])).to(DEV)
    audio = audio.clone()
    for b, n in enumerate(lengths):                       # what lies past a clip's length must not matter
        audio[b, n:] = 1e6
    got = _gpu(audio, lengths, order=2)
    _check(got, names, lengths, order=2, what="lengths")
    for b, n in enumerate(lengths):
        assert (got[b, M.n_frames(n):] == 0).all()


def test_out_of_range_lengths_are_clamped_and_neighbours_untouched():
    names = ["s0", "s1", "s2", "noise", "wav_half"]
    L = 8000
    audio = torch.from_numpy(np.stack([M.as_samples(_signals()[n])[:L] for n in names])).to(DEV)
    good = [L, 4000, L, 1280, L]
    bad = [0, 4000, L + 7, -1, L]
    outs = [_gpu(audio, lens) for lens in (good, bad)]
    # rows with in-range lengths do not depend on their neighbours' lengths, bit for bit
    for b in (1, 4):
        assert np.array_equal(outs[0][b], outs[1][b])
    # 0 and -1 behave as 1280, L + 7 as L
    ref = _gpu(audio, [1280, 4000, L, 1280, L])
    assert np.array_equal(outs[1], ref)
    _check(ref, names, [1280, 4000, L, 1280, L], what="clamped lengths")


def test_out_of_range_lengths_stay_inside_the_buffers():
    """Audio and output sit inside canary-filled allocations; lengths far out of range neither change the canaries of
    the output nor read anything but the clips (the canaries of the audio are NaN: one sample read would poison a row)."""
    L, B, T, F = 1600, 4, 12, 64
    big = torch.full((B * L + 2 * 4096,), float("nan"), device=DEV)
    audio = big[4096:4096 + B * L].view(B, L)
    audio.copy_(torch.from_numpy(np.stack([M.as_samples(_signals()[n])[:L] for n in ("s0", "s1", "s2", "noise")])))
    out_big = torch.full((B * T * F + 2 * 4096,), -7.25e11, device=DEV)
    lens = torch.tensor([2 ** 31 - 1, -2 ** 31, L + 1, 1279], dtype=torch.int32, device=DEV)
    _raw(_lib.MfccDesc(B, L, L, 0, 32, 1, 9, T, 80.0, 0), audio, lens, out_big, 4096)
    got = out_big[4096:4096 + B * T * F].view(B, T, F)
    assert torch.isfinite(got).all()
    assert (out_big[:4096] == -7.25e11).all() and (out_big[-4096:] == -7.25e11).all()
    ref = mfcc_features(audio, torch.tensor([L, 1280, L, 1280], dtype=torch.int32, device=DEV), max_len=T)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("L", (1280, 15999))
def test_tensor_widths(L):
    names = ["s0", "wav"]
    audio = torch.from_numpy(np.stack([M.as_samples(_signals()[n])[:L] for n in names])).to(DEV)
    got = _gpu(audio, order=2)
    _check(got, names, [L, L], order=2, what="L=%d" % L)


# ---- 4. content edges ------------------------------------------------------------------------------------------------
def test_content_edges():
    names = ["silence", "dc", "imp0", "imp_last", "tone_sil"]
    got = _gpu(_batch(names), order=2)
    _check(got, names, order=2, what="content edges")
    for b, name in enumerate(names):                      # which clip carries the worst ratio
        _check(got[b:b + 1], [name], order=2, what="content edge " + name)


def test_peak_normalize():
    pcm = torch.from_numpy(np.stack([_signals()["wav"], np.zeros(16000, dtype=np.int16)])).to(DEV)
    got = _gpu(pcm, order=1, peak=True)
    _check(got, ["wav", "silence"], order=1, peak=True, what="peak int16")
    got = _gpu(_batch(["s1", "silence"]), order=2, peak=True)
    _check(got, ["s1", "silence"], order=2, peak=True, what="peak fp32")


def test_no_top_db():
    names = ["tone_sil", "s0"]
    for top in (-1.0, None):
        got = _gpu(_batch(names), order=1, top_db=top)
        _check(got, names, order=1, top_db=-1.0, what="top_db %s" % top)
    assert not np.array_equal(got, _gpu(_batch(names), order=1))


def test_max_len_cuts_after_the_delta_and_pads():
    # n = 101 cut to 99: frames 97, 98 are interior frames of the 101, not edge copies
    got = _gpu(_batch(["s0"]), order=2, max_len=99)
    _check(got, ["s0"], order=2, max_len=99, what="cut 101 -> 99")
    full = _gpu(_batch(["s0"]), order=2, max_len=101)
    assert np.array_equal(full[:, :99], got)
    # (h = 4: frames 97..100 of the 101 copy frame 96; a delta taken after the cut would copy frame 94 from 95 on)
    assert np.array_equal(got[0, 98, 32:], got[0, 96, 32:]) and not np.array_equal(got[0, 95, 32:64], got[0, 96, 32:64])
    # n = 51 padded to 99
    audio = _batch(["wav"])
    got = _gpu(audio, [8000], order=2)
    _check(got, ["wav"], [8000], order=2, what="pad 51 -> 99")
    assert (got[0, 51:] == 0).all() and (got[0, 50] != 0).any()
    got = _gpu(audio, order=1, max_len=1)
    _check(got, ["wav"], order=1, max_len=1, what="max_len 1")
    got = _gpu(audio, order=1, max_len=130)
    _check(got, ["wav"], order=1, max_len=130, what="max_len 130")


# ---- 5. overlap and alignment ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.int16, torch.float32))
@pytest.mark.parametrize("offset", (0, 1))
def test_overlapping_clips_of_a_recording(dtype, offset):
    rec = M.recording(21, 2.0, M.fixture()["pcm"], 9000)
    if offset:
        rec = np.concatenate([rec[:1], rec])                      # the recording starts one element into its buffer
    buf = torch.from_numpy(rec if dtype == torch.int16 else M.as_samples(rec)).to(DEV)
    view = MFCCFrontend.clips_of(buf[offset:])
    assert view.shape == (21, 16000) and view.stride() == (800, 1)
    assert view.data_ptr() + view.element_size() * (20 * 800 + 16000) == buf.data_ptr() + buf.element_size() * buf.numel()
    got = _gpu(view, order=1)
    worst = [0.0, 0.0]
    for b in range(21):
        y = rec[offset + 800 * b: offset + 800 * b + 16000]
        r64, r32 = M.oracle_pair(y, 99, n_mfcc=32, order=1, width=9)
        r = M.check_clip(got[b], r64, r32, 32, 1, what="overlap clip %d" % b)
        worst = [max(a, c) for a, c in zip(worst, r)]
    print("overlap %s offset %d: worst error/bound per block %s" % (dtype, offset, ["%.3f" % w for w in worst]))
    assert np.array_equal(got, _gpu(view.contiguous(), order=1))


# ---- 6. many clips ---------------------------------------------------------------------------------------------------
def test_many_clips():
    names = ["s0", "s1", "s2", "wav", "noise", "tone_sil", "dc", "silence"]
    B = 1030
    audio = _batch(names)[torch.arange(B, device=DEV) % 8].contiguous()
    got = _gpu(audio, order=1)
    _check(got[:8], names, order=1, what="many clips")
    assert np.array_equal(got, got[:8][np.arange(B) % 8])


# ---- 7. output writes ------------------------------------------------------------------------------------------------
def test_every_output_element_is_written_once_and_nothing_else():
    B, T, F = 3, 99, 96
    audio = _batch(["s0", "s1", "s2"])
    buf = torch.full(((B + 2) * T * F,), float("nan"), device=DEV)
    buf[:T * F] = -7.25e11
    buf[-T * F:] = -7.25e11
    lens = torch.tensor([16000, 8000, 1280], dtype=torch.int32, device=DEV)
    _raw(_lib.MfccDesc(B, 16000, 16000, 0, 32, 2, 9, T, 80.0, 0), audio, lens, buf, T * F)
    assert (buf[:T * F] == -7.25e11).all() and (buf[-T * F:] == -7.25e11).all()
    body = buf[T * F:-T * F]
    assert not torch.isnan(body).any()
    assert torch.equal(body.view(B, T, F), mfcc_features(audio, lens, feature_type="delta_delta"))


# ---- 8. repeatability ------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_and_a_graph_replays_on_new_audio():
    a0, a1 = _batch(["s0", "wav", "s1"]), _batch(["s2", "noise", "tone_sil"])
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"], std=fx["std"], peak_normalize=True, device=DEV)
    want0, again, want1 = fe(a0), fe(a0), fe(a1)
    assert torch.equal(want0, again) and not torch.equal(want0, want1)
    buf = a0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fe(buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fe(buf)
    for a, want in ((a1, want1), (a0, want0)):
        buf.copy_(a)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


# ---- 9. the live loop ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter():
    d, full = G.trained_state_dict()
    m = G.build_model(DEV, batch_first=True)
    m.load_state_dict(full)
    m.eval()
    fx = M.fixture()
    return m, MFCCFrontend(mean=fx["mean"], std=fx["std"], device=DEV), fx


def test_the_shipped_model_hears_down_on_the_gpu(spotter):
    m, fe, fx = spotter
    pcm = torch.from_numpy(fx["pcm"]).to(DEV)
    pred, maj, event = m.detect_audio(pcm, fe, num_windows=1, majority=1)
    assert pred.shape == (1, 1) and pred.dtype == torch.int32
    assert int(pred[0, 0]) == 0 and int(maj[0, 0]) == 0 and int(event[0, 0]) == 0 and fx["classes"][0] == "down"
    fe.peak_normalize = True
    try:
        feats = fe(pcm[None])
    finally:
        fe.peak_normalize = False
    p2, logp = m.predict(feats)
    m.init_hidden()
    assert int(p2[0]) == 0 and float(logp[0, 0]) > -1e-2
    r64, r32 = M.oracle_pair(fx["pcm"], 99, n_mfcc=32, order=1, width=9, peak=True)
    M.check_clip(feats[0].cpu().numpy(), r64, r32, 32, 1, fx["mean"], fx["std"], "fixture clip, normalised")


def test_detect_audio_is_the_composition(spotter):
    m, fe, fx = spotter
    rec = torch.from_numpy(M.recording(33, 3.0, fx["pcm"], 20000)).to(DEV)
    pred, maj, event = m.detect_audio(rec, fe, num_windows=10, majority=5)
    B = (48000 - 16000) // 800 + 1
    assert pred.shape == maj.shape == event.shape == (1, B)
    assert not fe.peak_normalize                                   # (left as it was)
    fe.peak_normalize = True
    try:
        feats = fe(MFCCFrontend.clips_of(rec))
    finally:
        fe.peak_normalize = False
    assert feats.shape == (B, 99, 64)
    m.init_hidden()
    p2, _ = m.predict(feats)                                       # batch_first model: [B,T,F], a zero state per clip
    m.init_hidden()
    maj2, ev2 = head.vote_windows(p2.reshape(1, B), 10, 5)
    assert torch.equal(pred.reshape(-1), p2) and torch.equal(maj, maj2) and torch.equal(event, ev2)
    assert (pred == 0).any() and (event == 0).any()                # "down" is in there and gets reported
    assert m.hidden_states == [None] * 3


def test_layer_zero_reads_the_pool_in_place_where_the_windowed_scans_hold_it(spotter):
    m, fe, fx = spotter
    rec = torch.from_numpy(M.recording(34, 1.5, fx["pcm"][:8000], 3000)).to(DEV)
    feats = fe(MFCCFrontend.clips_of(rec))
    B, T, F = feats.shape
    l0 = m.rnn_list[0]
    flags = _lib.FLAG_BATCH_MAJOR | _lib.FLAG_PREACT_AFFINE
    served = fastgrnn_cuda.windows_supported(T, B, F, 256, 0, 0, l0.cell._gate_code, l0.cell._update_code, torch.float32, flags)
    starts = torch.arange(B, device=DEV) * T
    with torch.no_grad():
        in_place = l0.forward_windows(feats.view(B * T, F), starts, T)
        gathered = l0(feats, hiddenState=None, training=False)
    print("forward_windows serves layer 0 of the shipped model: %s" % bool(served))
    assert torch.equal(in_place, gathered)                         # (not served: forward_windows gathers, the same call)
