"""Device-side augmentation on the GPU.  The central check has no tolerance: the fused call -- the featuriser reading the
audio bank through records -- equals the unfused chain, ``AudioAugment.apply`` followed by the plain featuriser, bit for
bit, and the materialised audio equals the numpy oracle of tests/augment_cases.py bit for bit.

Shapes: a bank of N = 11 clips of L = 16 000 samples with lengths that include 1280, 1281, 15 999 and 16 000; B = 37
output clips; noises of 1, 7, 4000 and 20 001 samples."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import augment_cases as A
from tests import mfcc_cases as M
from tests import support as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from kws_amd import (AudioAugment, FusedAdam, GraphedStep, MFCCFrontend, RNNClassifierModel, _lib, features,
                         mfcc_features, pack_augment)
    from kws_amd.fastgrnn_cuda import _get_raw_stream
DEV = torch.device("cuda:0")
TYPES = {0: "mfcc", 1: "delta", 2: "delta_delta"}
N, L, B = 11, 16000, 37
LENGTHS = np.array([1280, 1281, 15999, 16000, 8000, 12345, 16000, 1440, 9999, 3000, 15840], dtype=np.int32)
NLEN = np.array([1, 7, 4000, 20001], dtype=np.int32)
NMAX = 20001
CANARY = -7.25e11


@functools.lru_cache(maxsize=None)
def _host(dtype):
    """(bank [N+2, L] with a guard clip on either side, noises) on the host: float32 samples or int16 PCM."""
    rng = np.random.default_rng(21)
    clips = [M.speech_like(30 + c) if c % 2 else M.noise(40 + c, amp=0.2) for c in range(N + 2)]
    noises = [np.array([0.25], dtype=np.float32), (0.3 * rng.standard_normal(7)).astype(np.float32),
              M.noise(50, 4000, 0.2), M.noise(51, 20001, 0.05)]
    bank = np.stack(clips).astype(np.float32)
    if dtype == "i16":
        to_pcm = lambda y: np.clip(np.round(y * 20000.0), -32768, 32767).astype(np.int16)
        return to_pcm(bank), [to_pcm(z) for z in noises]
    return bank, noises


@functools.lru_cache(maxsize=None)
def _device(dtype):
    """(bank view [N, L] between its guard clips, lengths, an AudioAugment whose noise bank lies between guard rows)."""
    bank, noises = _host(dtype)
    whole = torch.from_numpy(bank).to(DEV)
    aug = AudioAugment(p_augment=1.0, max_shift=4000, gain=(-1.0, 1.5), p_noise=0.6, noise_gain=(0.05, 0.5),
                       seed=(0xC0FFEE << 32) | 0x1234, noises=[torch.from_numpy(z) for z in noises], device=DEV)
    guarded = torch.zeros((len(noises) + 2, NMAX), dtype=whole.dtype, device=DEV)
    guarded[1:-1] = aug.noise
    aug.noise = guarded[1:-1]
    return whole[1:N + 1], torch.from_numpy(LENGTHS).to(DEV), aug


def _edge_records():
    """Hand-made edges, all in range: shifts around a clip's length, gains 0 and negative, noises that wrap thousands
    of times, noise_off = nlen - 1, a repeated src."""
    rows = []
    for src in (1, 2):                                               # len 1281 and 15 999
        n = int(LENGTHS[src])
        for s in (1, -1, n - 1, -(n - 1), n, -n, n + 5, -(n + 5)):
            rows.append((src, s, 1.0, len(rows) % 4, 3 if len(rows) % 4 else 0, 0.3))
    rows += [(3, 0, 0.0, 2, 0, 0.1), (3, 0, -0.5, -1, 0, 0.0), (3, 100, 0.0, -1, 0, 0.0), (0, 17, 1.0, 0, 0, 0.5),
             (6, -3, 1.0, 1, 6, 0.5), (6, 0, 1.0, 2, 3999, 0.1), (6, 0, 1.0, 3, 20000, 1.0), (6, 0, 1.0, 3, 0, 0.1)]
    a = np.asarray(rows, dtype=np.float64)
    return A.pack(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5])


@functools.lru_cache(maxsize=None)
def _records():
    edges = _edge_records()
    idx = np.random.default_rng(2).integers(0, N, B - len(edges))
    drawn = A.draw(77, 3, idx, p_augment=0.9, max_shift=4000, gain=(-1.0, 1.5), p_noise=0.6, noise_gain=(0.05, 0.5),
                   noise_lengths=NLEN, noise_len_max=NMAX)
    rec = np.concatenate([edges, drawn])
    assert rec.shape == (B, 6)
    return rec


def _fused(bank, lengths, rec, aug, *, n_mfcc=32, order=1, width=9, peak=False, mean=None, std=None, check=True):
    return mfcc_features(bank, lengths, n_mfcc=n_mfcc, feature_type=TYPES[order], width=width, peak_normalize=peak,
                         mean=mean, std=std, augment=rec, noise=aug.noise, noise_lengths=aug.noise_lengths, check=check)


def _unfused(bank, lengths, rec, aug, *, n_mfcc=32, order=1, width=9, peak=False, mean=None, std=None):
    audio = aug.apply(bank, lengths, rec)
    src = rec[:, 0].clamp(0, bank.shape[0] - 1).long()
    return audio, mfcc_features(audio, lengths[src].contiguous(), n_mfcc=n_mfcc, feature_type=TYPES[order], width=width,
                                peak_normalize=peak, mean=mean, std=std)


# ---- 1. identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "i16"))
def test_identity_records_reproduce_the_plain_call(dtype):
    bank, lengths, aug = _device(dtype)
    rec = pack_augment(torch.arange(N, device=DEV), 0, 1.0)
    want = mfcc_features(bank, lengths)
    assert S.bits_equal(_fused(bank, lengths, rec, aug), want)
    assert S.bits_equal(mfcc_features(bank, lengths, augment=rec), want)            # no noise bank at all
    assert S.bits_equal(mfcc_features(bank, None, augment=rec), mfcc_features(bank, None))


# ---- 2. fused == unfused, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cfg", (
    ("f32", dict()), ("i16", dict()), ("f32", dict(peak=True)), ("i16", dict(peak=True, norm=True)),
    ("f32", dict(norm=True)), ("f32", dict(n_mfcc=16, order=2, width=3))))
def test_the_fused_call_equals_the_unfused_chain(dtype, cfg):
    bank, lengths, aug = _device(dtype)
    cfg = dict(cfg)
    if cfg.pop("norm", False):
        fx = M.fixture()
        cfg.update(mean=torch.from_numpy(fx["mean"]).to(DEV), std=torch.from_numpy(fx["std"]).to(DEV))
    rec = torch.from_numpy(_records()).to(DEV)
    got = _fused(bank, lengths, rec, aug, **cfg)
    audio, want = _unfused(bank, lengths, rec, aug, **cfg)
    torch.cuda.synchronize()
    host_bank, host_noises = _host(dtype)
    oracle, olen = A.augment_batch(host_bank[1:N + 1], LENGTHS, _records(), host_noises)
    assert np.array_equal(audio.cpu().numpy().view(np.int32), oracle.view(np.int32))
    assert got.shape == (B, 99, cfg.get("n_mfcc", 32) * (cfg.get("order", 1) + 1)) and S.bits_equal(got, want)
    assert bool(torch.isfinite(got).all())
    # the edges did what they say: shift = len with gain 1 leaves the (one-sample) noise alone; gain 0, no noise: silence
    n1, z0 = int(LENGTHS[1]), A.as_samples(host_noises[0])[0]
    assert olen[4] == n1 and (oracle[4, :n1] == np.float32(0.3) * z0).all() and not oracle[4, n1:].any()
    assert not oracle[18].any() and oracle[17].any()


def test_a_bank_that_is_a_strided_view():
    """Overlapping bank clips of one recording (``clips_of``, clip_stride < L), int16."""
    rec_pcm = torch.from_numpy(M.recording(5, seconds=1.5, pcm=M.fixture()["pcm"], at=3000)).to(DEV)
    bank = MFCCFrontend.clips_of(rec_pcm, hop_samples=800, clip=L)              # [11, 16000], stride 800
    assert bank.shape == (N, L) and bank.stride() == (800, 1)
    _, lengths, aug = _device("i16")
    rec = torch.from_numpy(_records()).to(DEV)
    got = _fused(bank, lengths, rec, aug)
    audio, want = _unfused(bank, lengths, rec, aug)
    assert S.bits_equal(got, want)
    oracle, _ = A.augment_batch(bank.cpu().numpy(), LENGTHS, _records(), _host("i16")[1])
    assert np.array_equal(audio.cpu().numpy().view(np.int32), oracle.view(np.int32))


def test_an_absent_noise_reads_no_noise():
    bank, lengths, aug = _device("f32")
    poisoned = copy.deepcopy(aug)
    poisoned.noise = torch.full_like(aug.noise, float("nan"))
    rec = pack_augment(torch.arange(N, device=DEV), 5, 0.5, noise=-1, noise_off=3, noise_gain=2.0)
    got = _fused(bank, lengths, rec, poisoned)
    assert bool(torch.isfinite(got).all()) and S.bits_equal(got, mfcc_features(bank, lengths, augment=rec))


def test_the_range_check():
    bank, lengths, aug = _device("f32")
    good = pack_augment(torch.arange(3, device=DEV), 0, 1.0, noise=3, noise_off=20000, noise_gain=0.1)
    _fused(bank, lengths, good, aug)
    for bad in (pack_augment(torch.tensor([0, N], device=DEV), 0, 1.0), pack_augment(torch.tensor([-1], device=DEV), 0, 1.0),
                pack_augment(torch.tensor([0], device=DEV), 0, 1.0, noise=4, noise_gain=0.1),
                pack_augment(torch.tensor([0], device=DEV), 0, 1.0, noise=1, noise_off=7, noise_gain=0.1),
                pack_augment(torch.tensor([0], device=DEV), 0, 1.0, noise=1, noise_off=-1, noise_gain=0.1)):
        with pytest.raises(ValueError, match="range"):
            _fused(bank, lengths, bad, aug)
    with pytest.raises(ValueError, match="range"):                               # a noise index without a noise bank
        mfcc_features(bank, lengths, augment=pack_augment(torch.tensor([0], device=DEV), 0, 1.0, noise=0))


# ---- 3. records outside their ranges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "i16"))
def test_hostile_records_give_the_clamped_records_result_and_stay_inside(dtype):
    bank, lengths, aug = _device(dtype)
    hostile = A.hostile_records(N, len(NLEN))
    clamped = A.clamp_records(hostile, N, NLEN, NMAX)
    assert not np.array_equal(hostile, clamped)
    Bh, T, F = len(hostile), 99, 64
    rec = torch.from_numpy(hostile).to(DEV)
    out = torch.full((Bh + 2, T, F), CANARY, dtype=torch.float32, device=DEV)    # feats between two canary rows
    desc = _lib.MfccDesc(Bh, L, L, 0 if dtype == "f32" else 1, 32, 1, 9, T, 80.0, 0)
    bankd = _lib.MfccBank(N, len(NLEN), NMAX, NMAX, 0)
    st = _lib.load().fastgrnn_hip_mfcc_augment(
        C.byref(desc), C.byref(bankd), bank.data_ptr(), lengths.data_ptr(), aug.noise.data_ptr(),
        aug.noise_lengths.data_ptr(), rec.data_ptr(), features.mfcc_tables(DEV).data_ptr(), None, None,
        out.data_ptr() + 4 * T * F, None, 0, _get_raw_stream(torch.cuda.current_device()))
    assert st == 0
    torch.cuda.synchronize()
    assert bool((out[0] == CANARY).all()) and bool((out[-1] == CANARY).all())
    want = _fused(bank, lengths, torch.from_numpy(clamped).to(DEV), aug)          # (in range: check=True passes)
    assert S.bits_equal(out[1:-1], want)
    assert S.bits_equal(_fused(bank, lengths, rec, aug, check=False), want)
    audio, unfused = _unfused(bank, lengths, rec, aug)                            # apply clamps alike
    assert S.bits_equal(unfused, want)
    host_bank, host_noises = _host(dtype)
    oracle, _ = A.augment_batch(host_bank[1:N + 1], LENGTHS, clamped, host_noises)
    assert np.array_equal(audio.cpu().numpy().view(np.int32), oracle.view(np.int32))
    # without noises every noise index means none
    none = A.clamp_records(hostile, N, None, 1)
    assert S.bits_equal(mfcc_features(bank, lengths, augment=rec, check=False),
                      mfcc_features(bank, lengths, augment=torch.from_numpy(none).to(DEV)))


# ---- 4. the draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bd", (1, 37, 1030))
def test_the_draw_equals_the_numpy_draw(Bd):
    _, _, aug = _device("f32")
    step = (1 << 32) + 12345
    idx = np.random.default_rng(Bd).integers(0, N, Bd).astype(np.int32)
    got = aug.draw(torch.from_numpy(idx).to(DEV), torch.tensor([step], dtype=torch.int64, device=DEV))
    want = A.draw(aug.seed, step, idx, p_augment=aug.p_augment, max_shift=aug.max_shift, gain=aug.gain,
                  p_noise=aug.p_noise, noise_gain=aug.noise_gain, noise_lengths=NLEN, noise_len_max=NMAX)
    assert aug.seed >> 32 and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    quarter = AudioAugment(p_augment=0.25, max_shift=100, seed=aug.seed, device=DEV)       # no noises; most clips plain
    got = quarter.draw(torch.from_numpy(idx).to(DEV), torch.tensor([step], dtype=torch.int64, device=DEV))
    assert np.array_equal(got.cpu().numpy(), A.draw(aug.seed, step, idx, p_augment=0.25, max_shift=100))


# ---- 5. one captured graph draws anew at every replay --------------------------------------------------------------------
def test_a_captured_draw_and_front_end_follow_the_step_scalar():
    bank, lengths, aug = _device("i16")
    fe = MFCCFrontend(device=DEV)
    index = torch.from_numpy(np.random.default_rng(9).integers(0, N, B).astype(np.int32)).to(DEV)
    step_t = torch.tensor([5], dtype=torch.int64, device=DEV)

    def fn():
        rec = aug.draw(index, step_t)
        return rec, fe(bank, lengths, augment=rec, noise=aug.noise, noise_lengths=aug.noise_lengths, check=False)

    eager = []
    for s in (5, 6, 7):
        step_t.fill_(s)
        eager.append(tuple(t.clone() for t in fn()))
    step_t.fill_(5)
    graphed = GraphedStep(fn)
    for s, (rec, feats) in zip((5, 6, 7), eager):
        step_t.fill_(s)
        got_rec, got = graphed()
        torch.cuda.synchronize()
        assert torch.equal(got_rec, rec) and S.bits_equal(got, feats), s
    assert not torch.equal(eager[0][0], eager[1][0]) and not S.bits_equal(eager[1][1], eager[2][1])
    index.copy_(index.flip(0))                                                   # index is a captured input
    got_rec, _ = graphed()
    assert torch.equal(got_rec[:, 0], index)


# ---- 6. a training step from the audio bank ------------------------------------------------------------------------------
def _model():
    torch.manual_seed(3)
    return RNNClassifierModel("FastGRNNCUDA", 64, 1, [128], [None], [None], [1.0], [1.0], "sigmoid", "tanh",
                              num_classes=12, device=DEV)


def test_train_step_audio_equals_train_step_on_the_materialised_audio():
    bank, lengths, aug = _device("i16")
    fx = M.fixture()
    fe = MFCCFrontend(mean=fx["mean"], std=fx["std"], device=DEV)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 12, N)).to(DEV)
    index = torch.from_numpy(np.random.default_rng(4).integers(0, N, B).astype(np.int32)).to(DEV)
    model = _model()
    twin, third = copy.deepcopy(model), copy.deepcopy(model)
    start = [p.detach().clone() for p in model.parameters()]
    opt, t_opt = FusedAdam(model.parameters(), lr=0.01), FusedAdam(twin.parameters(), lr=0.01)

    def unfused_step():
        rec = aug.draw(index, t_opt.step_t)
        audio = aug.apply(bank, lengths, rec)
        feats = fe(audio, lengths[rec[:, 0].long()].contiguous())
        twin.init_hidden()
        return twin.train_step(feats.transpose(0, 1).contiguous(), labels[index.long()], t_opt)

    def fused_step(m, o, check=False):
        m.init_hidden()
        return m.train_step_audio(bank, lengths, labels, index, fe, aug, o, check=check)

    la, lb = fused_step(model, opt, check=True), unfused_step()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and bool(torch.isfinite(la)), (float(la), float(lb))
    for (name, p), q, p0 in zip(model.named_parameters(), twin.parameters(), start):
        assert torch.equal(p, q), name
        assert not torch.equal(p, p0), name
    for _ in range(2):
        fused_step(model, opt)
    # three replays of one captured step equal the three eager steps
    g_opt = FusedAdam(third.parameters(), lr=0.01, capturable=True)
    graphed = GraphedStep(lambda: fused_step(third, g_opt), undo=(third, g_opt))
    for _ in range(3):
        graphed()
    torch.cuda.synchronize()
    assert int(g_opt.step_t) == 3 == int(opt.step_t)
    for (name, p), q in zip(model.named_parameters(), third.parameters()):
        assert torch.equal(p, q), name
    with pytest.raises(TypeError):
        model.train_step_audio(bank, lengths, labels, index, fe, aug, torch.optim.Adam(model.parameters()))
