"""Device-side augmentation without a GPU: Philox known answers, the numpy oracle of tests/augment_cases.py against
independent facts, the draw oracle's properties, the C ABI's symbols and refusals (all before any launch), the shim's
argument errors and packing, and the static scans of the new kernel file's assembly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kws_amd import AudioAugment, MFCCFrontend, _lib, mfcc_features, pack_augment, unpack_augment
from tests import augment_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kws_amd", "csrc", "kernels_augment.hip")
OK, NULLP, SHAPE, DTYPE, WS, UNSUP = 0, 1, 2, 4, 5, 7


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))))
def test_philox_known_answers(counter, key, want):
    assert tuple(int(v) for v in A.philox(counter, key)) == want


def test_philox_is_elementwise():
    c0 = np.arange(5, dtype=np.uint32)
    got = A.philox((c0, 7, 9, 1), (3, 4))
    for i in range(5):
        assert [int(v[i]) for v in got] == [int(v) for v in A.philox((i, 7, 9, 1), (3, 4))]


# ---- the sample oracle against independent facts -------------------------------------------------------------------------
def _bank(seed=0, N=3, L=16000):
    return (0.3 * np.random.default_rng(seed).standard_normal((N, L))).astype(np.float32)


def test_the_identity_record_returns_the_clip():
    bank = _bank()
    lengths = np.array([16000, 1281, 9000], dtype=np.int32)
    for src in range(3):
        y, n = A.augment_clip(bank, lengths, A.pack([src], 0, 1.0)[0], [])
        assert n == lengths[src] and np.array_equal(y[:n], bank[src, :n]) and not y[n:].any()
    y, n = A.augment_clip(bank, None, A.pack([1], 0, 1.0)[0], [])
    assert n == 16000 and np.array_equal(y, bank[1])


@pytest.mark.parametrize("s", (1, -1, 37, -4000, 8999, -8999, 9000, 9005, -9005))
def test_a_shift_is_a_roll_with_the_wrapped_part_zeroed(s):
    bank, lengths = _bank(1), np.array([16000, 1281, 9000], dtype=np.int32)
    y, n = A.augment_clip(bank, lengths, A.pack([2], s, 1.0)[0], [])
    want = np.roll(bank[2, :9000], s)
    if s >= 0:
        want[:min(s, 9000)] = 0
    else:
        want[max(9000 + s, 0):] = 0
    assert n == 9000 and np.array_equal(y[:n], want) and (abs(s) < 9000) == bool(y.any())


def test_noise_at_a_tenth_is_the_references_wrapped_pad():
    bank = _bank(2)
    noise = (0.2 * np.random.default_rng(5).standard_normal(4000)).astype(np.float32)
    y, n = A.augment_clip(bank, None, A.pack([0], 0, 1.0, 0, 0, 0.1)[0], [noise])
    clip = bank[0].copy()                                   # audioAugmentation.py:47-49
    padded = np.pad(noise, (0, len(clip) - len(noise)), mode="wrap")
    want = clip + (np.float32(0.1) * padded[:len(clip)]).astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(y, want)
    # gain 0: the noise-only clip; a start offset rotates the noise
    y0, _ = A.augment_clip(bank, None, A.pack([0], 0, 0.0, 0, 3999, 0.1)[0], [noise])
    assert np.array_equal(y0[1:], (np.float32(0.1) * padded[:-1]).astype(np.float32)) and y0[0] == np.float32(0.1) * noise[3999]


def test_an_absent_noise_ignores_a_bank_full_of_nan():
    bank = _bank(3)
    y, _ = A.augment_clip(bank, None, A.pack([1], 5, 2.0, -1, 0, 0.5)[0], [np.full(7, np.nan, dtype=np.float32)])
    assert np.isfinite(y).all() and np.array_equal(y[5:], (np.float32(2.0) * bank[1, :-5]))


def test_int16_samples_are_exact():
    pcm = np.random.default_rng(4).integers(-32768, 32768, (2, 1280), dtype=np.int16)
    nz = np.array([-32768, 32767, 1], dtype=np.int16)
    y, _ = A.augment_clip(pcm, None, A.pack([1], 0, 1.0, 0, 1, 1.0)[0], [nz])
    want = pcm[1].astype(np.float64) / 32768 + nz[(1 + np.arange(1280)) % 3].astype(np.float64) / 32768
    assert np.array_equal(y, want.astype(np.float32))


def test_clamped_records_are_in_range_and_fixed_points():
    nlen = np.array([1, 7, 4000], dtype=np.int32)
    rec = A.clamp_records(A.hostile_records(11, 3), 11, nlen, 4000)
    assert (rec[:, 0] >= 0).all() and (rec[:, 0] < 11).all() and (rec[:, 2] < 3).all() and (rec[:, 2] >= 0).all()
    assert (rec[:, 3] >= 0).all() and (rec[:, 3] < nlen[rec[:, 2]]).all() and (np.abs(rec[:, 1]) <= 1 << 20).all()
    assert np.array_equal(A.clamp_records(rec, 11, nlen, 4000), rec)
    none = A.clamp_records(A.hostile_records(11, 3), 11, None, 1)
    assert (none[:, 2] == -1).all()


# ---- the draw oracle -----------------------------------------------------------------------------------------------------
SEED, STEP = 0x9E3779B97F4A7C15, (1 << 33) + 5
NLEN = np.array([1, 7, 4000], dtype=np.int32)
KW = dict(p_augment=1.0, max_shift=1600, gain=(0.5, 1.5), p_noise=0.5, noise_gain=(0.05, 0.2), noise_lengths=NLEN,
          noise_len_max=4000)


def test_a_record_depends_on_seed_step_and_clip_alone():
    idx = np.arange(4096, dtype=np.int32)[::-1].copy()
    big = A.draw(SEED, STEP, idx, **KW)
    for B in (1, 37, 1030):
        assert np.array_equal(A.draw(SEED, STEP, idx[:B], **KW), big[:B])
    nxt = A.draw(SEED, STEP + 1, idx, **KW)
    assert not np.array_equal(nxt[:, 1:], big[:, 1:]) and np.array_equal(nxt[:, 0], idx)
    assert not np.array_equal(A.draw(SEED + (1 << 32), STEP, idx, **KW)[:, 1:], big[:, 1:])      # the seed's high word
    assert not np.array_equal(A.draw(SEED, STEP + (1 << 32), idx, **KW)[:, 1:], big[:, 1:])      # the step's high word


def test_the_draws_lie_in_their_ranges_and_the_coin_is_fair():
    rec = A.draw(SEED, STEP, np.arange(4096, dtype=np.int32), **KW)
    with_noise = rec[:, 2] >= 0
    assert abs(int(with_noise.sum()) - 2048) <= 192                  # six binomial standard deviations of 32
    assert (np.abs(rec[:, 1]) <= 1600).all() and rec[:, 1].min() < -1500 and rec[:, 1].max() > 1500
    assert (rec[:, 2] < 3).all() and set(rec[with_noise, 2]) == {0, 1, 2}
    assert (rec[:, 3] >= 0).all() and (rec[with_noise, 3] < NLEN[rec[with_noise, 2]]).all()
    g, ng = A.gains(rec)
    assert (g >= 0.5).all() and (g <= 1.5).all() and (ng[with_noise] >= np.float32(0.05)).all() and (ng <= np.float32(0.2)).all()
    assert (rec[~with_noise, 3] == 0).all() and (ng[~with_noise] == 0).all()


def test_an_unaugmented_clip_gets_the_identity_record():
    idx = np.arange(512, dtype=np.int32) * 3
    rec = A.draw(SEED, 7, idx, **dict(KW, p_augment=0.25))
    g, ng = A.gains(rec)
    plain = (rec[:, 1] == 0) & (rec[:, 2] == -1) & (rec[:, 3] == 0) & (g == 1) & (ng == 0)
    assert 0.6 < plain.mean() < 0.9 and np.array_equal(rec[:, 0], idx)
    assert np.array_equal(A.draw(SEED, 7, idx, **dict(KW, p_augment=0.0)), A.pack(idx, 0, 1.0))
    # the reference's settings: a constant noise gain is that constant, bit for bit
    ref = A.draw(SEED, 7, idx, p_augment=1.0, noise_lengths=NLEN, noise_len_max=4000)
    assert set(A.gains(ref)[1][ref[:, 2] >= 0]) == {np.float32(0.1)} and (A.gains(ref)[0] == 1).all()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


ONE = C.c_void_p(256)                          # a non-NULL pointer that no refused call may touch


def _desc(**kw):
    f = dict(B=2, L=16000, clip_stride=16000, audio_dtype=0, n_mfcc=32, order=1, width=9, max_len=99, top_db=80.0, flags=0)
    f.update(kw)
    return _lib.MfccDesc(**f)


def _bankd(**kw):
    f = dict(n_clips=5, n_noise=2, noise_stride=4000, noise_len_max=4000, reserved=0)
    f.update(kw)
    return _lib.MfccBank(**f)


def _aug(lib, d=None, bank=None, audio=ONE, lengths=None, noise=ONE, nlen=ONE, aug=ONE, tables=ONE, mean=None, std=None,
         feats=ONE, no_desc=False, no_bank=False):
    d = _desc() if d is None else d
    bank = _bankd() if bank is None else bank
    return lib.fastgrnn_hip_mfcc_augment(None if no_desc else C.byref(d), None if no_bank else C.byref(bank), audio,
                                         lengths, noise, nlen, aug, tables, mean, std, feats, None, 0, None)


def _ranges(**kw):
    f = dict(p_augment=0.25, p_noise=0.5, max_shift=1600, reserved=0, gain_lo=0.8, gain_hi=1.2, noise_gain_lo=0.1,
             noise_gain_hi=0.1)
    f.update(kw)
    return _lib.AugmentRanges(**f)


def _draw(lib, B=4, step=ONE, index=ONE, r=None, n_noise=2, nmax=4000, nlen=ONE, aug=ONE, no_ranges=False):
    r = _ranges() if r is None else r
    return lib.fastgrnn_hip_augment_draw(B, 1 << 40, step, index, None if no_ranges else C.byref(r), n_noise, nmax, nlen,
                                         aug, None)


def test_symbols_exist_and_the_abi_version_stays(lib):
    header = open(os.path.join(ROOT, "include", "fastgrnn_hip.h")).read()
    for name in ("fastgrnn_hip_mfcc_augment", "fastgrnn_hip_augment_draw"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and name + "(" in header
    assert lib.fastgrnn_hip_abi_version() == 1
    assert C.sizeof(_lib.MfccAug) == 24 and C.sizeof(_lib.MfccBank) == 24 and C.sizeof(_lib.AugmentRanges) == 32
    for word in ("fastgrnn_mfcc_aug;", "fastgrnn_mfcc_bank;", "fastgrnn_augment_ranges;", "0xD2511F53", "0xBB67AE85"):
        assert word in header


def test_the_augmented_call_refuses_null_pointers(lib):
    assert _aug(lib, no_desc=True) == NULLP and _aug(lib, no_bank=True) == NULLP
    for kw in (dict(audio=None), dict(aug=None), dict(tables=None), dict(feats=None), dict(noise=None), dict(nlen=None),
               dict(mean=ONE), dict(std=ONE)):
        assert _aug(lib, **kw) == NULLP, kw
    # without noises the noise pointers may be NULL and the noise sizes are not read (the next refusal in line shows it)
    assert _aug(lib, bank=_bankd(n_noise=0, noise_stride=0, noise_len_max=0), noise=None, nlen=None, feats=None) == NULLP


def test_the_augmented_call_refuses_bad_shapes_and_sizes(lib):
    for kw in (dict(n_clips=0), dict(n_clips=-1), dict(n_noise=-1), dict(noise_stride=0), dict(noise_stride=-4000)):
        assert _aug(lib, bank=_bankd(**kw)) == SHAPE, kw
    for kw in (dict(noise_len_max=0), dict(noise_len_max=-1), dict(noise_len_max=(1 << 24) + 1)):
        assert _aug(lib, bank=_bankd(**kw)) == UNSUP, kw
    for kw in (dict(noise_len_max=1 << 24), dict(noise_len_max=1), dict(noise_stride=1), dict(n_clips=1 << 30)):
        assert _aug(lib, bank=_bankd(**kw), feats=None) == NULLP, kw
    # everything the plain call refuses is still refused
    for kw, st in ((dict(B=0), SHAPE), (dict(clip_stride=0), SHAPE), (dict(top_db=float("nan")), SHAPE),
                   (dict(audio_dtype=2), DTYPE), (dict(L=1279), UNSUP), (dict(L=16001), UNSUP), (dict(n_mfcc=65), UNSUP),
                   (dict(order=3), UNSUP), (dict(width=4), UNSUP), (dict(flags=2), UNSUP)):
        assert _aug(lib, _desc(**kw)) == st, kw


def test_the_draw_refuses(lib):
    assert _draw(lib, no_ranges=True) == NULLP
    for kw in (dict(step=None), dict(index=None), dict(aug=None), dict(nlen=None)):
        assert _draw(lib, **kw) == NULLP, kw
    assert _draw(lib, B=0) == SHAPE and _draw(lib, B=-2) == SHAPE and _draw(lib, n_noise=-1) == SHAPE
    nan, inf = float("nan"), float("inf")
    for kw in (dict(p_augment=-0.01), dict(p_augment=1.01), dict(p_augment=nan), dict(p_noise=2.0), dict(p_noise=nan),
               dict(gain_lo=1.3), dict(gain_hi=inf), dict(gain_lo=-inf), dict(gain_lo=nan), dict(gain_hi=nan),
               dict(noise_gain_lo=0.2), dict(noise_gain_hi=inf), dict(noise_gain_lo=nan),
               dict(gain_lo=-3e38, gain_hi=3e38)):
        assert _draw(lib, r=_ranges(**kw)) == SHAPE, kw
    for kw in (dict(max_shift=-1), dict(max_shift=(1 << 20) + 1)):
        assert _draw(lib, r=_ranges(**kw)) == UNSUP, kw
    assert _draw(lib, nmax=0) == UNSUP and _draw(lib, nmax=(1 << 24) + 1) == UNSUP
    # the edges pass (the next refusal in line shows it); no noises: the lengths may be NULL
    for kw in (dict(p_augment=0.0), dict(p_augment=1.0, p_noise=1.0), dict(max_shift=0), dict(max_shift=1 << 20),
               dict(gain_lo=1.0, gain_hi=1.0), dict(gain_lo=-1.0, gain_hi=0.0)):
        assert _draw(lib, r=_ranges(**kw), aug=None) == NULLP, kw
    assert _draw(lib, n_noise=0, nmax=0, nlen=None, aug=None) == NULLP


# ---- the shim ------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_round_trip():
    src = torch.tensor([3, 0, 7], dtype=torch.int64)
    rec = pack_augment(src, torch.tensor([5, -5, 0]), torch.tensor([1.0, 0.0, -0.5]), noise=torch.tensor([-1, 2, 0]),
                       noise_off=torch.tensor([0, 6, 1]), noise_gain=0.1)
    assert rec.shape == (3, 6) and rec.dtype == torch.int32 and rec.is_contiguous()
    want = A.pack([3, 0, 7], [5, -5, 0], [1.0, 0.0, -0.5], [-1, 2, 0], [0, 6, 1], 0.1)
    assert np.array_equal(rec.numpy(), want)
    s, sh, g, nz, off, ng = unpack_augment(rec)
    assert s.tolist() == [3, 0, 7] and sh.tolist() == [5, -5, 0] and nz.tolist() == [-1, 2, 0] and off.tolist() == [0, 6, 1]
    assert g.dtype == torch.float32 and g.tolist() == [1.0, 0.0, -0.5] and torch.equal(ng, torch.full((3,), 0.1))
    ident = pack_augment(torch.arange(4), 0, 1.0)
    assert np.array_equal(ident.numpy(), A.pack(np.arange(4), 0, 1.0))
    for bad in (lambda: pack_augment(torch.tensor(3), 0, 1.0), lambda: pack_augment(torch.arange(3), torch.arange(2), 1.0),
                lambda: unpack_augment(torch.zeros(3, 5, dtype=torch.int32)), lambda: unpack_augment(torch.zeros(3, 6))):
        with pytest.raises(ValueError):
            bad()


def test_audio_augment_construction_and_set_noise_need_no_gpu():
    aug = AudioAugment(p_augment=1.0, max_shift=1600, gain=(0.5, 1.5), noise_gain=0.1, seed=(1 << 63) + 9)
    assert aug.n_noise == 0 and aug.noise is None and aug.gain == (0.5, 1.5) and aug.noise_gain == (0.1, 0.1)
    aug.set_noise([torch.ones(1), torch.arange(7.0), torch.full((4000,), 2.0)])
    assert aug.noise.shape == (3, 4000) and aug.noise.dtype == torch.float32 and aug.noise_lengths.tolist() == [1, 7, 4000]
    assert aug.noise_lengths.dtype == torch.int32 and aug.noise[1, :8].tolist() == [0, 1, 2, 3, 4, 5, 6, 0]
    assert set(aug.state_dict()) == {"noise", "noise_lengths"}
    pcm = AudioAugment(noises=[torch.tensor([1, -2, 3], dtype=torch.int16)])
    assert pcm.noise.dtype == torch.int16 and pcm.noise_lengths.tolist() == [3]
    aug.set_noise([])
    assert aug.n_noise == 0
    for bad in (dict(p_augment=1.5), dict(p_noise=-0.1), dict(max_shift=-1), dict(max_shift=(1 << 20) + 1),
                dict(gain=(1.0, 0.5)), dict(noise_gain=float("inf")), dict(seed=-1), dict(seed=1 << 64),
                dict(noises=[torch.zeros(0)]), dict(noises=[torch.zeros(3), torch.zeros(3, dtype=torch.int16)]),
                dict(noises=[torch.zeros(3, dtype=torch.float64)]), dict(noises=[torch.zeros(2, 3)])):
        with pytest.raises(ValueError):
            AudioAugment(**bad)


def test_apply_is_the_oracle_on_the_host():
    """``AudioAugment.apply`` is plain torch: on the CPU it must give the numpy oracle's samples bit for bit, for in-range
    records and -- through the clamped records -- for the hostile ones."""
    rng = np.random.default_rng(8)
    bank = (0.3 * rng.standard_normal((11, 2000))).astype(np.float32)
    lengths = np.array([1280, 1281, 1999, 2000, 1500, 1280, 2000, 1700, 1281, 1999, 2000], dtype=np.int32)
    noises = [np.array([0.5], dtype=np.float32), rng.standard_normal(7).astype(np.float32),
              rng.standard_normal(1500).astype(np.float32)]
    aug = AudioAugment(noises=[torch.from_numpy(z) for z in noises])
    nlen = np.array([1, 7, 1500], dtype=np.int32)
    rec = np.concatenate([A.draw(5, 9, rng.integers(0, 11, 20), p_augment=0.9, max_shift=2100, gain=(-1.0, 1.0),
                                 noise_gain=(0.05, 0.2), noise_lengths=nlen, noise_len_max=1500),
                          A.hostile_records(11, 3)])
    want, wlen = A.augment_batch(bank, lengths, A.clamp_records(rec, 11, nlen, 1500), noises)
    got = aug.apply(torch.from_numpy(bank), torch.from_numpy(lengths), torch.from_numpy(rec))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    pcm = rng.integers(-32768, 32768, (11, 2000), dtype=np.int16)
    aug16 = AudioAugment(noises=[torch.from_numpy((z * 20000).astype(np.int16)) for z in noises])
    want, _ = A.augment_batch(pcm, None, A.clamp_records(rec, 11, nlen, 1500), [(z * 20000).astype(np.int16) for z in noises])
    got = aug16.apply(torch.from_numpy(pcm), None, torch.from_numpy(rec))
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


def test_the_shims_argument_errors():
    x = torch.zeros(2, 16000)
    rec = pack_augment(torch.arange(2), 0, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        mfcc_features(x, augment=rec)
    with pytest.raises(RuntimeError, match="GPU"):
        MFCCFrontend()(x, augment=rec)
    with pytest.raises(RuntimeError, match="go with augment"):
        mfcc_features(_FakeCuda(x), noise=x)
    aug = AudioAugment()
    with pytest.raises(RuntimeError, match="CUDA"):
        aug.draw(torch.arange(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError):
        aug.draw([0, 1], torch.zeros(1, dtype=torch.int64))
    from kws_amd import features
    dev_less = lambda **kw: features._check_augment_operands(kw.get("augment", _FakeCuda(rec)), kw.get("noise"),
                                                             kw.get("noise_lengths"), _FakeCuda(x))
    for kw, msg in ((dict(augment=_FakeCuda(rec.to(torch.int64))), "int32 records"),
                    (dict(augment=_FakeCuda(rec[:, :5].contiguous())), "int32 records"),
                    (dict(augment=_FakeCuda(rec.t().contiguous().t())), "contiguous"),
                    (dict(noise=_FakeCuda(torch.zeros(1, 8))), "go together"),
                    (dict(noise=_FakeCuda(torch.zeros(1, 8, dtype=torch.int16)),
                          noise_lengths=_FakeCuda(torch.ones(1, dtype=torch.int32))), "audio's dtype"),
                    (dict(noise=_FakeCuda(torch.zeros(8)), noise_lengths=_FakeCuda(torch.ones(1, dtype=torch.int32))),
                     "noise_len_max"),
                    (dict(noise=_FakeCuda(torch.zeros(2, 8)), noise_lengths=_FakeCuda(torch.ones(1, dtype=torch.int32))),
                     "noise_lengths must be int32")):
        with pytest.raises(RuntimeError, match=msg):
            dev_less(**kw)
    assert dev_less() == (2, 0, 1, 1)
    assert dev_less(noise=_FakeCuda(torch.zeros(3, 8)), noise_lengths=_FakeCuda(torch.ones(3, dtype=torch.int32))) == (2, 3, 8, 8)


class _FakeCuda(torch.Tensor):
    """A host tensor that says it is on the device: the shim's shape, dtype and contiguity checks run without a GPU."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


# ---- static scans of the new kernel source -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def augment_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels_augment.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                    "-o", out, SRC], check=True, cwd=os.path.dirname(SRC), capture_output=True)
    return out


def test_war_scan_clean(augment_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "war_scan.py"), augment_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "UNBOUNDED" not in r.stdout and "NOT SCANNED" not in r.stdout
    assert r.stdout.strip().splitlines()[-1] == "total pairs: 0"


@pytest.mark.parametrize("mode", ("--strict", "--narrow"))
def test_no_lds_write_pending_at_a_branch_with_memory_instructions_behind_it(augment_asm, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_branch_vmem_scan.py"), augment_asm, mode],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "sites in loops: 0", r.stdout[-2000:]


def test_no_branch_between_the_mfmas_of_a_loop(augment_asm):
    """As tests/test_mfcc_cpu.py for mfcc_k: the three products' MFMA stretches are whole batches."""
    kernels, cur = {}, None
    for line in open(augment_asm):
        s = line.split(";")[0].strip()
        if s.endswith(":") and s.startswith("_Z"):
            cur = kernels.setdefault(s[:-1], [])
        elif cur is not None and s and (s.endswith(":") or not s.startswith(".")):
            cur.append(s)
    mine = {k: v for k, v in kernels.items() if "mfcc_aug_k" in k}
    assert len(mine) == 2 and not any("mfcc_k" in k for k in kernels)
    for name, ins in mine.items():
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
        assert len(blocks) == 3 and [b % q for b, q in zip(blocks, (56, 16, 8))] == [0, 0, 0], (name, blocks)


def test_the_kernels_use_no_scratch_and_fit_sixteen_waves():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    rows = {r["pretty"]: r for r in resource_usage.usage(SRC)}
    main = [r for n, r in rows.items() if "mfcc_aug_k" in n]
    assert len(main) == 2                                                        # fp32 and int16 banks
    for r in main:
        assert r["scratch"] == 0 and r["vgpr"] + r.get("agpr", 0) <= 128 and r["lds"] <= 163840
    draw = [r for n, r in rows.items() if "aug_draw_k" in n]
    assert len(draw) == 1 and draw[0]["scratch"] == 0 and draw[0]["lds"] == 0
