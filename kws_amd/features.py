"""MFCC and delta features from raw audio on the device, behind the C ABI's ``fastgrnn_hip_mfcc``.

The reference featurises on the host with ``librosa.feature.mfcc`` + ``librosa.feature.delta``
(data_pipeline/mfccProcessor.py:43-58): once per file for the dataset (data_pipeline/preprocessing.py) and every 50 ms
in the live detector (inferencetry.py:165-200: the last second of PCM, peak-normalised, featurised, padded or cut to 99
frames, normalised with ``mean`` / ``std``).  ``mfcc_features`` is that chain in one launch per batch of clips --
librosa 0.10.2's defaults restated in include/fastgrnn_hip.h -- and ``MFCCFrontend`` the module that keeps its
settings, the constant tables and the normalisation statistics.  Its output ``[B, max_len, F]`` is a frame pool:
``RNNClassifierModel.detect_audio`` and ``loss_windows(feats.view(B * T, F), starts, labels)`` read it in place.
With ``augment=records`` the same call reads an audio BANK through per-clip augmentation records (``kws_amd.augment``;
``fastgrnn_hip_mfcc_augment``): shift, gain and noise are applied while a clip is loaded and no augmented audio is
written.  There is no host fallback: without the library every call raises.
"""
from __future__ import annotations

import ctypes as C
import functools

import torch
from torch import nn

from . import _lib
from .fastgrnn_cuda import _call, _check_input, _ptr

FEATURE_TYPES = {"mfcc": 0, "delta": 1, "delta_delta": 2}     # mfccProcessor.py:25-30 -> the delta order
_AUDIO_DTYPES = {torch.float32: _lib.MFCC_AUDIO_F32, torch.int16: _lib.MFCC_AUDIO_I16}

_tables_cache = {}


def mfcc_tables(device):
    """The featuriser's constant tables on ``device`` (window-folded DFT basis, mel weights, DCT, delta taps), computed
    once per device by ``fastgrnn_hip_mfcc_init_tables``: a float32 tensor the calls only read."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("mfcc tables live on the GPU (got device %s)" % device)
    idx = torch.cuda.current_device() if device.index is None else device.index
    tab = _tables_cache.get(idx)
    if tab is None:
        lib = _lib.load()
        dev = torch.device("cuda", idx)
        with torch.cuda.device(dev):
            tab = torch.empty(lib.fastgrnn_hip_mfcc_tables_bytes() // 4, dtype=torch.float32, device=dev)
            _call(lib.fastgrnn_hip_mfcc_init_tables, "fastgrnn mfcc_init_tables", None, dev, None, _ptr(tab))
        _tables_cache[idx] = tab
    return tab


@functools.lru_cache(maxsize=256)
def _mfcc_plan(B, L, clip_stride, audio_dtype, n_mfcc, order, width, max_len, top_db, flags):
    """The C descriptor of a call signature and its workspace size: one ctypes round trip per signature."""
    desc = _lib.MfccDesc(B, L, clip_stride, audio_dtype, n_mfcc, order, width, max_len, top_db, flags)
    return desc, int(_lib.load().fastgrnn_hip_mfcc_workspace_bytes(C.byref(desc)))


@functools.lru_cache(maxsize=256)
def _augment_plan(B, L, clip_stride, audio_dtype, n_mfcc, order, width, max_len, top_db, flags, n_clips, n_noise,
                  noise_stride, noise_len_max):
    """``_mfcc_plan`` for the augmented call: the descriptor, the bank's sizes and the workspace size."""
    desc, nbytes = _mfcc_plan(B, L, clip_stride, audio_dtype, n_mfcc, order, width, max_len, top_db, flags)
    return desc, _lib.MfccBank(n_clips, n_noise, noise_stride, noise_len_max, 0), nbytes


def check_augment_range(augment, n_clips, noise_lengths=None):
    """The one host range check of an augmented call: every ``src`` in ``0..n_clips-1``, every ``noise`` below the
    number of noises, every ``noise_off`` of a record with a noise in ``0..nlen-1``; one device reduction, one
    device-to-host copy, ``ValueError`` otherwise.  (The kernel clamps whatever it is given; this tells the caller that
    it would have.)"""
    src, noise, off = augment[:, 0], augment[:, 2], augment[:, 3]
    n_noise = 0 if noise_lengths is None else noise_lengths.numel()
    bad = (src < 0) | (src >= n_clips) | (noise >= n_noise)
    if n_noise:
        nlen = noise_lengths[noise.clamp(0, n_noise - 1).long()]
        bad = bad | ((noise >= 0) & ((off < 0) | (off >= nlen)))
    if bool(bad.any()):
        raise ValueError("augment: a record lies outside its range (src in [0, %d), noise < %d, 0 <= noise_off < the "
                         "noise's length)" % (n_clips, n_noise))


def _order_of(feature_type):
    if feature_type not in FEATURE_TYPES:
        raise ValueError("Unknown feature type: %r (mfcc, delta, delta_delta)" % (feature_type,))
    return FEATURE_TYPES[feature_type]


def _check_settings(n_mfcc, order, width, max_len, L=None):
    n_mfcc, width, max_len = int(n_mfcc), int(width), int(max_len)
    if not 1 <= n_mfcc <= 64:
        raise ValueError("n_mfcc must be in 1..64 (got %d)" % n_mfcc)
    if width < 3 or width > 15 or width % 2 == 0:
        raise ValueError("width must be odd and in 3..15 (got %d)" % width)
    if max_len < 1:
        raise ValueError("max_len must be positive (got %d)" % max_len)
    if L is not None:
        if not _lib.MFCC_MIN_SAMPLES <= L <= _lib.MFCC_MAX_SAMPLES:
            raise ValueError("clips of %d..%d samples are supported (got %d)"
                             % (_lib.MFCC_MIN_SAMPLES, _lib.MFCC_MAX_SAMPLES, L))
        if L < 160 * (width - 1):
            raise ValueError("a delta of width %d needs %d frames: clips of at least %d samples (got %d)"
                             % (width, width, 160 * (width - 1), L))
    return n_mfcc, width, max_len


def mfcc_features(audio, lengths=None, *, n_mfcc=32, feature_type="delta", width=9, max_len=99, top_db=80.0,
                  mean=None, std=None, peak_normalize=False, tables=None, augment=None, noise=None, noise_lengths=None,
                  check=True):
    """``audio:[B,L]`` fp32 samples or int16 PCM on the device -> ``[B, max_len, F]`` fp32 features,
    ``F = n_mfcc * (order + 1)`` with ``feature_type`` ``"mfcc"`` / ``"delta"`` / ``"delta_delta"`` = order 0 / 1 / 2:
    ``[mfcc; delta; delta2]`` of every clip as ``MFCCProcessor.compute_features`` stacks them (transposed: time-major
    rows), padded with zeros or cut to ``max_len`` frames, then ``(f - mean) / std`` if both are given (``[F]``).

    ``audio`` needs unit stride along the samples and may have any positive row stride, also one below ``L``
    (``MFCCFrontend.clips_of``: overlapping clips of one recording, no copy).  ``1280 <= L <= 16000``.  ``lengths``:
    ``[B]`` int32 on the device, ``1280 <= lengths[b] <= L`` (the caller's obligation; the kernel clamps): clip ``b`` is
    its first ``lengths[b]`` samples and has ``1 + lengths[b] // 160`` frames.  ``peak_normalize`` divides every clip by
    its ``max|y|`` first (inferencetry.py:172-175).  ``top_db=None`` (or negative) switches the dB clip off.  One launch
    on the current stream; nothing synchronises.

    With ``augment`` (``[B, 6]`` int32 records on the device: ``kws_amd.pack_augment`` / ``AudioAugment.draw``) ``audio``
    is a BANK ``[N, L]``, ``lengths`` is ``[N]``, and output clip ``b`` is bank clip ``src[b]`` shifted, scaled and mixed
    with a noise while it is loaded (``fastgrnn_hip_mfcc_augment``; ``AudioAugment.apply`` is the same definition in
    torch ops): the output has ``B = augment.shape[0]`` clips and no augmented audio is ever written.  ``noise``:
    ``[n_noise, noise_len_max]`` of ``audio``'s dtype with unit stride along the samples, ``noise_lengths``: ``[n_noise]``
    int32, both or neither.  ``check=True`` validates the records' ranges (``check_augment_range``: one reduction and one
    synchronisation); pass ``check=False`` in a captured step -- the kernel clamps every record into its range."""
    lib = _lib.load()
    order = _order_of(feature_type)
    if not isinstance(audio, torch.Tensor):
        raise TypeError("audio must be a torch.Tensor")
    if not audio.is_cuda:
        raise RuntimeError("audio must be a CUDA tensor")
    if audio.dim() != 2:
        raise RuntimeError("audio must be [B, L] (got %d dimensions)" % audio.dim())
    if audio.dtype not in _AUDIO_DTYPES:
        raise RuntimeError("audio must be float32 samples or int16 PCM (got %s)" % audio.dtype)
    N, L = audio.shape                                   # (N: the clips of audio -- the batch, or the bank under augment)
    if N < 1:
        raise RuntimeError("audio holds no clips")
    n_mfcc, width, max_len = _check_settings(n_mfcc, order, width, max_len, L)
    if audio.stride(1) != 1 or (N > 1 and audio.stride(0) < 1):
        raise RuntimeError("audio needs unit stride along the samples and a positive row stride (got strides %s)"
                           % (tuple(audio.stride()),))
    dev = audio.device
    F = n_mfcc * (order + 1)
    if (mean is None) != (std is None):
        raise RuntimeError("mean and std go together")
    for t, name in ((mean, "mean"), (std, "std")):
        if t is not None:
            _check_input(t, name)
            if t.dtype != torch.float32 or t.numel() != F or t.device != dev:
                raise RuntimeError("%s must be float32 [%d] on %s" % (name, F, dev))
    if lengths is not None:
        _check_input(lengths, "lengths")
        if lengths.dtype != torch.int32 or lengths.numel() != N or lengths.device != dev:
            raise RuntimeError("lengths must be int32 [%d] on %s" % (N, dev))
    B = N
    if augment is None:
        if noise is not None or noise_lengths is not None:
            raise RuntimeError("noise and noise_lengths go with augment")
    else:
        B, n_noise, noise_stride, noise_len_max = _check_augment_operands(augment, noise, noise_lengths, audio)
        if check:
            check_augment_range(augment, N, noise_lengths)
    if tables is None:
        tables = mfcc_tables(dev)
    elif tables.device != dev or tables.dtype != torch.float32 or tables.numel() * 4 < lib.fastgrnn_hip_mfcc_tables_bytes():
        raise RuntimeError("tables must be the float32 tensor of mfcc_tables() on %s" % dev)
    top = -1.0 if top_db is None else float(top_db)
    flags = _lib.MFCC_PEAK_NORMALIZE if peak_normalize else 0
    plan = (B, L, int(audio.stride(0)) if N > 1 else L, _AUDIO_DTYPES[audio.dtype], n_mfcc, order, width, max_len, top,
            flags)
    with torch.cuda.device(dev):
        feats = torch.empty((B, max_len, F), dtype=torch.float32, device=dev)
        if augment is None:
            desc, nbytes = _mfcc_plan(*plan)
            _call(lib.fastgrnn_hip_mfcc, "fastgrnn mfcc", "mfcc", dev, nbytes, C.byref(desc), _ptr(audio),
                  _ptr(lengths), _ptr(tables), _ptr(mean), _ptr(std), _ptr(feats))
        else:
            desc, bank, nbytes = _augment_plan(*plan, N, n_noise, noise_stride, noise_len_max)
            _call(lib.fastgrnn_hip_mfcc_augment, "fastgrnn mfcc_augment", "mfcc_augment", dev, nbytes, C.byref(desc),
                  C.byref(bank), _ptr(audio), _ptr(lengths), _ptr(noise), _ptr(noise_lengths), _ptr(augment),
                  _ptr(tables), _ptr(mean), _ptr(std), _ptr(feats))
    return feats


@functools.lru_cache(maxsize=256)
def _stream_plan(N, hop, audio_dtype, clip0, B, n_mfcc, order, width, max_len, top_db, flags):
    """``_mfcc_plan`` for the streamed calls: the descriptor and the bytes of the frames workspace (a function of N)."""
    desc = _lib.MfccStreamDesc(N, hop, audio_dtype, clip0, B, n_mfcc, order, width, max_len, top_db, flags)
    return desc, int(_lib.load().fastgrnn_hip_mfcc_stream_workspace_bytes(C.byref(desc)))


def _check_stream_geometry(N, hop_samples, clip):
    """The clip count of a recording of ``N`` samples, or the ``ValueError`` that names the broken rule."""
    hop_samples, clip = int(hop_samples), int(clip)
    if clip != _lib.MFCC_STREAM_CLIP:
        raise ValueError("the streamed front end takes clips of exactly %d samples (got %d)" % (_lib.MFCC_STREAM_CLIP, clip))
    if hop_samples < 1 or hop_samples % _lib.MFCC_STREAM_HOP_UNIT:
        raise ValueError("the streamed front end takes hops that are a positive multiple of %d samples, the frame hop "
                         "(got %d)" % (_lib.MFCC_STREAM_HOP_UNIT, hop_samples))
    if N < clip:
        raise ValueError("recording of %d samples is shorter than a clip of %d" % (N, clip))
    if N >= 2 ** 31:
        raise ValueError("recordings of fewer than 2^31 samples are supported (got %d)" % N)
    return (N - clip) // hop_samples + 1


def mfcc_stream_features(recording, hop_samples=800, *, clip0=0, num_clips=None, frames=None, return_frames=False,
                         clip=16000, n_mfcc=32, feature_type="delta", width=9, max_len=99, top_db=80.0, mean=None,
                         std=None, peak_normalize=False, tables=None):
    """The features of the detector's overlapping clips of ONE 1-D ``recording`` (fp32 samples or int16 PCM on the
    device, unit stride) -> ``[B, max_len, F]``: what ``mfcc_features(MFCCFrontend.clips_of(recording, hop_samples))``
    returns for clips ``clip0 .. clip0 + num_clips - 1`` (``num_clips=None``: all from ``clip0`` on), with every 10 ms
    frame of the recording taken through the DFT and the mel projection once instead of once per clip that contains it
    (``fastgrnn_hip_mfcc_stream_frames`` / ``_clips``).  Without ``peak_normalize`` the result equals the per-clip
    call's bit for bit; with it, by fp32 roundings of the interior frames' scaling only.

    ``hop_samples`` is a multiple of 160 and ``clip`` is 16000: anything else is a ``ValueError`` -- there is no
    fallback to the per-clip call.  ``frames``: the workspace of an earlier call on the same recording
    (``return_frames=True`` returns ``(feats, frames)``); given it, the frames call is skipped and only the clips are
    featurised, so a long recording is scored chunk by chunk in bounded memory.  The other settings are
    ``mfcc_features``'s.  Two launches (one with ``frames``) on the current stream; nothing synchronises."""
    lib = _lib.load()
    order = _order_of(feature_type)
    if not isinstance(recording, torch.Tensor):
        raise TypeError("recording must be a torch.Tensor")
    if not recording.is_cuda:
        raise RuntimeError("recording must be a CUDA tensor")
    if recording.dim() != 1:
        raise ValueError("recording must be 1-D (got %d dimensions)" % recording.dim())
    if recording.dtype not in _AUDIO_DTYPES:
        raise RuntimeError("recording must be float32 samples or int16 PCM (got %s)" % recording.dtype)
    N = recording.shape[0]
    n_mfcc, width, max_len = _check_settings(n_mfcc, order, width, max_len)
    total = _check_stream_geometry(N, hop_samples, clip)
    if recording.stride(0) != 1:
        raise RuntimeError("recording needs unit stride (got %d)" % recording.stride(0))
    clip0 = int(clip0)
    B = total - clip0 if num_clips is None else int(num_clips)
    if clip0 < 0 or B < 1 or clip0 + B > total:
        raise ValueError("clips %d .. %d lie outside the recording's %d clips" % (clip0, clip0 + B - 1, total))
    dev = recording.device
    F = n_mfcc * (order + 1)
    if (mean is None) != (std is None):
        raise RuntimeError("mean and std go together")
    for t, name in ((mean, "mean"), (std, "std")):
        if t is not None:
            _check_input(t, name)
            if t.dtype != torch.float32 or t.numel() != F or t.device != dev:
                raise RuntimeError("%s must be float32 [%d] on %s" % (name, F, dev))
    if tables is None:
        tables = mfcc_tables(dev)
    elif tables.device != dev or tables.dtype != torch.float32 or tables.numel() * 4 < lib.fastgrnn_hip_mfcc_tables_bytes():
        raise RuntimeError("tables must be the float32 tensor of mfcc_tables() on %s" % dev)
    top = -1.0 if top_db is None else float(top_db)
    flags = _lib.MFCC_PEAK_NORMALIZE if peak_normalize else 0
    desc, nbytes = _stream_plan(N, int(hop_samples), _AUDIO_DTYPES[recording.dtype], clip0, B, n_mfcc, order, width,
                                max_len, top, flags)
    with torch.cuda.device(dev):
        if frames is None:
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            _call(lib.fastgrnn_hip_mfcc_stream_frames, "fastgrnn mfcc_stream_frames", "mfcc_stream_frames", dev, None,
                  C.byref(desc), _ptr(recording), _ptr(tables), _ptr(ws), nbytes)
        else:
            ws = frames
            _check_input(ws, "frames")
            if ws.dtype != torch.float32 or ws.device != dev or ws.numel() * 4 < nbytes or ws.data_ptr() % 256:
                raise RuntimeError("frames must be the workspace an earlier call on this recording returned "
                                   "(float32, %d bytes, on %s)" % (nbytes, dev))
        feats = torch.empty((B, max_len, F), dtype=torch.float32, device=dev)
        _call(lib.fastgrnn_hip_mfcc_stream_clips, "fastgrnn mfcc_stream_clips", "mfcc_stream_clips", dev, None,
              C.byref(desc), _ptr(recording), _ptr(tables), _ptr(ws), nbytes, _ptr(mean), _ptr(std), _ptr(feats))
    return (feats, ws) if return_frames else feats


def _check_augment_operands(augment, noise, noise_lengths, audio):
    """The argument errors of the augmented call; ``(B, n_noise, noise_stride, noise_len_max)``."""
    dev = audio.device
    _check_input(augment, "augment")
    if augment.dtype != torch.int32 or augment.dim() != 2 or augment.shape[1] != 6 or augment.shape[0] < 1:
        raise RuntimeError("augment must be int32 records [B, 6] (got %s %s)" % (augment.dtype, tuple(augment.shape)))
    if augment.device != dev:
        raise RuntimeError("augment must be on the audio's device")
    if (noise is None) != (noise_lengths is None):
        raise RuntimeError("noise and noise_lengths go together")
    if noise is None:
        return augment.shape[0], 0, 1, 1
    if not isinstance(noise, torch.Tensor) or not noise.is_cuda or noise.device != dev:
        raise RuntimeError("noise must be a CUDA tensor on the audio's device")
    if noise.dtype != audio.dtype:
        raise RuntimeError("noise must have the audio's dtype %s (got %s)" % (audio.dtype, noise.dtype))
    if noise.dim() != 2 or noise.shape[0] < 1 or not 1 <= noise.shape[1] <= _lib.MFCC_NOISE_LEN_MAX:
        raise RuntimeError("noise must be [n_noise, noise_len_max] with 1 <= noise_len_max <= 2^24 (got %s)"
                           % (tuple(noise.shape),))
    if noise.stride(1) != 1 or (noise.shape[0] > 1 and noise.stride(0) < 1):
        raise RuntimeError("noise needs unit stride along the samples and a positive row stride (got strides %s)"
                           % (tuple(noise.stride()),))
    _check_input(noise_lengths, "noise_lengths")
    if noise_lengths.dtype != torch.int32 or noise_lengths.numel() != noise.shape[0] or noise_lengths.device != dev:
        raise RuntimeError("noise_lengths must be int32 [%d] on %s" % (noise.shape[0], dev))
    n_noise, nmax = noise.shape
    return augment.shape[0], n_noise, int(noise.stride(0)) if n_noise > 1 else nmax, nmax


class MFCCFrontend(nn.Module):
    """``MFCCProcessor`` (data_pipeline/mfccProcessor.py) + pad / cut + normalisation as a module in front of a model:
    ``forward(audio, lengths=None)`` is ``mfcc_features`` with this module's settings.  ``mean`` / ``std`` (``[F]``,
    persistent buffers: they travel with a checkpoint) and the constant tables (a non-persistent buffer, filled on the
    first call on a device -- call once before capturing a graph) live on the module's device."""

    def __init__(self, n_mfcc=32, feature_type="delta", width=9, max_len=99, top_db=80.0, mean=None, std=None,
                 peak_normalize=False, device=None):
        super().__init__()
        self.order = _order_of(feature_type)
        self.feature_type = feature_type
        self.n_mfcc, self.width, self.max_len = _check_settings(n_mfcc, self.order, width, max_len)
        self.top_db = top_db
        self.peak_normalize = bool(peak_normalize)
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together")
        self.register_buffer("mean", None)
        self.register_buffer("std", None)
        self.register_buffer("tables", None, persistent=False)
        if mean is not None:
            self.set_normalization(mean, std)
        if device is not None:
            self.to(device)

    @property
    def num_features(self):
        return self.n_mfcc * (self.order + 1)

    def set_normalization(self, mean, std):
        """``mean`` / ``std``: anything ``torch.as_tensor`` takes with ``F`` elements (the reference's ``mean.npy`` /
        ``std.npy`` are ``[1,F,1]``)."""
        dev = self.mean.device if self.mean is not None else (self.tables.device if self.tables is not None else None)
        mean = torch.as_tensor(mean).detach().to(torch.float32).reshape(-1).contiguous()
        std = torch.as_tensor(std).detach().to(torch.float32).reshape(-1).contiguous()
        if mean.numel() != self.num_features or std.numel() != self.num_features:
            raise ValueError("mean and std must hold %d values (got %d, %d)" % (self.num_features, mean.numel(), std.numel()))
        self.mean = mean.clone() if dev is None else mean.to(dev)
        self.std = std.clone() if dev is None else std.to(dev)

    def forward(self, audio, lengths=None, normalize=True, augment=None, noise=None, noise_lengths=None, check=True):
        """``audio:[B,L]`` on the device -> ``[B, max_len, F]``; ``normalize=False`` leaves ``mean`` / ``std`` out (the
        raw features ``fit_normalization`` takes).  ``augment`` (with ``noise`` / ``noise_lengths`` / ``check``): the
        augmented call of ``mfcc_features`` -- ``audio`` is the bank, the output has one clip per record."""
        if self.tables is None or self.tables.device != audio.device:
            self.tables = mfcc_tables(audio.device)
        use = normalize and self.mean is not None
        if use and self.mean.device != audio.device:        # (once: the statistics follow the audio's device)
            self.mean, self.std = self.mean.to(audio.device), self.std.to(audio.device)
        mean, std = (self.mean, self.std) if use else (None, None)
        return mfcc_features(audio, lengths, n_mfcc=self.n_mfcc, feature_type=self.feature_type, width=self.width,
                             max_len=self.max_len, top_db=self.top_db, mean=mean, std=std,
                             peak_normalize=self.peak_normalize, tables=self.tables, augment=augment, noise=noise,
                             noise_lengths=noise_lengths, check=check)

    def stream(self, recording, hop_samples=800, clip=16000, normalize=True, **chunk):
        """``forward(clips_of(recording, hop_samples, clip))`` with the recording's frames computed once
        (``mfcc_stream_features`` with this module's settings, normalisation and ``peak_normalize``): ``[B, max_len, F]``
        for the 1-D ``recording`` on the device.  ``hop_samples`` must be a multiple of 160 and ``clip`` 16000
        (``ValueError``).  ``chunk``: ``clip0`` / ``num_clips`` / ``frames`` / ``return_frames`` of
        ``mfcc_stream_features``, to score a long recording piece by piece."""
        if self.tables is None or self.tables.device != recording.device:
            self.tables = mfcc_tables(recording.device)
        use = normalize and self.mean is not None
        if use and self.mean.device != recording.device:
            self.mean, self.std = self.mean.to(recording.device), self.std.to(recording.device)
        mean, std = (self.mean, self.std) if use else (None, None)
        return mfcc_stream_features(recording, hop_samples, clip=clip, n_mfcc=self.n_mfcc, feature_type=self.feature_type,
                                    width=self.width, max_len=self.max_len, top_db=self.top_db, mean=mean, std=std,
                                    peak_normalize=self.peak_normalize, tables=self.tables, **chunk)

    @staticmethod
    def clips_of(recording, hop_samples=800, clip=16000):
        """The clips the live detector slides over a recording (inferencetry.py:88,169: the last ``clip`` samples every
        ``hop_samples`` = 50 ms) as a strided VIEW ``[B, clip]`` of the 1-D ``recording``: clip ``b`` is samples
        ``b * hop_samples .. b * hop_samples + clip - 1``, ``B = (N - clip) // hop_samples + 1``.  No copy: the rows
        overlap, which ``mfcc_features`` reads in place."""
        if recording.dim() != 1:
            raise ValueError("recording must be 1-D (got %d dimensions)" % recording.dim())
        hop_samples, clip = int(hop_samples), int(clip)
        if hop_samples < 1 or clip < 1:
            raise ValueError("hop_samples and clip must be positive (got %d, %d)" % (hop_samples, clip))
        N = recording.shape[0]
        if N < clip:
            raise ValueError("recording of %d samples is shorter than a clip of %d" % (N, clip))
        s = recording.stride(0)
        return recording.as_strided(((N - clip) // hop_samples + 1, clip), (hop_samples * s, s))

    @torch.no_grad()
    def fit_normalization(self, batches):
        """``compute_normalization_stats`` (preprocessing.py:60-66) over an iterable of RAW feature batches ``[..., F]``
        (``forward(audio, normalize=False)``; any device): population mean and standard deviation per feature over
        batch and time, ``std == 0 -> 1e-6``, reduced in fp64 batch by batch (means and centred sums of squares merged
        pairwise, so no ``E[x^2] - E[x]^2`` cancellation).  Sets and returns ``(mean, std)``."""
        Fn = self.num_features
        count, mean, m2 = 0, None, None
        for x in batches:
            if x.shape[-1] != Fn:
                raise ValueError("a batch of raw features must end in %d features (got shape %s)" % (Fn, tuple(x.shape)))
            x = x.reshape(-1, Fn).to(torch.float64)
            nb = x.shape[0]
            if nb == 0:
                continue
            mb = x.mean(dim=0)
            sb = ((x - mb) ** 2).sum(dim=0)
            if mean is None:
                count, mean, m2 = nb, mb, sb
            else:
                mb, sb = mb.to(mean.device), sb.to(mean.device)
                delta = mb - mean
                tot = count + nb
                mean = mean + delta * (nb / tot)
                m2 = m2 + sb + delta ** 2 * (count * nb / tot)
                count = tot
        if mean is None:
            raise ValueError("fit_normalization: no batches")
        std = torch.sqrt(m2 / count)
        std = torch.where(std == 0, torch.full_like(std, 1e-6), std)
        self.set_normalization(mean, std)
        return self.mean, self.std
