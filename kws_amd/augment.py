"""Augmentation of raw audio on the device, inside the MFCC front end.

The reference augments once, on the host, and writes the copies to disk (data_pipeline/audioAugmentation.py: a quarter
of the training files, background noise at gain 0.1 wrapped to the clip's length; preprocessing.py:13 lists time
shifting as a to-do).  Here the dataset stays on the device as an audio bank ``[N, L]`` (fp32 samples or int16 PCM), a
batch is a vector of clip indices, and every clip of every batch gets a fresh augmentation:

* a RECORD per output clip says what to read: ``(src, shift, noise, noise_off, gain, noise_gain)``, a ``[B, 6]`` int32
  tensor whose two last columns hold float bits (``pack_augment`` / ``unpack_augment``; the C struct
  ``fastgrnn_mfcc_aug``).  Output sample ``i`` of a clip of ``len`` samples is
  ``gain * y[i - shift] + noise_gain * nz[(noise_off + i) mod nlen]``, ``y`` zero outside ``0..len-1``, the noise term
  absent for ``noise < 0`` (include/fastgrnn_hip.h spells out the roundings and the clamps);
* ``mfcc_features(bank, lengths, augment=records, noise=..., noise_lengths=...)`` applies the records while the kernel
  loads the clip -- the augmented audio is never written;
* ``AudioAugment.draw(index, step_t)`` fills the records on the device from Philox4x32-10 keyed by ``(seed, step,
  clip)``: no host random numbers, so a captured graph draws new augmentations at every replay;
* ``AudioAugment.apply`` is the same definition in plain torch ops, materialising ``[B, L]``: the unfused chain, for
  comparison and for users of the augmented audio itself.

Time stretch and pitch shift (librosa's phase vocoder and resampler) are not built.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib
from .fastgrnn_cuda import _call, _check_input, _ptr

_SHIFT_CAP = 1 << 20                # the kernel's cap on |shift|: 16 000 already empties a clip


def _column(v, B, dtype, device, name):
    t = torch.as_tensor(v, device=device)
    if t.dim() == 0:
        t = t.expand(B)
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError("%s must be a scalar or hold %d values (got shape %s)" % (name, B, tuple(t.shape)))
    return t.to(dtype)


def pack_augment(src, shift, gain, noise=None, noise_off=None, noise_gain=None):
    """Records ``[B, 6]`` int32 on ``src``'s device from columns (tensors of ``B`` values, or scalars): ``src`` the bank
    clip, ``shift`` in samples, ``gain``; ``noise`` the noise row (default -1: none), ``noise_off`` its first sample
    (default 0), ``noise_gain`` (default 0).  The two gains are float32, bit-cast into their columns."""
    src = torch.as_tensor(src)
    if src.dim() != 1 or src.shape[0] < 1:
        raise ValueError("src must be a 1-D tensor of clip indices (got shape %s)" % (tuple(src.shape),))
    B, dev = src.shape[0], src.device
    ints = [_column(v, B, torch.int32, dev, n) for v, n in
            ((src, "src"), (shift, "shift"), (-1 if noise is None else noise, "noise"),
             (0 if noise_off is None else noise_off, "noise_off"))]
    flts = [_column(v, B, torch.float32, dev, n).contiguous().view(torch.int32) for v, n in
            ((gain, "gain"), (0.0 if noise_gain is None else noise_gain, "noise_gain"))]
    return torch.stack(ints + flts, dim=1).contiguous()


def unpack_augment(records):
    """``pack_augment``'s inverse: ``(src, shift, gain, noise, noise_off, noise_gain)``, the gains as float32."""
    if records.dim() != 2 or records.shape[1] != 6 or records.dtype != torch.int32:
        raise ValueError("records must be int32 [B, 6] (got %s %s)" % (records.dtype, tuple(records.shape)))
    r = records.contiguous()
    f = r.view(torch.float32)
    return r[:, 0], r[:, 1], f[:, 4], r[:, 2], r[:, 3], f[:, 5]


def _pair(v, name):
    lo, hi = (v, v) if isinstance(v, (int, float)) else v
    lo, hi = float(lo), float(hi)
    if not (lo <= hi and abs(lo) != float("inf") and abs(hi) != float("inf")):
        raise ValueError("%s must be a finite value or a finite (lo, hi) with lo <= hi (got %r)" % (name, v))
    return lo, hi


class AudioAugment(nn.Module):
    """The augmentation settings, the noise bank and the seed in front of an ``MFCCFrontend``.

    ``p_augment``: the probability that a clip is augmented at all (the reference's ``augmentation_fraction`` 0.25);
    an augmented clip gets a shift uniform in ``-max_shift..max_shift`` samples, a gain uniform in ``gain`` (a value or
    ``(lo, hi)``) and, with probability ``p_noise`` (the reference's coin, 0.5), a noise of the bank from a uniform
    offset at a gain uniform in ``noise_gain`` (the reference's 0.1).  ``seed``: 64 bits.  The noise bank and its lengths
    are persistent buffers (``noise:[n_noise, noise_len_max]`` padded with zeros, ``noise_lengths`` int32): they travel
    with a checkpoint and with ``.to(device)``.  Construction and ``set_noise`` need no GPU; ``draw`` does."""

    def __init__(self, p_augment=0.25, max_shift=0, gain=1.0, p_noise=0.5, noise_gain=0.1, seed=0, noises=None,
                 device=None):
        super().__init__()
        self.p_augment, self.p_noise = float(p_augment), float(p_noise)
        for p, n in ((self.p_augment, "p_augment"), (self.p_noise, "p_noise")):
            if not 0.0 <= p <= 1.0:
                raise ValueError("%s must be a probability (got %r)" % (n, p))
        self.max_shift = int(max_shift)
        if not 0 <= self.max_shift <= _lib.AUGMENT_MAX_SHIFT:
            raise ValueError("max_shift must be in 0..2^20 samples (got %d)" % self.max_shift)
        self.gain = _pair(gain, "gain")
        self.noise_gain = _pair(noise_gain, "noise_gain")
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must fit 64 bits (got %d)" % self.seed)
        self.register_buffer("noise", None)
        self.register_buffer("noise_lengths", None)
        if noises is not None:
            self.set_noise(noises)
        if device is not None:
            self.to(device)

    @property
    def n_noise(self):
        return 0 if self.noise is None else self.noise.shape[0]

    def set_noise(self, noises):
        """``noises``: a list of 1-D tensors of one dtype (float32 samples or int16 PCM -- the audio bank's), each of
        1 to 2^24 samples.  Pads them with zeros into ``noise:[n_noise, noise_len_max]`` and keeps their lengths; an
        empty list removes the bank."""
        noises = [torch.as_tensor(z) for z in noises]
        if not noises:
            self.noise = self.noise_lengths = None
            return
        dev = self.noise.device if self.noise is not None else None
        dtype = noises[0].dtype
        if dtype not in (torch.float32, torch.int16):
            raise ValueError("noises must be float32 samples or int16 PCM (got %s)" % dtype)
        for z in noises:
            if z.dim() != 1 or z.dtype != dtype or not 1 <= z.shape[0] <= _lib.MFCC_NOISE_LEN_MAX:
                raise ValueError("every noise must be a 1-D %s tensor of 1 to 2^24 samples (got %s %s)"
                                 % (dtype, z.dtype, tuple(z.shape)))
        nmax = max(z.shape[0] for z in noises)
        bank = torch.zeros((len(noises), nmax), dtype=dtype)
        for k, z in enumerate(noises):
            bank[k, :z.shape[0]] = z.detach().cpu()
        lens = torch.tensor([z.shape[0] for z in noises], dtype=torch.int32)
        self.noise = bank if dev is None else bank.to(dev)
        self.noise_lengths = lens if dev is None else lens.to(dev)

    def _ranges(self):
        return _lib.AugmentRanges(self.p_augment, self.p_noise, self.max_shift, 0, self.gain[0], self.gain[1],
                                  self.noise_gain[0], self.noise_gain[1])

    def draw(self, index, step_t):
        """Records ``[B, 6]`` for the clips ``index:[B]`` (int32 on the device; copied to ``src``) at step
        ``step_t[0]`` (an int64 DEVICE scalar that is only read, e.g. a fused optimizer's ``step_t``): one library
        call, nothing drawn on the host, nothing synchronises.  Record ``b`` depends on ``(seed, step, b)`` alone."""
        _check_input(index, "index")
        _check_input(step_t, "step_t")
        if index.dim() != 1 or index.shape[0] < 1 or index.dtype != torch.int32:
            raise RuntimeError("index must be a 1-D int32 tensor of clip indices (got %s %s)"
                               % (index.dtype, tuple(index.shape)))
        if step_t.dtype != torch.int64 or step_t.numel() != 1 or step_t.device != index.device:
            raise RuntimeError("step_t must be one int64 on the index's device")
        dev = index.device
        if self.noise is not None and self.noise_lengths.device != dev:
            raise RuntimeError("the noise bank is on %s, the index on %s" % (self.noise_lengths.device, dev))
        B = index.shape[0]
        ranges = self._ranges()
        with torch.cuda.device(dev):
            rec = torch.empty((B, 6), dtype=torch.int32, device=dev)
            _call(_lib.load().fastgrnn_hip_augment_draw, "fastgrnn augment_draw", "augment_draw", dev, None, B,
                  C.c_uint64(self.seed), _ptr(step_t), _ptr(index), C.byref(ranges), self.n_noise,
                  self.noise.shape[1] if self.noise is not None else 1, _ptr(self.noise_lengths), _ptr(rec))
        return rec

    def apply(self, audio, lengths, records):
        """The augmented clips themselves, ``[B, L]`` float32: the definition of ``fastgrnn_hip_mfcc_augment`` in plain
        torch ops (gathers, two multiplies, one add, each rounded on its own), with the same clamps.  ``audio``: the bank
        ``[N, L]`` (float32 or int16, on any device), ``lengths``: ``[N]`` or None.  Samples past a clip's length are
        zero; the clip's length is ``lengths[src]``.  ``mfcc_features(apply(...), lengths[src])`` is the unfused chain
        and gives the bits of the fused call."""
        N, L = audio.shape
        dev = audio.device
        src, shift, gain, noise, off, ngain = unpack_augment(records.to(dev))
        src = src.clamp(0, N - 1).long()
        shift = shift.clamp(-_SHIFT_CAP, _SHIFT_CAP).long()
        if lengths is None:
            length = torch.full_like(src, L)
        else:
            length = lengths.to(dev)[src].clamp(_lib.MFCC_MIN_SAMPLES, L).long()
        i = torch.arange(L, device=dev)
        zero = torch.zeros((), dtype=torch.float32, device=dev)

        def samples(bank, rows, cols):
            v = bank[rows[:, None], cols]
            return v.to(torch.float32) * (1.0 / 32768.0) if bank.dtype == torch.int16 else v.to(torch.float32)

        q = i[None, :] - shift[:, None]
        y = samples(audio, src, q.clamp(0, L - 1))
        y = torch.where((q >= 0) & (q < length[:, None]), y, zero)
        out = gain[:, None] * y
        if self.noise is not None:
            bank, n_noise = self.noise.to(dev), self.noise.shape[0]
            row = noise.clamp(0, n_noise - 1).long()
            nlen = self.noise_lengths.to(dev)[row].clamp(1, bank.shape[1]).long()
            k = (torch.remainder(off.long(), nlen)[:, None] + i[None, :]) % nlen[:, None]
            mixed = out + ngain[:, None] * samples(bank, row, k)
            out = torch.where((noise >= 0)[:, None], mixed, out)
        return torch.where(i[None, :] < length[:, None], out, zero)
