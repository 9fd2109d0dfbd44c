"""Numpy restatements for the device-side augmentation (include/fastgrnn_hip.h: fastgrnn_hip_mfcc_augment,
fastgrnn_hip_augment_draw): the sample definition in fp32 with three separately rounded operations, Philox4x32-10, the
draw, and builders for records outside their ranges with the clamped records the header defines for them.

A record is a row ``(src, shift, noise, noise_off, gain bits, noise_gain bits)`` of an int32 ``[B, 6]`` array."""
import numpy as np

MINLEN, SHIFT_CAP = 1280, 1 << 20
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


# ---- records -----------------------------------------------------------------------------------------------------------
def pack(src, shift, gain, noise=-1, noise_off=0, noise_gain=0.0):
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    B = len(src)
    col = lambda v, dt: np.broadcast_to(np.asarray(v, dtype=dt), (B,))
    rec = np.empty((B, 6), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = src, col(shift, np.int64), col(noise, np.int64), col(noise_off, np.int64)
    rec[:, 4] = col(gain, np.float32).copy().view(np.int32)
    rec[:, 5] = col(noise_gain, np.float32).copy().view(np.int32)
    return rec


def gains(rec):
    rec = np.ascontiguousarray(rec)
    return rec[:, 4].copy().view(np.float32), rec[:, 5].copy().view(np.float32)


def as_samples(y):
    y = np.asarray(y)
    return y.astype(np.float32) * np.float32(2.0 ** -15) if y.dtype == np.int16 else y.astype(np.float32)


def clip_length(lengths, src, L):
    return L if lengths is None else int(min(max(int(lengths[src]), MINLEN), L))


# ---- the sample definition ---------------------------------------------------------------------------------------------
def augment_clip(bank, lengths, record, noises):
    """``(y', len)`` for ONE record with every field in its range: ``y'`` float32 ``[L]``, zero from ``len`` on.
    ``bank``: ``[N, L]`` float32 or int16; ``noises``: a list of 1-D arrays of the bank's dtype (their true lengths)."""
    src, shift, noise, off = (int(v) for v in record[:4])
    gain, ngain = (g[0] for g in gains(np.asarray(record)[None]))
    L = bank.shape[1]
    n = clip_length(lengths, src, L)
    y = as_samples(bank[src][:n])
    i = np.arange(n)
    q = i - shift                                                   # (Python integers: no overflow)
    ok = (q >= 0) & (q < n)
    shifted = np.where(ok, y[np.clip(q, 0, n - 1)], np.float32(0))
    out = (np.float32(gain) * shifted).astype(np.float32)           # one rounding
    if noise >= 0:
        nz = as_samples(noises[noise])
        term = (np.float32(ngain) * nz[(off + i) % len(nz)]).astype(np.float32)      # one rounding
        out = (out + term).astype(np.float32)                       # one rounding
    full = np.zeros(L, dtype=np.float32)
    full[:n] = out
    return full, n


def augment_batch(bank, lengths, records, noises):
    """``([B, L] float32, [B] int32 lengths)`` of in-range records."""
    ys, ns = zip(*(augment_clip(bank, lengths, r, noises) for r in records))
    return np.stack(ys), np.asarray(ns, dtype=np.int32)


def clamp_records(records, n_clips, noise_lengths, noise_len_max):
    """The in-range records that define the result of arbitrary ones: ``src`` into ``0..n_clips-1``, ``shift`` into
    ``+-2^20`` (beyond 16 000 every value empties the clip alike), ``noise`` to below the number of noises (none if
    there are no noises), ``noise_off`` to its non-negative remainder mod the noise's (clamped) length."""
    out = np.array(records, dtype=np.int32, copy=True)
    n_noise = 0 if noise_lengths is None else len(noise_lengths)
    for r in out:
        r[0] = min(max(int(r[0]), 0), n_clips - 1)
        r[1] = min(max(int(r[1]), -SHIFT_CAP), SHIFT_CAP)
        if r[2] >= 0 and n_noise > 0:
            r[2] = min(int(r[2]), n_noise - 1)
            nlen = min(max(int(noise_lengths[r[2]]), 1), noise_len_max)
            r[3] = int(r[3]) % nlen                                  # (Python's %: the non-negative remainder)
        elif r[2] >= 0:
            r[2] = -1
    return out


def hostile_records(n_clips, n_noise):
    """Records outside their ranges: src -1 and N, noise = n_noise, a negative and a huge noise_off, shift at both ends
    of int32.  Every one with a noise (where there are noises) and gains that leave both terms visible."""
    imax, imin = 2 ** 31 - 1, -2 ** 31
    rows = [(-1, 0, 0, 0), (n_clips, 3, 1, 2), (-(2 ** 31), 0, 0, 0), (imax, -7, 1, 1),
            (1, 0, n_noise, 0), (2, 5, imax, 3), (3, 0, 0, -1), (4, 0, 1, -5), (5, 0, 2, imax), (6, 0, 2, imin),
            (7, imax, 0, 0), (8, imin + 1, 1, 0), (9, imin, 2, 4), (n_clips + 5, imax, n_noise + 9, imin)]
    a = np.asarray(rows, dtype=np.int64)
    return pack(a[:, 0], a[:, 1], 0.75, a[:, 2], a[:, 3], 0.5)


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------
def philox(counter, key):
    """``counter``: four uint32 arrays (or scalars), ``key``: two -> four uint32 arrays.  Ten rounds; the key is bumped
    by the Weyl constants between rounds."""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & np.uint64(0xFFFFFFFF), p1 >> np.uint64(32), p1 & np.uint64(0xFFFFFFFF)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def _unit(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)          # exact


def _below(x, n):
    return ((x.astype(np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _between(lo, hi, u):
    lo, hi = np.float32(lo), np.float32(hi)
    return (lo + ((hi - lo).astype(np.float32) * u).astype(np.float32)).astype(np.float32)


def draw(seed, step, index, p_augment=0.25, max_shift=0, gain=(1.0, 1.0), p_noise=0.5, noise_gain=(0.1, 0.1),
         noise_lengths=None, noise_len_max=1):
    """The records ``[B, 6]`` of ``fastgrnn_hip_augment_draw``."""
    index = np.asarray(index, dtype=np.int32)
    B = len(index)
    b = np.arange(B, dtype=np.uint32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    s_lo, s_hi = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    x = philox((b, s_lo, s_hi, 0), key) + philox((b, s_lo, s_hi, 1), key)
    n_noise = 0 if noise_lengths is None else len(noise_lengths)
    aug = _unit(x[0]) < np.float32(p_augment)
    shift = _below(x[1], 2 * max_shift + 1) - max_shift
    g = _between(gain[0], gain[1], _unit(x[2]))
    with_noise = aug & (n_noise > 0) & (_unit(x[3]) < np.float32(p_noise))
    if n_noise:
        noise = _below(x[4], n_noise)
        nlen = np.clip(np.asarray(noise_lengths, dtype=np.int64), 1, noise_len_max)[noise]
        off = _below(x[5], nlen)
    else:
        noise = off = np.zeros(B, dtype=np.int64)
    ng = _between(noise_gain[0], noise_gain[1], _unit(x[6]))
    return pack(index, np.where(aug, shift, 0), np.where(aug, g, np.float32(1)), np.where(with_noise, noise, -1),
                np.where(with_noise, off, 0), np.where(with_noise, ng, np.float32(0)))
