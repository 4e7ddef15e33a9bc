"""numpy model of the mel spectrogram features of include/afg.h (afg_mel_basis, afg_mel_filters, afg_melspec_hip,
afg_batch_decode_mel): the float64 definition of the tables and of the power spectrum, and the float32 restatement of the
kernel's sums -- every sum a chain of fmaf from +0.0f in ascending index order -- on an exact float32 fmaf.

fmaf32: the product of two float32 is exact in float64 (48 bits); the sum with c is rounded to float64 once, TwoSum gives
what that rounding lost, and where it lost something the float64 sum is moved to its neighbour with an odd last bit
(round to odd).  Narrowing a round-to-odd float64 (53 bits >= 24 + 2) to float32 rounds the exact value once."""
import numpy as np

PAD_REFLECT, PAD_ZERO = 0, 1
POWER, LOG10 = 0, 1
SCALE_SLANEY, SCALE_HTK = 0, 1
NORM_NONE, NORM_SLANEY = 0, 1


def fmaf32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded (non-finite results: whatever IEEE gives a * b + c)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                            # exact
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                        # s + e == p + c exactly
        odd = (s.view(np.int64) & 1) != 0
        fix = np.isfinite(s) & (e != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def naive_fma32(a, b, c):
    """float32(a * b + c) through float64: two roundings, wrong now and then (tests/test_melspec_model.py has triples)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        return (a * b + c).astype(np.float32)


def n_bins(n_fft):
    return n_fft // 2 + 1


def nb16(n_fft):
    return (n_bins(n_fft) + 15) // 16 * 16


def basis64(n_fft, win_length):
    """(C, S) in float64, [win_length, n_bins]: row j is sample n_lo + j of a frame"""
    n_lo = (n_fft - win_length) // 2
    j = np.arange(win_length, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j.astype(np.float64) / win_length)
    k = np.arange(n_bins(n_fft), dtype=np.int64)
    a = 2.0 * np.pi * (((n_lo + j)[:, None] * k[None, :]) % n_fft).astype(np.float64) / n_fft
    return w[:, None] * np.cos(a), -w[:, None] * np.sin(a)


def split_basis(table, n_fft):
    """afg_mel_basis's table [win_length, 2 * nb16] -> (C, S) float32 [win_length, n_bins]; the padding columns must be +0.0f"""
    nb, n16 = n_bins(n_fft), nb16(n_fft)
    assert table.shape[1] == 2 * n16
    pad = np.concatenate([table[:, nb:n16], table[:, n16 + nb:]], axis=1)
    assert (pad.view(np.uint32) == 0).all()
    return np.ascontiguousarray(table[:, :nb]), np.ascontiguousarray(table[:, n16:n16 + nb])


def hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == SCALE_HTK:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-300) / 1000.0) / np.log(6.4))


def mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == SCALE_HTK:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp(np.log(6.4) * (m - 15.0) / 27.0))


def mel_points(samplerate, n_mels, f_min=0.0, f_max=0.0, scale=SCALE_SLANEY):
    """f[0 .. n_mels + 1] in Hz"""
    f_max = f_max or samplerate / 2.0
    lo, hi = float(hz_to_mel(f_min, scale)), float(hz_to_mel(f_max, scale))
    return mel_to_hz(lo + (hi - lo) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1), scale)


def filters64(samplerate, n_fft, n_mels, f_min=0.0, f_max=0.0, scale=SCALE_SLANEY, norm=NORM_SLANEY):
    """the bank in float64, [n_mels, n_bins]"""
    f = mel_points(samplerate, n_mels, f_min, f_max, scale)
    fk = np.arange(n_bins(n_fft), dtype=np.float64) * samplerate / n_fft
    up = (fk[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    down = (f[2:, None] - fk[None, :]) / (f[2:] - f[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(up, down))
    if norm == NORM_SLANEY:
        w = w * (2.0 / (f[2:] - f[:-2]))[:, None]
    return w


def max_frames(in_frames, n_fft, hop, center):
    num = in_frames + 2 * (n_fft // 2 if center else 0) - n_fft
    return 0 if num < 0 else 1 + num // hop


def frames_of(x, n_fft, win_length, hop, center, pad_mode, n_frames):
    """[n_frames, win_length]: the samples under the window of every frame, reflected or +0.0f outside the row"""
    x = np.asarray(x)
    pad = n_fft // 2 if center else 0
    n_lo = (n_fft - win_length) // 2
    idx = (np.arange(n_frames, dtype=np.int64) * hop)[:, None] + (n_lo - pad + np.arange(win_length, dtype=np.int64))[None, :]
    if pad_mode == PAD_REFLECT:
        assert n_frames == 0 or pad == 0 or len(x) > pad
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= len(x), 2 * (len(x) - 1) - idx, idx)
    ok = (idx >= 0) & (idx < len(x))
    if len(x) == 0:
        return np.zeros(idx.shape, x.dtype)
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], x.dtype.type(0))


def power64(x, C, S, n_fft, win_length, hop, center, pad_mode, n_frames):
    """the definition in float64: (re, im, p, sum |x C|, sum |x S|), each [n_bins, n_frames]"""
    fr = frames_of(np.asarray(x, np.float64), n_fft, win_length, hop, center, pad_mode, n_frames)
    C, S = np.asarray(C, np.float64), np.asarray(S, np.float64)
    re, im = (fr @ C).T, (fr @ S).T
    return re, im, re * re + im * im, (np.abs(fr) @ np.abs(C)).T, (np.abs(fr) @ np.abs(S)).T


def chain32(A, B):
    """[M, K] x [K, N] -> [M, N], every element the fmaf chain over k = 0 .. K - 1 of fmaf(A[m][k], B[k][n], acc) from +0.0f"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = fmaf32(A[:, k][:, None], B[k][None, :], acc)
    return acc


def melspec32(x, C, S, Wm, n_fft, win_length, hop, center, pad_mode, n_frames):
    """the kernel's sums in float32: (p [n_bins, n_frames], mel [n_mels, n_frames]) with AFG_MEL_POWER"""
    fr = frames_of(np.ascontiguousarray(x, np.float32), n_fft, win_length, hop, center, pad_mode, n_frames)
    with np.errstate(all="ignore"):
        re, im = chain32(fr, C), chain32(fr, S)              # [n_frames, n_bins]
        p = fmaf32(im, im, (re * re).astype(np.float32)).T
        return p, chain32(Wm, p)


def log10_64(mel, log_floor=0.0):
    """float64 log10 of the float32 fmaxf(mel, floor): what AFG_MEL_LOG10's log10f approximates"""
    floor = np.float32(log_floor if log_floor else 1e-10)
    return np.log10(np.fmax(np.asarray(mel, np.float32), floor).astype(np.float64))


def same_bits(got, want):
    """indexes where two float32 arrays differ: bit for bit, except that where `want` is NaN any NaN will do"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.argwhere(np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32)))
