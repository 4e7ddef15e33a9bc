"""numpy model of the inverse STFT stage (include/afg.h: afg_istft_hip): the float64 definition as a direct sum -- no FFT --
and the interval the header states.

  x_f[j] = (1 / n_fft) (re_0 + [n_fft even] (-1)^j re_{n_fft/2} + 2 sum_{0 < k < n_fft/2} (re_k cos(2 pi k j / n_fft) - im_k sin(2 pi k j / n_fft)))
  N[t] = sum_f w[t - f hop - n_lo] x_f[t - f hop],  D[t] = sum_f w[t - f hop - n_lo]^2,  value N / D at t = pad + first + i;
  u = 2^-24, B = 8 ceil(log2 n_fft) + 8, m = ceil(win_length / hop), A'_f = (1 / n_fft) sum_k c_k (|re_k| + |im_k|),
  S[t] = sum_f w A'_f, E[t] = (B + 2 m + 8) u S[t] / D[t]."""
import functools
import math

import numpy as np

import melspec_fft_model as fm

U = fm.U

outside = fm.outside
used_fraction = fm.used_fraction


def n_bins(n_fft):
    return n_fft // 2 + 1


def window64(win_length):
    """the forward stage's window: periodic Hann (melspec_fft_model.fft_tables64's first part)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)


def real_only(n_fft):
    """the bins whose imaginary part takes no part"""
    return [0, n_fft // 2] if n_fft % 2 == 0 else [0]


@functools.lru_cache(maxsize=8)
def basis(n_fft):
    """(C, S, c): cos and sin of 2 pi k j / n_fft as [n_bins, n_fft] with the angle reduced in integers, and the weights c_k"""
    k = np.arange(n_bins(n_fft), dtype=np.int64)[:, None]
    j = np.arange(n_fft, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * j) % n_fft).astype(np.float64) / n_fft
    c = np.full(n_bins(n_fft), 2.0)
    c[real_only(n_fft)] = 1.0
    return np.cos(a), np.sin(a), c


def frames64(re, im, n_fft):
    """x_f[j] as [n_frames, n_fft] from re, im [n_bins, n_frames]; a NaN that is read makes NaN of its whole frame"""
    C, S, c = basis(n_fft)
    re = np.asarray(re, np.float64)
    im = np.array(im, np.float64)
    im[real_only(n_fft)] = 0.0                                   # not read
    with np.errstate(all="ignore"):
        return ((re * c[:, None]).T @ C - (im * c[:, None]).T @ S) / n_fft


def line64(re, im, n_fft, win_length, hop):
    """(N, D, S) over the whole line of n_fft + hop (n_frames - 1) samples"""
    w = window64(win_length)
    n_lo = (n_fft - win_length) // 2
    x = frames64(re, im, n_fft)
    F = x.shape[0]
    _, _, c = basis(n_fft)
    im0 = np.abs(np.array(im, np.float64))
    im0[real_only(n_fft)] = 0.0
    with np.errstate(all="ignore"):
        A = (c[:, None] * (np.abs(np.asarray(re, np.float64)) + im0)).sum(axis=0) / n_fft
    L = n_fft + hop * (F - 1)
    N, D, S = np.zeros(L), np.zeros(L), np.zeros(L)
    with np.errstate(all="ignore"):
        for f in range(F):                                       # ascending, as the device sums
            a = f * hop + n_lo
            N[a:a + win_length] += w * x[f, n_lo:n_lo + win_length]
            D[a:a + win_length] += w * w
            S[a:a + win_length] += w * A[f]
    return N, D, S


def envelope(n_fft, win_length, hop, n_frames):
    """D over the whole line"""
    w = window64(win_length)
    n_lo = (n_fft - win_length) // 2
    D = np.zeros(n_fft + hop * (n_frames - 1))
    for f in range(n_frames):
        D[f * hop + n_lo:f * hop + n_lo + win_length] += w * w
    return D


def delivered(n_fft, center, first, count):
    pad = n_fft // 2 if center else 0
    return slice(pad + first, pad + first + count)


def bound_k(n_fft, win_length, hop):
    return fm.bound_b(n_fft) + 2 * math.ceil(win_length / hop) + 8


def interval(re, im, n_fft, win_length, hop, center, first, count):
    """(lo, hi, mid) of the `count` delivered samples from `first`, float64; NaN in all three under a frame with a NaN read"""
    N, D, S = line64(re, im, n_fft, win_length, hop)
    s = delivered(n_fft, center, first, count)
    assert s.stop <= len(N)
    with np.errstate(all="ignore"):
        mid = N[s] / D[s]
        E = bound_k(n_fft, win_length, hop) * U * S[s] / D[s]
    return mid - E, mid + E, mid


def istft64(re, im, n_fft, win_length, hop, center, first, count):
    return interval(re, im, n_fft, win_length, hop, center, first, count)[2]
