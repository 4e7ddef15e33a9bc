"""numpy model of the FFT path of the mel spectrogram features (include/afg.h: afg_mel_fft_tables, afg_melspec_fft_hip): the
table in float64, and the interval the header states for the output, computed from tests/melspec_model.py's float64
definition (basis64, power64, filters64's bank as the library rounded it).

  u = 2^-24, A_f = sum |x_n| w[n] of frame f, B = 8 ceil(log2 n_fft) + 8, E_f = B u A_f bounds |re - re64| and |im - im64|;
  p_hi = (|re64| + E)^2 + (|im64| + E)^2, p_lo = max(|re64| - E, 0)^2 + max(|im64| - E, 0)^2;
  AFG_MEL_POWER lies in [(1 - (n_bins + 4) u) W p_lo, (1 + (n_bins + 4) u) W p_hi] (weights >= 0), AFG_MEL_LOG10 within
  3 float32 ulp of log10 of that interval after the floor."""
import math

import numpy as np

import melspec_model as mm

U = 2.0 ** -24


def fft_tables64(n_fft, win_length):
    """(w [win_length], tw [n_fft, 2]) in float64: the periodic Hann window, and (cos, -sin) of 2 pi j / n_fft"""
    j = np.arange(win_length, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win_length)
    a = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return w, np.stack([np.cos(a), -np.sin(a)], axis=1)


def fft_tables32(n_fft, win_length):
    """afg_mel_fft_tables' layout: win_length window floats, then n_fft pairs, each rounded once"""
    w, tw = fft_tables64(n_fft, win_length)
    return np.concatenate([w, tw.reshape(-1)]).astype(np.float32)


def supported(n_fft):
    if not 16 <= n_fft <= 2048:
        return False
    for q in (2, 3, 5):
        while n_fft % q == 0:
            n_fft //= q
    return n_fft == 1


def bound_b(n_fft):
    return 8 * math.ceil(math.log2(n_fft)) + 8


def spectrum64(x, n_fft, win_length, hop, center, pad_mode, n_frames):
    """(re64, im64, E), each [n_bins, n_frames] (E broadcast over the bins), of a float32 row"""
    x = np.ascontiguousarray(x, np.float32)
    C, S = mm.basis64(n_fft, win_length)
    with np.errstate(all="ignore"):
        re, im, _, _, _ = mm.power64(x, C, S, n_fft, win_length, hop, center, pad_mode, n_frames)
        w, _ = fft_tables64(n_fft, win_length)
        fr = mm.frames_of(x.astype(np.float64), n_fft, win_length, hop, center, pad_mode, n_frames)
        A = np.abs(fr) @ w
    return re, im, np.broadcast_to(bound_b(n_fft) * U * A[None, :], re.shape)


def power_interval(x, bank32, n_fft, win_length, hop, center, pad_mode, n_frames):
    """(lo, hi, mid), each [n_mels, n_frames] float64: the AFG_MEL_POWER interval and the float64 value itself.  A frame with a
    NaN sample under it is NaN in all three."""
    re, im, E = spectrum64(x, n_fft, win_length, hop, center, pad_mode, n_frames)
    W = np.asarray(bank32, np.float32).astype(np.float64)
    assert (W >= 0).all()
    nb = mm.n_bins(n_fft)
    with np.errstate(all="ignore"):
        p_hi = (np.abs(re) + E) ** 2 + (np.abs(im) + E) ** 2
        p_lo = np.maximum(np.abs(re) - E, 0.0) ** 2 + np.maximum(np.abs(im) - E, 0.0) ** 2
        p_lo = np.where(np.isnan(re) | np.isnan(im), np.nan, p_lo)
        return (1.0 - (nb + 4) * U) * (W @ p_lo), (1.0 + (nb + 4) * U) * (W @ p_hi), W @ (re * re + im * im)


def log_interval(lo, hi, log_floor=0.0):
    """the AFG_MEL_LOG10 interval of a power interval: log10 after the float32 floor, widened by 3 float32 ulp"""
    floor = np.float64(np.float32(log_floor if log_floor else 1e-10))
    with np.errstate(all="ignore"):
        a, b = np.log10(np.maximum(lo, floor)), np.log10(np.maximum(hi, floor))
    ulp = lambda v: np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)
    return a - 3.0 * ulp(a), b + 3.0 * ulp(b)


def outside(got, lo, hi):
    """indexes of the float32 values that are not inside [lo, hi] (a NaN anywhere counts)"""
    g = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.argwhere(~((g >= lo) & (g <= hi)))


def used_fraction(got, lo, hi, mid):
    """the largest deviation from the float64 value as a fraction of the interval's half-width (power values)"""
    g = np.asarray(got, np.float32).astype(np.float64)
    half = (hi - lo) / 2.0
    ok = half > 0
    return float((np.abs(g - mid)[ok] / half[ok]).max()) if ok.any() else 0.0
