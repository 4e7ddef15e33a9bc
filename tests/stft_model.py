"""numpy model of the linear spectrogram stage (include/afg.h: afg_stft_hip): the interval the header states for each of
the four kinds, computed from tests/melspec_fft_model.py's spectrum64 -- the float64 definition (basis64, power64 of
tests/melspec_model.py) and E_f = B u A_f.

  COMPLEX    [re64 - E, re64 + E] and [im64 - E, im64 + E], stacked on a last axis of 2 (re first, as the device lays pairs);
  POWER      [(1 - 4u) p_lo, (1 + 4u) p_hi], p_hi = (|re64| + E)^2 + (|im64| + E)^2, p_lo = max(|re64| - E, 0)^2 + max(|im64| - E, 0)^2;
  MAGNITUDE  the square root of that interval, widened by 2 float32 ulp;
  LOG10      log10 of that interval after the float32 floor, widened by 3 float32 ulp (melspec_fft_model.log_interval)."""
import numpy as np

import melspec_fft_model as fm
import melspec_model as mm

COMPLEX, MAGNITUDE, POWER, LOG10 = 0, 1, 2, 3
KIND_NAMES = {COMPLEX: "complex", MAGNITUDE: "magnitude", POWER: "power", LOG10: "log10"}
U = fm.U

outside = fm.outside
used_fraction = fm.used_fraction


def comps(kind):
    return 2 if kind == COMPLEX else 1


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64).astype(np.float32))).astype(np.float64)


def power_bounds(re, im, E):
    """(lo, hi) of AFG_STFT_POWER; NaN in both where a NaN sample lies under the frame"""
    with np.errstate(all="ignore"):
        p_hi = (np.abs(re) + E) ** 2 + (np.abs(im) + E) ** 2
        p_lo = np.maximum(np.abs(re) - E, 0.0) ** 2 + np.maximum(np.abs(im) - E, 0.0) ** 2
        p_lo = np.where(np.isnan(re) | np.isnan(im), np.nan, p_lo)
    return (1.0 - 4.0 * U) * p_lo, (1.0 + 4.0 * U) * p_hi


def interval(kind, x, n_fft, win_length, hop, center, pad_mode, n_frames, log_floor=0.0, spectrum=None):
    """(lo, hi, mid) of a float32 row for one kind: [n_bins, n_frames] float64, with a last axis of 2 for COMPLEX.  mid is the
    float64 value itself (LOG10: of the floored power).  spectrum: spectrum64 of the same arguments, when the caller has it."""
    re, im, E = spectrum if spectrum is not None else fm.spectrum64(x, n_fft, win_length, hop, center, pad_mode, n_frames)
    if kind == COMPLEX:
        mid = np.stack([re, im], axis=-1)
        e = np.stack([E, E], axis=-1)
        return mid - e, mid + e, mid
    lo, hi = power_bounds(re, im, E)
    with np.errstate(all="ignore"):
        p = re * re + im * im
        if kind == POWER:
            return lo, hi, p
        if kind == MAGNITUDE:
            a, b = np.sqrt(lo), np.sqrt(hi)
            return a - 2.0 * ulp32(a), b + 2.0 * ulp32(b), np.sqrt(p)
        assert kind == LOG10
        a, b = fm.log_interval(lo, hi, log_floor)
        return a, b, np.log10(np.maximum(p, np.float64(np.float32(log_floor if log_floor else 1e-10))))


def floor_value(log_floor=0.0):
    """log10 of the float32 floor, in float64: what AFG_STFT_LOG10 gives silence to within 3 float32 ulp"""
    return float(np.log10(np.float64(np.float32(log_floor if log_floor else 1e-10))))
