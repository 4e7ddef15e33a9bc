"""The convolution stage (include/afg.h: afg_convolve_*) in float64: the definition, the float32 restatement of the direct
path (one fused multiply-add per tap, ascending), S[b] of the FFT path's bound and the interval it gives."""
import numpy as np

import melspec_fft_model as fm

U = 2.0 ** -24
B = 1024                                                         # AFG_CONV_BLOCK
B_F = 8 * 11 + 8                                                 # per transform of 2048: 8 ceil(log2 n_fft) + 8
MAX_TAPS, DIRECT_MAX, DIRECT_TILE, TABLE_FLOATS, SPEC_FLOATS = 65536, 128, 4096, 4096, 2050

outside = fm.outside
used_fraction = fm.used_fraction


def partitions(taps):
    return -(-taps // B)


def bound_c(taps):
    """C of E[b] = C u S[b], counted in include/afg.h"""
    return 6 * B_F + 2 * partitions(taps) + 11


def line64(x, h):
    """y[n], n = 0 .. frames + taps - 2, in float64 from float32 data: the terms of each sample added in ascending k"""
    x, h = np.asarray(x, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    y = np.zeros(len(x) + len(h) - 1)
    if len(x) <= len(h):                                         # one pass per value of the shorter side; the order inside a sample is k's either way
        for m in range(len(x)):
            with np.errstate(invalid="ignore"):
                y[m:m + len(h)] += h * x[m]
    else:
        for k in range(len(h)):
            with np.errstate(invalid="ignore"):
                y[k:k + len(x)] += h[k] * x
    return y


def mode_range(mode, frames, taps, first=0):
    """(out_first, out_frames) of "full", "same" and "head" """
    if mode == "full":
        return 0, frames + taps - 1
    if mode == "same":
        return (taps - 1) // 2, frames
    assert mode == "head" and 0 <= first <= taps - 1
    return first, frames


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded: the product of two float32 is exact in float64; the float64 sum
    is rounded to odd from its exact error (two-sum), and a value rounded to odd at 53 bits rounds to 24 as the exact one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
    fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
    with np.errstate(invalid="ignore"):
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def direct32(x, h, first, count):
    """the direct path's float32 values: acc = +0.0f, acc = fmaf(h[k], x[n - k], acc) for k ascending over the terms inside the row"""
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    frames, taps = len(x), len(h)
    n = first + np.arange(count, dtype=np.int64)
    acc = np.zeros(count, np.float32)
    xp = np.concatenate([np.zeros(taps, np.float32), x, np.zeros(taps, np.float32)])
    for k in range(taps):
        inside = (n - k >= 0) & (n - k < frames)
        if not inside.any():
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            nxt = fma32(np.full(count, h[k], np.float32), xp[n - k + taps], acc)
        acc = np.where(inside, nxt, acc)
    return acc


def s_blocks(x, h):
    """S[b] = sum over p of A_h(p) A_x(b - p) for every block b of the line; A_x(j) is the sum of |x| over block pair j,
    x[(j - 1) B .. (j + 1) B) inside the row; a NaN stays a NaN"""
    x, h = np.abs(np.asarray(x, np.float32).astype(np.float64)), np.abs(np.asarray(h, np.float32).astype(np.float64))
    P, n_blocks = partitions(len(h)), -(-(len(x) + len(h) - 1) // B)
    a_h = np.array([h[p * B:(p + 1) * B].sum() for p in range(P)])
    a_x = np.array([x[max(0, (j - 1) * B):(j + 1) * B].sum() for j in range(n_blocks + 1)])
    S = np.zeros(n_blocks)
    for b in range(n_blocks):
        for p in range(min(P, b + 1)):
            S[b] += a_h[p] * a_x[b - p]
    return S


def interval(x, h, first, count):
    """(lo, hi, mid) of the `count` delivered samples from `first`, float64"""
    mid = line64(x, h)[first:first + count]
    assert len(mid) == count
    n = first + np.arange(count)
    E = bound_c(len(h)) * U * s_blocks(x, h)[n // B]
    return mid - E, mid + E, mid
