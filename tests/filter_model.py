"""The filter stage of include/afg.h stated again in numpy: the coefficient helper's formulas, the sequential recurrence of a
cascade -- in numpy.longdouble where that is wider than float64, float64 otherwise --, the bound E / max|x| and the interval
the device's result is held to.  Nothing here looks at the library."""
import math

import numpy as np

WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64
TILE, CHUNK, K, MAX_SECTIONS = 4096, 16, 64, 8
KINDS = ("lowpass", "highpass", "bandpass", "notch", "allpass", "peaking", "lowshelf", "highshelf", "preemphasis", "dc_block")
ROW_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("frames", np.uint32), ("reserved", np.uint32)])


def design(kind, samplerate=1.0, f0=0.0, q=math.sqrt(0.5), gain_db=0.0):
    """(b0, b1, b2, a1, a2) with a0 == 1: the Audio EQ Cookbook's sections, pre-emphasis (its coefficient in f0) and the DC
    blocker"""
    if kind == "preemphasis":
        return (1.0, -f0, 0.0, 0.0, 0.0)
    w = 2.0 * math.pi * f0 / samplerate
    if kind == "dc_block":
        return (1.0, -1.0, 0.0, -math.exp(-w), 0.0)
    c, alpha = math.cos(w), math.sin(w) / (2.0 * q)
    A = 10.0 ** (gain_db / 40.0)
    a = (1.0 + alpha, -2.0 * c, 1.0 - alpha)
    if kind == "lowpass":
        b = ((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0)
    elif kind == "highpass":
        b = ((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0)
    elif kind == "bandpass":
        b = (alpha, 0.0, -alpha)
    elif kind == "notch":
        b = (1.0, -2.0 * c, 1.0)
    elif kind == "allpass":
        b = (1.0 - alpha, -2.0 * c, 1.0 + alpha)
    elif kind == "peaking":
        b = (1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A)
        a = (1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A)
    elif kind in ("lowshelf", "highshelf"):
        S = 2.0 * math.sqrt(A) * alpha
        if kind == "lowshelf":
            b = (A * ((A + 1.0) - (A - 1.0) * c + S), 2.0 * A * ((A - 1.0) - (A + 1.0) * c), A * ((A + 1.0) - (A - 1.0) * c - S))
            a = ((A + 1.0) + (A - 1.0) * c + S, -2.0 * ((A - 1.0) + (A + 1.0) * c), (A + 1.0) + (A - 1.0) * c - S)
        else:
            b = (A * ((A + 1.0) + (A - 1.0) * c + S), -2.0 * A * ((A - 1.0) + (A + 1.0) * c), A * ((A + 1.0) + (A - 1.0) * c - S))
            a = ((A + 1.0) - (A - 1.0) * c + S, 2.0 * ((A - 1.0) - (A + 1.0) * c), (A + 1.0) - (A - 1.0) * c - S)
    else:
        raise ValueError(kind)
    return (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])


def response(sec, z):
    """H(z) of one section at the complex points z"""
    b0, b1, b2, a1, a2 = sec
    zi = 1.0 / np.asarray(z, dtype=np.complex128)
    return (b0 + b1 * zi + b2 * zi * zi) / (1.0 + a1 * zi + a2 * zi * zi)


def stable(sec):
    return all(math.isfinite(v) for v in sec) and abs(sec[4]) < 1.0 and abs(sec[3]) < 1.0 + sec[4]


def norms(sec):
    """(|g|_1, |h|_1): the impulse responses of 1 / A and of the section, summed in blocks until a block no longer counts"""
    b0, b1, b2, a1, a2 = sec
    if a1 == 0.0 and a2 == 0.0:
        return 1.0, abs(b0) + abs(b1) + abs(b2)
    g1 = g2 = 0.0
    sg = sh = 0.0
    n = 0
    while n < 1 << 28:
        bg = bh = 0.0
        for _ in range(1024):
            g = (1.0 if n == 0 else 0.0) - a1 * g1 - a2 * g2
            bg += abs(g)
            bh += abs(b0 * g + b1 * g1 + b2 * g2)
            g2, g1 = g1, g
            n += 1
        sg += bg
        sh += bh
        # a block that adds less than 2^-70 of the sum: the blocks behind it shrink geometrically from there
        if bg <= sg * 2.0 ** -70 and bh <= sh * 2.0 ** -70:
            return sg, sh
    raise ValueError("the impulse response does not decay")


def bound(sos):
    """E / max|x| of include/afg.h"""
    G, H = zip(*(norms(s) for s in sos))
    total, P = 0.0, 1.0
    for s, sec in enumerate(sos):
        beta, alpha = abs(sec[0]) + abs(sec[1]) + abs(sec[2]), abs(sec[3]) + abs(sec[4])
        after = 1.0
        for t in range(s + 1, len(sos)):
            after *= H[t]
        total += G[s] * (beta * P + alpha * P * H[s]) * after
        P *= H[s]
    return total * 2.0 ** -53


def run(sos, x):
    """the cascade over the rows of x ([rows, frames], zero history): the signals sig[0] = x, sig[s + 1] = section s's
    output, each [rows, frames] in the wide type, sample after sample"""
    x = np.atleast_2d(np.asarray(x))
    sig = [x.astype(WIDE)]
    for sec in sos:
        b0, b1, b2, a1, a2 = (WIDE(v) for v in sec)
        u = sig[-1]
        fir = b0 * u
        fir[:, 1:] += b1 * u[:, :-1]
        fir[:, 2:] += b2 * u[:, :-2]
        v = np.zeros_like(u)
        if a1 == 0 and a2 == 0:
            v = fir
        else:
            cols = np.ascontiguousarray(fir.T)               # [frames, rows]
            vt = np.zeros_like(cols)
            v1 = np.zeros(x.shape[0], WIDE)
            v2 = np.zeros(x.shape[0], WIDE)
            for n in range(cols.shape[0]):
                vn = cols[n] - a1 * v1 - a2 * v2
                vt[n] = vn
                v2, v1 = v1, vn
            v = np.ascontiguousarray(vt.T)
        sig.append(v)
    return sig


def state_at(sig, row, frames):
    """[n_sections, 4]: u[n-1], u[n-2], v[n-1], v[n-2] of every section behind frame `frames` - 1 of a row (zero history)"""
    def at(a, n):
        return a[row, n] if n >= 0 else WIDE(0)
    return np.array([[at(sig[s], frames - 1), at(sig[s], frames - 2), at(sig[s + 1], frames - 1), at(sig[s + 1], frames - 2)]
                     for s in range(len(sig) - 1)], dtype=WIDE)


def ulp32(a):
    """the spacing of float32 at magnitude a, never below 2^-149"""
    a = np.asarray(a, dtype=np.float64)
    _, e = np.frexp(a)
    return np.ldexp(1.0, np.where(a > 0.0, np.maximum(e - 24, -149), -149))


def allowance(want, KE):
    """the interval's half width round the exact result `want`: ulp32(|want| + K E) / 2 + K E"""
    mag = np.abs(np.asarray(want, dtype=np.float64)) + KE
    return 0.5 * ulp32(mag) + KE


def share(got, want, KE):
    """how much of K E an output uses: what its distance from `want` exceeds half an ulp32 by, over K E"""
    want = np.asarray(want)
    err = np.abs(np.asarray(got).astype(WIDE) - want).astype(np.float64)
    mag = np.abs(want.astype(np.float64)) + KE
    return np.maximum(err - 0.5 * ulp32(mag), 0.0) / KE
