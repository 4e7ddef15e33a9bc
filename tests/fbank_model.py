"""numpy model of the Kaldi-compatible filter-bank stage (include/afg.h: afg_fbank_hip): the float64 definition, the host
tables in float64, and the intervals the header states for every delivered element.

  frames     snip_edges: 0 when N < ws, else 1 + (N - ws) / hop; otherwise (N + hop / 2) / hop.
  sample j   of frame f is index f * hop + j - pad, pad = 0 or ws / 2 - hop / 2, mirrored with the edge repeated until inside.
  per frame  s = float32(x * scale); then in float64 mu = mean(s), d = s - mu, e_j = d_j - c d_(j-1) (d_(-1) = d_0), z = e w,
             zero padded to n_fft, X = DFT(z), p = |X|^2 or |X|, mel = W p, log over 2^-23; the energy sum d^2 or sum z^2.
  bound      u = 2^-24, A_f = sum_j w_j (|d_j| + c |d_(j-1)|), B = 8 ceil(log2 n_fft) + 12, E_f = B u A_f on re and im;
             p_hi = (|re| + E)^2 + (|im| + E)^2, p_lo = max(|re| - E, 0)^2 + max(|im| - E, 0)^2;
             mel in [(1 - (n_bins + 4) u) W q_lo, (1 + (n_bins + 4) u) W q_hi] with q = p, or for magnitudes the square roots of
             [(1 - 4u) p_lo, (1 + 4u) p_hi] widened by 2 float32 ulp; logs within 3 float32 ulp after the floor;
             raw energy within (ws + 12) u relative; windowed in (1 -+ (ws + 4) u) sum (|z_j| -+ eps_j)^2,
             eps_j = 4 u w_j (|d_j| + c |d_(j-1)|), clamped at 0 per term."""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -23
FRAMES_MAJOR, MEL_MAJOR = 0, 1
POVEY, HAMMING, HANNING, BLACKMAN, RECTANGULAR = range(5)


def params(win_length=400, hop=160, n_fft=None, n_mels=23, snip_edges=1, remove_dc=1, preemph=0.97, use_power=1, use_log=1, use_energy=0,
           raw_energy=1, htk_compat=0, energy_floor=0.0, scale=0.0, layout=FRAMES_MAJOR):
    """the fields of afg_fbank_params (preemph, energy_floor and scale as the float32 the structure holds)"""
    f32 = lambda v: float(np.float32(v))
    return SimpleNamespace(win_length=win_length, hop=hop, n_fft=n_fft_of(win_length) if n_fft is None else n_fft, n_mels=n_mels,
                           snip_edges=int(snip_edges), remove_dc=int(remove_dc), use_power=int(use_power), use_log=int(use_log),
                           use_energy=int(use_energy), raw_energy=int(raw_energy), htk_compat=int(htk_compat), layout=layout,
                           preemph=f32(preemph), energy_floor=f32(energy_floor), scale=f32(scale))


def n_fft_of(ws, round_pow2=True):
    return 1 << (ws - 1).bit_length() if round_pow2 else ws


def n_frames(N, ws, hop, snip_edges):
    if snip_edges:
        return 0 if N < ws else 1 + (N - ws) // hop
    return (N + hop // 2) // hop


def pad_of(ws, hop, snip_edges):
    return 0 if snip_edges else ws // 2 - hop // 2


def mirror(i, N):
    """Kaldi's loop over an index array: reflected with the edge repeated until inside [0, N)"""
    i = np.array(i, dtype=np.int64)
    while True:
        lo, hi = i < 0, i >= N
        if not (lo.any() or hi.any()):
            return i
        i = np.where(lo, -1 - i, np.where(hi, 2 * N - 1 - i, i))


def frame_index(N, ws, hop, snip_edges, F):
    """[F, ws] sample indexes"""
    i = np.arange(F, dtype=np.int64)[:, None] * hop + np.arange(ws, dtype=np.int64)[None, :] - pad_of(ws, hop, snip_edges)
    return mirror(i, N) if F else i


def window64(window_type, ws, blackman_coeff=0.42):
    a = 2.0 * np.pi * np.arange(ws, dtype=np.float64) / (ws - 1)
    if window_type == POVEY:
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if window_type == HAMMING:
        return 0.54 - 0.46 * np.cos(a)
    if window_type == HANNING:
        return 0.5 - 0.5 * np.cos(a)
    if window_type == BLACKMAN:
        return blackman_coeff - 0.5 * np.cos(a) + (0.5 - blackman_coeff) * np.cos(2.0 * a)
    assert window_type == RECTANGULAR
    return np.ones(ws)


def tables32(window_type, ws, n_fft, blackman_coeff=0.42):
    """afg_fbank_tables' layout: ws window floats, then n_fft pairs (cos, -sin), each rounded once"""
    a = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    return np.concatenate([window64(window_type, ws, blackman_coeff), np.stack([np.cos(a), -np.sin(a)], axis=1).reshape(-1)]).astype(np.float32)


def mel_of(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def filters64(samplerate, n_fft, n_mels, low_freq=20.0, high_freq=0.0):
    """[n_mels, n_fft // 2 + 1] float64, the Nyquist column zero"""
    nyquist = samplerate / 2.0
    if high_freq <= 0.0:
        high_freq += nyquist
    assert 0.0 <= low_freq < high_freq <= nyquist
    m_lo = float(mel_of(low_freq))
    delta = (float(mel_of(high_freq)) - m_lo) / (n_mels + 1)
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    left, centre, right = m_lo + m * delta, m_lo + (m + 1.0) * delta, m_lo + (m + 2.0) * delta
    mk = mel_of(np.arange(n_fft // 2 + 1, dtype=np.float64) * samplerate / n_fft)[None, :]
    W = np.maximum(0.0, np.minimum((mk - left) / (centre - left), (right - mk) / (right - centre)))
    if n_fft % 2 == 0:
        W[:, n_fft // 2] = 0.0
    return W


def cols_of(prm):
    return prm.n_mels + prm.use_energy


def pieces64(x, prm, window, F):
    """(d [F, ws], dprev, z [F, n_fft], w) in float64 from a float32 row; a NaN sample makes NaN of its frames"""
    x = np.ascontiguousarray(x, np.float32)
    ws = prm.win_length
    w = np.asarray(window, np.float64)[:ws]
    idx = frame_index(len(x), ws, prm.hop, prm.snip_edges, F)
    with np.errstate(all="ignore"):
        s = (x[idx] * np.float32(prm.scale if prm.scale else 1.0)).astype(np.float32).astype(np.float64)
        d = s - s.mean(axis=1, keepdims=True) if prm.remove_dc else s
        dprev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
        z = np.zeros((F, prm.n_fft))
        z[:, :ws] = (d - prm.preemph * dprev) * w
    return d, dprev, z, w


def _arrange(prm, mel, energy):
    if not prm.use_energy:
        return mel
    return np.concatenate([mel, energy[:, None]] if prm.htk_compat else [energy[:, None], mel], axis=1)


def values64(x, prm, window, bank, F):
    """the definition: [F, cols] float64 (frames-major whatever prm.layout says)"""
    d, dprev, z, w = pieces64(x, prm, window, F)
    with np.errstate(all="ignore"):
        X = np.fft.rfft(z, axis=1)
        p = np.abs(X) ** 2 if prm.use_power else np.abs(X)
        mel = p @ np.asarray(bank, np.float64).T
        if prm.use_log:
            mel = np.log(np.maximum(mel, EPS))
        en = np.log(np.maximum((d * d).sum(axis=1) if prm.raw_energy else (z * z).sum(axis=1), EPS))
        if prm.energy_floor > 0.0:
            en = np.maximum(en, math.log(prm.energy_floor))
    return _arrange(prm, mel, en)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64).astype(np.float32))).astype(np.float64)


def bound_b(n_fft):
    return 8 * math.ceil(math.log2(n_fft)) + 12


def _log_bounds(lo, hi):
    with np.errstate(all="ignore"):
        a, b = np.log(np.maximum(lo, EPS)), np.log(np.maximum(hi, EPS))
    return a - 3.0 * ulp32(a), b + 3.0 * ulp32(b)


def intervals(x, prm, window32, bank32, F):
    """(lo, hi, mid), each [F, cols] float64: the interval of every delivered element and the float64 value itself.  window32
    and bank32 are the float32 tables the device is given.  A frame with a NaN sample under it is NaN in lo and hi."""
    d, dprev, z, w = pieces64(x, prm, np.asarray(window32, np.float32), F)
    W = np.asarray(bank32, np.float32).astype(np.float64)
    assert (W >= 0).all()
    ws, nb, c = prm.win_length, prm.n_fft // 2 + 1, prm.preemph
    with np.errstate(all="ignore"):
        X = np.fft.rfft(z, axis=1)
        re, im = X.real, X.imag
        reach = w[None, :] * (np.abs(d) + c * np.abs(dprev))
        E = (bound_b(prm.n_fft) * U * reach.sum(axis=1))[:, None]
        p_hi = (np.abs(re) + E) ** 2 + (np.abs(im) + E) ** 2
        p_lo = np.maximum(np.abs(re) - E, 0.0) ** 2 + np.maximum(np.abs(im) - E, 0.0) ** 2
        p_lo = np.where(np.isnan(re) | np.isnan(im), np.nan, p_lo)
        if prm.use_power:
            q_lo, q_hi, q = p_lo, p_hi, re * re + im * im
        else:
            a, b = np.sqrt((1.0 - 4.0 * U) * p_lo), np.sqrt((1.0 + 4.0 * U) * p_hi)
            q_lo, q_hi, q = np.maximum(a - 2.0 * ulp32(a), 0.0), b + 2.0 * ulp32(b), np.sqrt(re * re + im * im)
            q_lo = np.where(np.isnan(a), np.nan, q_lo)
        lo, hi, mid = (1.0 - (nb + 4) * U) * (q_lo @ W.T), (1.0 + (nb + 4) * U) * (q_hi @ W.T), q @ W.T
        if prm.use_log:
            lo, hi = _log_bounds(lo, hi)
            mid = np.log(np.maximum(mid, EPS))
        if not prm.use_energy:
            return lo, hi, mid
        if prm.raw_energy:
            en = (d * d).sum(axis=1)
            e_lo, e_hi = en * (1.0 - (ws + 12) * U), en * (1.0 + (ws + 12) * U)
        else:
            zz, eps = np.abs(z[:, :ws]), 4.0 * U * reach
            en = (zz * zz).sum(axis=1)
            e_lo = (1.0 - (ws + 4) * U) * (np.maximum(zz - eps, 0.0) ** 2).sum(axis=1)
            e_hi = (1.0 + (ws + 4) * U) * ((zz + eps) ** 2).sum(axis=1)
            e_lo = np.where(np.isnan(en), np.nan, e_lo)
        e_lo, e_hi = _log_bounds(e_lo, e_hi)
        e_mid = np.log(np.maximum(en, EPS))
        if prm.energy_floor > 0.0:
            fl = math.log(prm.energy_floor)
            e_lo, e_hi = np.maximum(e_lo, fl - 3.0 * ulp32(fl)), np.maximum(e_hi, fl + 3.0 * ulp32(fl))
            e_mid = np.maximum(e_mid, fl)
    return _arrange(prm, lo, e_lo), _arrange(prm, hi, e_hi), _arrange(prm, mid, e_mid)


def outside(got, lo, hi):
    """indexes of the float32 values that are not inside [lo, hi] (a NaN anywhere counts)"""
    g = np.asarray(got, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.argwhere(~((g >= lo) & (g <= hi)))


def used_share(got, lo, hi, mid):
    """the largest deviation from the float64 value as a share of the interval's half-width"""
    g = np.asarray(got, np.float32).astype(np.float64)
    half = (hi - lo) / 2.0
    ok = np.isfinite(half) & (half > 0)
    return float((np.abs(g - mid)[ok] / half[ok]).max()) if ok.any() else 0.0
