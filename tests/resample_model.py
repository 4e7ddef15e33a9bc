"""numpy model of the sample-rate conversion and mono mix of include/afg.h (afg_resample_taps, afg_resample_hip,
afg_batch_decode_resampled): the float64 definition, the float32 restatement of the kernel's sum -- every product and
every add rounded to float32 on its own, the taps in order -- the mix, and the tensor the batch entry fills."""
import math

import numpy as np

ROLLOFF = 0.99


def shape(in_rate, out_rate, Z=6):
    """(M, L, W, fc) of a rate pair; equal rates have no filter: W = 0"""
    g = math.gcd(in_rate, out_rate)
    M, L = in_rate // g, out_rate // g
    fc = ROLLOFF * min(1.0, L / M)
    return M, L, (0 if in_rate == out_rate else math.ceil(Z / fc)), fc


def taps64(in_rate, out_rate, Z=6):
    """the table h[p][k] in float64, [L, 2 W]"""
    M, L, W, fc = shape(in_rate, out_rate, Z)
    k = np.arange(2 * W, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    d = (k - (W - 1)) - p / L
    x = np.clip(d * fc, -float(Z), float(Z))
    with np.errstate(all="ignore"):
        s = np.where(x == 0.0, 1.0, np.sin(np.pi * x) / (np.pi * x))
    c = np.cos(np.pi * x / (2.0 * Z))
    return fc * s * (c * c)


def taps32(in_rate, out_rate, Z=6):
    """... rounded once to float32: what the kernel multiplies with"""
    return taps64(in_rate, out_rate, Z).astype(np.float32)


def _gather(x, M, L, W, n_out, in_frame0):
    """per output frame t: its phase and its 2 W input samples (0 where the index is outside the row, with `valid` false)"""
    t = np.arange(n_out, dtype=np.int64)
    q, p = in_frame0 + (t * M) // L, (t * M) % L
    idx = q[:, None] - (W - 1) + np.arange(2 * W, dtype=np.int64)[None, :]
    valid = (idx >= 0) & (idx < len(x))
    xs = np.where(valid, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0, 0).astype(x.dtype)
    return p, xs, valid


def resample64(x, h, M, L, W, n_out, in_frame0=0):
    """the definition in float64: x a row, h the table (float64, or the float32 table widened)"""
    x = np.asarray(x, np.float64)
    if W == 0:
        q = in_frame0 + np.arange(n_out, dtype=np.int64)
        ok = (q >= 0) & (q < len(x))
        return np.where(ok, x[np.clip(q, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    p, xs, _ = _gather(x, M, L, W, n_out, in_frame0)
    return (np.asarray(h, np.float64)[p] * xs).sum(1)


def abs_sum64(x, h, M, L, W, n_out, in_frame0=0):
    """sum |h_k x_k| per output frame: the scale of the float32 sum's forward error bound"""
    p, xs, _ = _gather(np.asarray(x, np.float64), M, L, W, n_out, in_frame0)
    return np.abs(np.asarray(h, np.float64)[p] * xs).sum(1)


def resample32(x, h, M, L, W, n_out, in_frame0=0):
    """the kernel's sum: float32 row, float32 table; acc = +0, then acc = acc + h[p][k] * x[...] for k = 0 .. 2 W - 1, the
    product rounded to float32 and then the add; indexes outside the row contribute nothing.  W == 0: the words at q."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(n_out, np.float32)
    if W == 0:
        q = in_frame0 + np.arange(n_out, dtype=np.int64)
        ok = (q >= 0) & (q < len(x))
        out.view(np.uint32)[ok] = x.view(np.uint32)[q[ok]]
        return out
    # only the outputs whose window reaches the row can be anything but +0
    t_end = min(n_out, max(0, -(-(len(x) + W - in_frame0) * L // M) + 1)) if len(x) else 0
    if t_end == 0:
        return out
    h = np.ascontiguousarray(h, np.float32)
    p, xs, valid = _gather(x, M, L, W, t_end, in_frame0)
    acc = np.zeros(t_end, np.float32)
    with np.errstate(all="ignore"):
        for k in range(2 * W):
            prod = h[p, k] * xs[:, k]                       # float32 * float32 -> float32: one rounding
            acc = np.where(valid[:, k], acc + prod, acc)    # ... and one more
    out[:t_end] = acc
    return out


def mix(rows):
    """[R, n] float32 -> the mono row: s = x[0], s = s + x[r] in row order, s / (float)R; one row is itself, word for word"""
    rows = np.ascontiguousarray(rows, np.float32)
    if rows.shape[0] == 1:
        return rows[0].copy()
    with np.errstate(all="ignore"):
        s = rows[0].copy()
        for r in range(1, rows.shape[0]):
            s = s + rows[r]
        return s / np.float32(rows.shape[0])


def refusal(item, mono, in_channels, max_in_rate):
    """why afg_batch_decode_resampled refuses a decoded file, or None"""
    rate = int(round(item["samplerate"]))
    if rate <= 0 or rate > max_in_rate:
        return "rate"
    if mono and item["channels"] > in_channels:
        return "channels"
    return None


def tensor(floats, C, T, samplerate, first_frame=None, mono=False, in_channels=0, max_in_rate=0, Z=0, taps_of=None):
    """afgpu.batch_decode's items as the [files, C, T] tensor afg_batch_decode_resampled fills.  taps_of(in_rate): the float32
    table [L, 2 W] to use (default: this module's)."""
    in_channels, max_in_rate, Z = in_channels or 2, max_in_rate or 48000, Z or 6
    ff = [0] * len(floats) if first_frame is None else first_frame
    out = np.zeros((len(floats), C, T), np.float32)
    for i, it in enumerate(floats):
        if it["status"] != 0 or it["pcm"] is None or refusal(it, mono, in_channels, max_in_rate):
            continue
        rate = int(round(it["samplerate"]))
        M, L, W, _ = shape(rate, samplerate, Z)
        h = None if W == 0 else (taps32(rate, samplerate, Z) if taps_of is None else taps_of(rate))
        rows = np.ascontiguousarray(np.asarray(it["pcm"], np.float32).reshape(-1, it["channels"]).T)
        if mono:
            out[i, 0] = resample32(mix(rows), h, M, L, W, T, int(ff[i]))
        else:
            for k in range(min(C, it["channels"])):
                out[i, k] = resample32(rows[k], h, M, L, W, T, int(ff[i]))
    return out


def same_bits(got, want):
    """indexes where two float32 arrays differ: bit for bit, except that where `want` is NaN only NaN-ness is compared
    (how a payload travels through arithmetic is not part of the contract)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return np.argwhere(np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32)))
