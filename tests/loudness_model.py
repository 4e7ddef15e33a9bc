"""The loudness stage of include/afg.h stated again in numpy: the K-weighting's design, the blocks with libebur128's rounding,
their energies z_j -- the K-weighted rows from filter_model.run, in numpy.longdouble where that is wider than float64 --, the
two gates, the gain, and the interval B_j the device's block energies are held to.  Nothing here looks at the library."""
import functools
import math

import numpy as np

import filter_model as fm

WIDE = fm.WIDE
K_L = 64
UNGATED, GAIN_CLAMPED, PEAK_CLAMPED = 1, 2, 4
GAMMA_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
BS1770_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
              (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))             # the standard's table, a0 == 1
GROUP_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("stride", np.uint64), ("first_sub", np.uint64), ("first_block", np.uint64),
                        ("rows", np.uint32), ("valid", np.uint32), ("reserved", np.uint32, 4)])
STATS_DTYPE = np.dtype([("energy", np.float64), ("rel_threshold", np.float64), ("n_blocks", np.uint32), ("n_abs", np.uint32), ("n_gated", np.uint32),
                        ("flags", np.uint32), ("peak", np.float32), ("gain", np.float32)])


def kweight(samplerate):
    """the two sections (b0, b1, b2, a1, a2): the shelf, then the high-pass with the table's numerator (1, -2, 1)"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / samplerate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / samplerate)
    a0 = 1.0 + K / Q + K * K
    return [shelf, (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)]


def step_of(samplerate):
    return (samplerate + 5) // 10


def blocks_of(valid, step):
    return (valid - 4 * step) // step + 1 if valid >= 4 * step else 0


def lufs(energy):
    return -0.691 + 10.0 * math.log10(energy) if energy > 0 else -math.inf


@functools.lru_cache(maxsize=None)
def filter_bound(samplerate):
    """E / max|x| of the K-weighting (filter_model.bound)"""
    return fm.bound(kweight(samplerate))


def subblock_sums(x, samplerate):
    """x: [rows, frames] float32 (rows of different lengths padded with zeros behind them).  Returns the exact sums of squares
    of the K-weighted rows over consecutive sub-blocks of `step` frames, [rows, frames // step], in the wide type"""
    x = np.atleast_2d(x)
    step = step_of(samplerate)
    v = kweighted(x, samplerate, WIDE)
    n = x.shape[1] // step
    return (v[:, :n * step] ** 2).reshape(x.shape[0], n, step).sum(axis=2)


def kweighted(x, samplerate, dtype=np.float64, chunk=128):
    """the K-weighted rows of x [rows, frames] in `dtype`, for signals of minutes: every section runs over all chunks of
    `chunk` frames at once from a zero state, and the chunks' states are then carried through in order.  A chunk's zero-state run
    and its correction partly cancel, which costs a few of `dtype`'s last bits per doubling of the chunk: test_loudness_model.py
    holds the wide result to filter_model.run's sample-after-sample recurrence within a sixteenth of the filter bound's unit"""
    y = np.atleast_2d(np.asarray(x)).astype(dtype)
    rows, n = y.shape
    m = -(-n // chunk)
    for sec in kweight(samplerate):
        b0, b1, b2, a1, a2 = (dtype(c) for c in sec)
        u = np.zeros((rows, m * chunk), dtype)
        u[:, :n] = y
        fir = b0 * u
        fir[:, 1:] += b1 * u[:, :-1]
        fir[:, 2:] += b2 * u[:, :-2]
        v = fir.reshape(rows, m, chunk)
        h = np.zeros((2, chunk), dtype)                          # what v[-1] = 1 and what v[-2] = 1 leave in a chunk without input
        p = [(dtype(1), dtype(0)), (dtype(0), dtype(1))]         # (v[k-1], v[k-2]) of the two
        for k in range(chunk):
            if k >= 1:
                v[:, :, k] -= a1 * v[:, :, k - 1]
            if k >= 2:
                v[:, :, k] -= a2 * v[:, :, k - 2]
            for q in range(2):
                h[q, k] = -a1 * p[q][0] - a2 * p[q][1]
                p[q] = (h[q, k], p[q][0])
        for c in range(1, m):
            v[:, c, :] += v[:, c - 1, -1:] * h[0] + v[:, c - 1, -2:-1] * h[1]
        y = v.reshape(rows, m * chunk)[:, :n]
    return y


def weights_of(weights, rows):
    w = [0.0] * 8
    if weights is not None:
        w[:len(weights)] = [float(v) for v in weights]
    if not any(w):
        w = [1.0] * 8
    return np.array(w[:rows], dtype=WIDE)


def block_energies(S, valid, samplerate, weights=None):
    """S: a group's sub-block sums [rows, >= n_blocks + 3] (subblock_sums).  Returns (z, Sb): z_j in the wide type and the rows'
    block sums S_ij [rows, n_blocks]"""
    step = step_of(samplerate)
    nb = blocks_of(valid, step)
    rows = S.shape[0]
    if nb == 0:
        return np.zeros(0, WIDE), np.zeros((rows, 0), WIDE)
    Sb = S[:, 0:nb] + S[:, 1:nb + 1] + S[:, 2:nb + 2] + S[:, 3:nb + 3]
    G = weights_of(weights, rows)
    return (G[:, None] * Sb).sum(axis=0) / WIDE(4 * step), Sb


def block_bounds(z, Sb, peak, samplerate, weights=None):
    """B_j of include/afg.h round the delivered energies `z` (float64): (1 / N) sum_i G_i (2 e sqrt(N S_ij) + N e^2) + c 2^-53 z"""
    rows, N = Sb.shape[0], 4 * step_of(samplerate)
    e = K_L * filter_bound(samplerate) * float(peak)
    G = weights_of(weights, rows).astype(np.float64)
    first = (G[:, None] * (2.0 * e * np.sqrt(N * Sb.astype(np.float64)) + N * e * e)).sum(axis=0) / N
    return first + (N + rows + 8) * 2.0 ** -53 * np.asarray(z, dtype=np.float64)


def gate(z):
    """(n_abs, rel_threshold, gated mask, energy) of the block energies z"""
    z = np.asarray(z)
    above = z > GAMMA_ABS
    n_abs = int(above.sum())
    rel = 0.1 * (z[above].sum() / n_abs) if n_abs else z.dtype.type(0)
    gated = above & (z > rel)
    n = int(gated.sum())
    return n_abs, rel, gated, (z[gated].sum() / n if n else z.dtype.type(0))


def gate_margin(z):
    """the least |z_j / Gamma - 1| over both gates (inf without blocks): how far the decisions are from flipping"""
    z = np.asarray(z).astype(np.float64)
    if z.size == 0:
        return math.inf
    _, rel, _, _ = gate(z)
    m = np.abs(z / GAMMA_ABS - 1.0).min()
    return float(min(m, np.abs(z / rel - 1.0).min())) if rel > 0 else float(m)


def gain_of(energy, peak, target_lufs=-23.0, max_peak=0.0, max_gain=0.0):
    """(gain, flags) as float32 and int: the definition's operations on a float64 energy and a float32 peak"""
    if not energy > 0:
        return np.float32(1.0), UNGATED
    T = 10.0 ** ((target_lufs + 0.691) / 10.0)
    g, flags = np.float32(math.sqrt(T / float(energy))), 0
    if max_gain > 0 and g > np.float32(max_gain):
        g, flags = np.float32(max_gain), flags | GAIN_CLAMPED
    if max_peak > 0 and peak > 0:
        top = np.float32(max_peak) / np.float32(peak)
        if g > top:
            g, flags = top, flags | PEAK_CLAMPED
    return np.float32(g), flags


def measure(x, valid, samplerate, weights=None):
    """one group, x [rows, >= valid] float32: dict of z, Sb, peak, n_blocks, n_abs, rel, gated, energy (wide types)"""
    x = np.atleast_2d(x)[:, :valid]
    z, Sb = block_energies(subblock_sums(x, samplerate), valid, samplerate, weights)
    n_abs, rel, gated, energy = gate(z)
    return dict(z=z, Sb=Sb, peak=np.float32(np.abs(x).max()) if x.size else np.float32(0), n_blocks=len(z), n_abs=n_abs, rel=rel, gated=gated,
                energy=energy)
