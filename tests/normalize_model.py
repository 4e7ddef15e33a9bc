"""The normalisation stage of include/afg.h restated in numpy: the statistics of a group of rows in the definition's fixed
order (16 sequential vector steps per lane, a tree of 8 halvings over the 256 lanes, the tiles one after the other), what
each mode makes of them, and the float32 apply.  The device is compared with this bit for bit.

Two things numpy on a CPU would leave to the hardware are written out, as the definition has them: min and max order -0
below +0, and a NaN in a sum, in offset, scale or the output is always the positive quiet NaN (an x86 CPU makes the negative
one of inf - inf, and which of two NaN operands an add returns differs between machines)."""
import numpy as np

TILE, LANES = 4096, 256
NONE, PEAK, RMS, STANDARD, DYNAMIC_RANGE = range(5)
MODES = (NONE, PEAK, RMS, STANDARD, DYNAMIC_RANGE)
STATS_DTYPE = np.dtype([("sum", np.float64), ("sumsq", np.float64), ("count", np.uint64), ("min", np.float32), ("max", np.float32),
                        ("offset", np.float32), ("scale", np.float32)])
GROUP_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("stride", np.uint64), ("first_tile", np.uint64),
                        ("rows", np.uint32), ("valid", np.uint32), ("reserved", np.uint32, (2,))])
assert STATS_DTYPE.itemsize == 40 and GROUP_DTYPE.itemsize == 48
WHISPER = dict(range=8.0, shift=4.0, gain=0.25)
F32, F64 = np.float32, np.float64


def _one_nan(result):
    """result with every NaN replaced by the positive quiet NaN"""
    result = np.asarray(result)
    return np.where(np.isnan(result), np.asarray(np.nan, result.dtype), result).astype(result.dtype)


def tile_sums(x):
    """(sum, sumsq) of one tile of up to 4096 float32, in the definition's order"""
    assert x.dtype == np.float32 and x.ndim == 1 and 0 < x.size <= TILE
    v = np.zeros(TILE, F64)                                      # (a lane that adds +0.0 keeps its bits: a sum is never -0.0)
    v[:x.size] = x
    v = v.reshape(4, LANES, 4)                                   # element e = 1024 k + 4 lane + j
    s, q = np.zeros(LANES, F64), np.zeros(LANES, F64)
    with np.errstate(all="ignore"):
        for k in range(4):
            for j in range(4):                                   # 16 sequential steps, all lanes at once
                d = v[k, :, j]
                s = _one_nan(s + d)
                q = _one_nan(q + d * d)
        while s.size > 1:                                        # 8 halvings: v[l] = v[l] + v[l + d] for l % (2 d) == 0
            s = _one_nan(s[0::2] + s[1::2])
            q = _one_nan(q[0::2] + q[1::2])
    return s[0], q[0]


def min_max(x):
    """of the samples that are no NaN, -0 below +0; (+inf, -inf) when there is none"""
    f = x[~np.isnan(x)]
    if f.size == 0:
        return F32(np.inf), F32(-np.inf)
    mn, mx = f.min(), f.max()
    zeros = f[f == 0]
    if mn == 0:
        mn = F32(-0.0) if np.signbit(zeros).any() else F32(0.0)
    if mx == 0:
        mx = F32(0.0) if (~np.signbit(zeros)).any() else F32(-0.0)
    return F32(mn), F32(mx)


def chain(parts):
    """the parts added one after the other, starting from +0.0 (np.add.accumulate is sequential; np.sum is pairwise)"""
    parts = np.asarray(list(parts), F64)
    with np.errstate(all="ignore"):
        total = np.add.accumulate(np.concatenate([np.zeros(1, F64), parts]))[-1]
    return F64(np.nan) if np.isnan(total) else F64(total)


def group_sums(rows, tile_order=None):
    """(sum, sumsq) of a group given as [rows, valid] float32.  tile_order: another order of the tiles (the tests show that
    the order matters)"""
    tiles = [r[t:t + TILE] for r in rows for t in range(0, r.size, TILE)]
    if tile_order is not None:
        tiles = [tiles[i] for i in tile_order]
    parts = [tile_sums(np.ascontiguousarray(t)) for t in tiles]
    return chain([p[0] for p in parts]), chain([p[1] for p in parts])


def params(mode, target=1.0, eps=0.0, range=8.0, shift=4.0, gain=0.25):
    return dict(mode=mode, target=F32(target), eps=F32(eps), range=F32(range), shift=F32(shift), gain=F32(gain))


def group_stats(rows, prm):
    """the afg_norm_stats record of a group given as [rows, valid] float32"""
    st = np.zeros((), STATS_DTYPE)
    rows = np.asarray(rows, F32)
    if rows.size == 0:
        return st
    s, q = group_sums(rows)
    mn, mx = min_max(rows.ravel())
    count = F64(rows.size)
    offset, scale = F32(0.0), F32(1.0)
    mode = prm["mode"]
    with np.errstate(all="ignore"):
        if mode == PEAK:
            p = max(-mn, mx)                                     # (never a NaN; a zero of either sign gives scale 1)
            if p != 0 and np.isfinite(p):
                scale = F32(prm["target"]) / F32(p)
        elif mode == RMS:
            r = F32(np.sqrt(q / count))
            if r != 0 and np.isfinite(r):
                scale = F32(prm["target"]) / r
        elif mode == STANDARD:
            mean = s / count
            var = q / count - mean * mean
            if not var > 0:                                      # fmax(var, 0), a NaN gives 0
                var = F64(0.0)
            eps = F32(prm["eps"]) if prm["eps"] != 0 else F32(1e-7)
            offset = F32(mean)
            scale = F32(F64(1.0) / np.sqrt(var + F64(eps)))
        elif mode == DYNAMIC_RANGE:
            offset = F32(mx) - F32(prm["range"])
            scale = F32(prm["gain"])
    st["sum"], st["sumsq"], st["count"], st["min"], st["max"] = _one_nan(s), _one_nan(q), rows.size, mn, mx
    st["offset"], st["scale"] = _one_nan(offset), _one_nan(scale)
    return st


def apply(x, st, prm):
    """the valid elements x (float32, any shape) of a group with record st, in float32 operations"""
    x = np.asarray(x, F32)
    offset, scale = F32(st["offset"]), F32(st["scale"])
    with np.errstate(all="ignore"):
        if prm["mode"] == DYNAMIC_RANGE:
            m = np.where(x > offset, x, offset).astype(F32)
            a = m + F32(prm["shift"])
            return _one_nan(a * scale)
        d = x - offset
        return _one_nan(d * scale)


def normalize(plane_in, plane_out, groups, prm):
    """every group of `groups` (GROUP_DTYPE records, or dicts with in_off, out_off, stride, rows, valid): returns (a copy
    of plane_out with the groups' valid elements written, the STATS_DTYPE records).  Mode NONE writes nothing."""
    out = None if plane_out is None else plane_out.copy()
    stats = np.zeros(len(groups), STATS_DTYPE)
    for k, g in enumerate(groups):
        rows, valid, stride = int(g["rows"]), int(g["valid"]), int(g["stride"])
        if valid == 0:
            continue
        at = [int(g["in_off"]) + r * stride for r in range(rows)]
        x = np.stack([plane_in[a:a + valid] for a in at])
        stats[k] = group_stats(x, prm)
        if prm["mode"] != NONE:
            y = apply(x, stats[k], prm)
            for r in range(rows):
                o = int(g["out_off"]) + r * stride
                out[o:o + valid] = y[r]
    return out, stats


def layout(groups):
    """afg_norm_layout: fills first_tile, returns the tile count"""
    tiles = 0
    for g in groups:
        g["first_tile"] = tiles
        tiles += -(-int(g["valid"]) // TILE) * int(g["rows"])
    return tiles


def valid_length(frames, first_frame, in_rate, out_rate, T):
    """a file's valid length in the tensor at one rate: min(T, ceil((frames - first_frame) * L / M)), 0 when not positive"""
    from math import gcd
    g = gcd(int(in_rate), int(out_rate))
    M, L = int(in_rate) // g, int(out_rate) // g
    d = int(frames) - int(first_frame)
    return 0 if d <= 0 else min(int(T), -(-d * L // M))


def same_bits(got, want):
    """flat indices where two arrays of one 4- or 8-byte type differ as bit patterns"""
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    a, b = np.ascontiguousarray(got).view(u).ravel(), np.ascontiguousarray(want).view(u).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero(a != b)


def same_stats(got, want):
    """field names in which two STATS_DTYPE arrays differ as bit patterns, with the first index"""
    bad = []
    for name in STATS_DTYPE.names:
        w = same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]))
        if w.size:
            bad.append((name, int(w[0])))
    return bad
