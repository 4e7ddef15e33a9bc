"""The mixing stage of include/afg.h restated in numpy: the noise under a row (a clip read from a start, wrapping round its
end), both energies of a group in the normalisation's fixed order (normalize_model.tile_sums: 16 sequential steps per lane,
a tree of 8 halvings over the 256 lanes, the tiles one after the other), the gain, and the float32 apply whose product is
rounded before its sum.  The device is compared with this bit for bit.

As in normalize_model, what numpy on a CPU would leave to the hardware is written out: a NaN in an energy or the output is
always the positive quiet NaN."""
import numpy as np

import normalize_model as nm

TILE = nm.TILE
SNR, GAIN = 0, 1                                                 # afg_mix_group.flags
SILENT_SIGNAL, SILENT_NOISE, ENERGY_NOT_FINITE, GAIN_NOT_FINITE = 1, 2, 4, 8      # afg_mix_stats.flags
GROUP_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("stride", np.uint64), ("first_tile", np.uint64),
                        ("noise_off", np.uint64), ("noise_stride", np.uint64), ("ratio", np.float64), ("rows", np.uint32),
                        ("valid", np.uint32), ("noise_len", np.uint32), ("noise_start", np.uint32), ("flags", np.uint32),
                        ("gain", np.float32)])
STATS_DTYPE = np.dtype([("signal_energy", np.float64), ("noise_energy", np.float64), ("gain", np.float32), ("flags", np.uint32)])
assert GROUP_DTYPE.itemsize == 80 and STATS_DTYPE.itemsize == 24
F32, F64 = np.float32, np.float64


def ratio(snr_db):
    """10^(-snr_db / 10): what afg_mix_ratio computes (the library's own value goes into a record: pow is not correctly
    rounded everywhere, so the two may differ in the last place)"""
    return F64(10.0) ** (F64(-snr_db) / F64(10.0))


def noise_index(start, count, N):
    """the clip positions under elements 0 .. count - 1 of a row: (start + e) mod N"""
    return (np.uint64(start) + np.arange(count, dtype=np.uint64)) % np.uint64(N)


def noise_under(clip, start, count):
    """the noise samples as used under a row of `count` elements: the clip (its N samples) from `start`, looping"""
    clip = np.asarray(clip, F32)
    return clip[noise_index(start, count, clip.size).astype(np.int64)]


def energy(rows):
    """the sum of squares of a group given as [rows, valid] float32, in the definition's order"""
    return nm.group_sums(np.asarray(rows, F32))[1]


def gain64(es, en, ratio):
    """sqrt((Es / En) * ratio) in float64, each operation rounded: the gain before its rounding to float32"""
    with np.errstate(all="ignore"):
        q = F64(es) / F64(en)
        v = q * F64(ratio)
        return np.sqrt(v)


def group_stats(x, z, mode, ratio=0.0, gain=0.0):
    """the afg_mix_stats record of a group: x its rows [rows, valid], z the noise as used under them, same shape"""
    st = np.zeros((), STATS_DTYPE)
    x, z = np.asarray(x, F32), np.asarray(z, F32)
    if x.size == 0:
        return st
    es, en = energy(x), energy(z)
    st["signal_energy"], st["noise_energy"] = nm._one_nan(es), nm._one_nan(en)
    if mode == GAIN:
        st["gain"] = F32(gain)
        return st
    why = 0
    if es == 0:
        why |= SILENT_SIGNAL
    if en == 0:
        why |= SILENT_NOISE
    if not np.isfinite(es) or not np.isfinite(en):
        why |= ENERGY_NOT_FINITE
    g = F32(0.0)
    if why == 0:
        with np.errstate(all="ignore"):
            g = F32(gain64(es, en, ratio))
        if not np.isfinite(g):
            why, g = GAIN_NOT_FINITE, F32(0.0)
    st["gain"], st["flags"] = g, why
    return st


def apply(x, z, g):
    """y = x + g * z in float32, the product rounded first; the input's bits when g is 0"""
    x, z, g = np.asarray(x, F32), np.asarray(z, F32), F32(g)
    if g == 0:
        return x.copy()
    with np.errstate(all="ignore"):
        p = (g * z).astype(F32)
        return nm._one_nan((x + p).astype(F32))


def mix(plane_in, plane_noise, plane_out, groups):
    """every group of `groups` (GROUP_DTYPE records): returns (a copy of plane_out with the groups' valid elements written,
    the STATS_DTYPE records)"""
    out = plane_out.copy()
    stats = np.zeros(len(groups), STATS_DTYPE)
    for k, g in enumerate(groups):
        rows, valid, stride = int(g["rows"]), int(g["valid"]), int(g["stride"])
        if valid == 0:
            continue
        N, start, nstride = int(g["noise_len"]), int(g["noise_start"]), int(g["noise_stride"])
        x = np.stack([plane_in[int(g["in_off"]) + r * stride:][:valid] for r in range(rows)])
        z = np.stack([noise_under(plane_noise[int(g["noise_off"]) + r * nstride:][:N], start, valid) for r in range(rows)])
        stats[k] = group_stats(x, z, int(g["flags"]), g["ratio"], g["gain"])
        y = apply(x, z, stats[k]["gain"])
        for r in range(rows):
            o = int(g["out_off"]) + r * stride
            out[o:o + valid] = y[r]
    return out, stats


def layout(groups):
    """afg_mix_layout: fills first_tile, returns the tile count"""
    tiles = 0
    for g in groups:
        g["first_tile"] = tiles
        tiles += -(-int(g["valid"]) // TILE) * int(g["rows"])
    return tiles


def same_stats(got, want):
    """field names in which two STATS_DTYPE arrays differ as bit patterns, with the first index"""
    bad = []
    for name in STATS_DTYPE.names:
        w = nm.same_bits(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]))
        if w.size:
            bad.append((name, int(w[0])))
    return bad
