"""What afg_mp3_requant_hip computes, stated without the product (test infrastructure): `requant_numpy`, the float32
statement of the kernel (it takes its tables from the product: tests/test_mp3_requant.py holds it to the float front-end);
`tables_from_bands`, the same tables derived from scalefactor-band widths alone; `pow43_64`, the definition of the
requantiser's power in float64.  tests/test_mp3_requant_model.py holds the product's tables to the derived ones."""
import functools

import numpy as np

import afgpu
import mp3_bitstream as mb

# The 8 rate rows of every kind's table (minimp3.d:134-137: index = sample-rate field + 3 per MPEG version step, then one
# off for every row but the first, because the first two MPEG-2.5 rates share a table):
#   row 0  MPEG-2.5 11025 Hz and 12000 Hz        row 1  MPEG-2.5  8000 Hz
#   row 2  MPEG-2   22050 Hz       row 3  MPEG-2   24000 Hz       row 4  MPEG-2   16000 Hz
#   row 5  MPEG-1   44100 Hz       row 6  MPEG-1   48000 Hz       row 7  MPEG-1   32000 Hz
RATE_ROWS = (("mpeg25", 0), ("mpeg25", 2), ("mpeg2", 0), ("mpeg2", 1), ("mpeg2", 2), ("mpeg1", 0), ("mpeg1", 1), ("mpeg1", 2))
# table index = kind * 8 + row, kind 0 long, 1 short, 2 mixed
REFUSED = 2 * 8 + 1                                # mixed blocks at MPEG-2.5 8 kHz: afg_mp3_parse_q refuses them
MAX_ABS = 8206                                      # 8191 + 15: the largest value 13 linbits can escape to


def requant_numpy(q, granules, sdesc):
    """float32 statement of the device kernel: [blocks, 576] spectra."""
    bol, dst, p43 = afgpu.mp3_qtables()
    f32 = np.float32
    out = np.zeros(q.shape, f32)
    for g in granules:
        nch, b0 = int(g["nch"]), int(g["q_off"]) // 576
        x = np.zeros((nch, 576), f32)
        for c in range(nch):
            v = q[b0 + c].astype(np.int64)
            a = np.abs(v)
            one = g["scale"][c][bol[int(g["table"][c]) & 31]]
            p = np.zeros(576, f32)
            small = a < 129
            p[small] = p43[16 + a[small]]
            big = ~small
            if big.any():                                           # L3_pow_43 for x >= 129
                xb = a[big]
                mult = np.where(xb < 1024, 16, 256).astype(f32)
                xb = np.where(xb < 1024, xb << 3, xb)
                sign = (2 * xb) & 64
                frac = ((xb & 63) - sign).astype(f32) / ((xb & ~63) + sign).astype(f32)
                poly = f32(1.0) + frac * (f32(4.0) / f32(3) + frac * (f32(2.0) / f32(9)))
                p[big] = p43[16 + ((xb + sign) >> 6)] * poly * mult
            r = one.astype(f32) * p
            x[c] = np.where(v == 0, f32(0), np.where(v < 0, -r, r))
        if nch == 2 and g["stereo"]:
            mode = np.full(576, 1, np.uint8)
            fl = fr = None
            if g["stereo"] == 2:
                sd = sdesc[int(g["sdesc"])]
                b = bol[int(g["table"][0]) & 31]
                mode, fl, fr = sd["type"][b], sd["fl"][b], sd["fr"][b]
            a0, a1 = x[0].copy(), x[1].copy()
            ms = mode == 1
            x[0][ms], x[1][ms] = (a0 + a1)[ms], (a0 - a1)[ms]
            if fl is not None:
                it = mode == 2
                x[1][it], x[0][it] = (a0 * fr)[it], (a0 * fl)[it]
        for c in range(nch):
            t = int(g["table"][c])
            if t & 0x80:
                out[b0 + c][dst[t & 31]] = x[c]
            else:
                out[b0 + c] = x[c]
    return out


def band_widths(kind, row):
    """the scalefactor-band widths of table kind * 8 + row, from the generator's tables (mp3_bitstream.band_table)"""
    version, sr = RATE_ROWS[row]
    return mb.band_table(version, sr, 2 if kind else 0, kind == 2)


def long_bands_of_mixed(row):
    """a mixed block keeps 8 long bands at MPEG-1 rates and 6 below (ISO 11172-3 2.4.2.7, 13818-3 2.4.3.2)"""
    return 8 if RATE_ROWS[row][0] == "mpeg1" else 6


@functools.lru_cache(maxsize=None)
def tables_from_bands():
    """(band_of_line uint8 [24, 576], dst_of_src uint16 [24, 576], short_start [24]) from band widths alone.

    band_of_line: band b covers the next widths[b] lines.  dst_of_src: the permutation of L3_reorder (minimp3.d:984-1000).
    The short part is a run of groups of three bands of one width len -- one band per window -- and the line k of window
    w, at s0 + w * len + k, goes to s0 + 3 * k + w: window-major becomes line-interleaved.  Long tables have no short part;
    in a short table it is everything; in a mixed table it begins after the long bands.  short_start is its first line
    (576 for a long table)."""
    bol = np.zeros((24, 576), np.uint8)
    dst = np.tile(np.arange(576, dtype=np.uint16), (24, 1))
    start = np.full(24, 576, np.int64)
    for kind in range(3):
        for row in range(8):
            t = kind * 8 + row
            w = band_widths(kind, row)
            assert sum(w) == 576 and len(w) <= 40, (t, sum(w), len(w))
            bol[t] = np.repeat(np.arange(len(w)), w)
            if kind == 0:
                continue
            first = 0 if kind == 1 else long_bands_of_mixed(row)
            assert (len(w) - first) % 3 == 0
            s0 = start[t] = sum(w[:first])
            for b in range(first, len(w), 3):
                n = w[b]
                assert w[b + 1] == n and w[b + 2] == n
                for win in range(3):
                    dst[t, s0 + win * n + np.arange(n)] = s0 + 3 * np.arange(n) + win
                s0 += 3 * n
    return bol, dst, start


def pow43_64(a):
    """|v| ** (4/3), the requantiser's power (ISO 11172-3 2.4.3.4), in float64"""
    return np.asarray(a, np.float64) ** (4.0 / 3.0)


def pow43_model(a):
    """the model's p for magnitudes a >= 1: the table below 129, L3_pow_43's polynomial above (requant_numpy with scale 1)"""
    a = np.asarray(a, np.int64)
    out = np.zeros(a.size, np.float32)
    g = np.zeros(1, afgpu.MP3_QGRANULE_DTYPE)
    g["nch"], g["sdesc"] = 1, 0xffffffff
    g["scale"][0][0][:] = 1.0
    for at in range(0, a.size, 576):
        q = np.zeros((1, 576), np.int16)
        part = a[at:at + 576]
        q[0, :part.size] = part
        out[at:at + part.size] = requant_numpy(q, g, None)[0, :part.size]
    return out
