"""A float64 model of the MP3 transform stage (afg_mp3_transform_hip), a full-band input set and a per-block error scale.

`transform64` restates in numpy, vectorised over the granules of a stream, what the stage computes for one batch: alias
reduction, IMDCT36 or 3 x IMDCT12 with overlap, frequency inversion, the 32-point DCT-II and the 512-tap polyphase window
with its 15-slot history, samples 0 and 16 of every slot (mp3d_synth_pair) included; AFG_MP3_SUBBAND blocks skip the first
three.  The constants are the float32 table values of oracle/mp3_transform.c converted to float64, the transforms are the
fast forms of that file, and all arithmetic is float64: what separates the float32 oracle from this model is the oracle's
own rounding and nothing else.  tests/test_mp3_model.py pins the model against the oracle.

`fullband_cases` is the input set: unlike afgpu.synthetic.mp3_batch (zero above line 418, -45 dB at subband 20) every
subband carries data, and the flag word takes every value the header allows.  Flat spectra are N(0, 1) lines times
FLAT_LEVEL = 0.0015: the stage's gain on such lines, measured with the oracle over the flat case, is 33.5, and the oracle's
PCM over that case has an RMS of 0.0503 (0.0450 over the flags case).

`block_scale` is the error scale of an output block (stream, g, channel): 2^-24 * (L[g] + L[g-1] + L[g-2]), L the sum of
|line| over the channel's 576 lines of a granule -- PCM(g) depends on X[g], X[g-1] and X[g-2] only (csrc/mp3_transform.hip).

Measured on the CPU (tests/test_mp3_model.py prints them):
    R, the largest |oracle32 - model64| / scale over the input set:          23.8
    (per case: flat 1.84, onehot 23.8, flags 1.26, nzbands 2.81; a one-hot block's 18 lines add up in phase, a flat
    block's 576 do not, so the same rounding is a larger share of the line sum there)
    smallest relative perturbation of one band (29, one-hot streams) that
    leaves the bound 4 * R * scale:                                           2^-16
The device tests bound every sample by 4 * R * scale with R recomputed from the oracle at run time.

The keyword switches of `transform64` (MUTANTS) each make the model wrong in one place; the bound has to catch every one.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32


def _t(*v):
    return np.array(v, F32).astype(np.float64)


# float32 table values (oracle/mp3_transform.c, csrc/mp3_kernel.h) as float64
AA_CS = _t(0.85749293, 0.88174200, 0.94962865, 0.98331459, 0.99551782, 0.99916056, 0.99989920, 0.99999316)
AA_CA = _t(0.51449576, 0.47173197, 0.31337745, 0.18191320, 0.09457419, 0.04096558, 0.01419856, 0.00369997)
TWID9 = _t(0.73727734, 0.79335334, 0.84339145, 0.88701083, 0.92387953, 0.95371695, 0.97629601, 0.99144486, 0.99904822,
           0.67559021, 0.60876143, 0.53729961, 0.46174861, 0.38268343, 0.30070580, 0.21643961, 0.13052619, 0.04361938)
TWID3 = _t(0.79335334, 0.92387953, 0.99144486, 0.60876143, 0.38268343, 0.13052619)
MDCT_WINDOW = np.stack([
    _t(0.99904822, 0.99144486, 0.97629601, 0.95371695, 0.92387953, 0.88701083, 0.84339145, 0.79335334, 0.73727734,
       0.04361938, 0.13052619, 0.21643961, 0.30070580, 0.38268343, 0.46174861, 0.53729961, 0.60876143, 0.67559021),
    _t(1, 1, 1, 1, 1, 1, 0.99144486, 0.92387953, 0.79335334, 0, 0, 0, 0, 0, 0, 0.13052619, 0.38268343, 0.60876143)])
SEC = _t(10.19000816, 0.50060302, 0.50241929, 3.40760851, 0.50547093, 0.52249861, 2.05778098, 0.51544732,
         0.56694406, 1.48416460, 0.53104258, 0.64682180, 1.16943991, 0.55310392, 0.78815460, 0.97256821,
         0.58293498, 1.06067765, 0.83934963, 0.62250412, 1.72244716, 0.74453628, 0.67480832, 5.10114861)
C9 = _t(0.5, 0.93969262, 0.76604444, 0.17364818, 0.86602540, 0.98480775, 0.34202014, 0.64278761)
C8 = _t(0.70710677, 0.198912367, 0.382683432, 0.50979561, 0.54119611, 0.60134488, 0.89997619, 1.30656302, 2.56291556)
G_WIN = _t(
    -1, 26, -31, 208, 218, 401, -519, 2063, 2000, 4788, -5517, 7134, 5959, 35640, -39336, 74992,
    -1, 24, -35, 202, 222, 347, -581, 2080, 1952, 4425, -5879, 7640, 5288, 33791, -41176, 74856,
    -1, 21, -38, 196, 225, 294, -645, 2087, 1893, 4063, -6237, 8092, 4561, 31947, -43006, 74630,
    -1, 19, -41, 190, 227, 244, -711, 2085, 1822, 3705, -6589, 8492, 3776, 30112, -44821, 74313,
    -1, 17, -45, 183, 228, 197, -779, 2075, 1739, 3351, -6935, 8840, 2935, 28289, -46617, 73908,
    -1, 16, -49, 176, 228, 153, -848, 2057, 1644, 3004, -7271, 9139, 2037, 26482, -48390, 73415,
    -2, 14, -53, 169, 227, 111, -919, 2032, 1535, 2663, -7597, 9389, 1082, 24694, -50137, 72835,
    -2, 13, -58, 161, 224, 72, -991, 2001, 1414, 2330, -7910, 9592, 70, 22929, -51853, 72169,
    -2, 11, -63, 154, 221, 36, -1064, 1962, 1280, 2006, -8209, 9750, -998, 21189, -53534, 71420,
    -2, 10, -68, 147, 215, 2, -1137, 1919, 1131, 1692, -8491, 9863, -2122, 19478, -55178, 70590,
    -3, 9, -73, 139, 208, -29, -1210, 1870, 970, 1388, -8755, 9935, -3300, 17799, -56778, 69679,
    -3, 8, -79, 132, 200, -57, -1283, 1817, 794, 1095, -8998, 9966, -4533, 16155, -58333, 68692,
    -4, 7, -85, 125, 189, -83, -1356, 1759, 605, 814, -9219, 9959, -5818, 14548, -59838, 67629,
    -4, 7, -91, 117, 177, -106, -1428, 1698, 402, 545, -9416, 9916, -7154, 12980, -61289, 66494,
    -5, 6, -97, 111, 163, -127, -1498, 1634, 185, 288, -9585, 9838, -8540, 11455, -62684, 65290).reshape(15, 16)
PAIR0 = (29.0, 213.0, 459.0, 2037.0, 5153.0, 6574.0, 37489.0, 75038.0)
PAIR16 = ((14, 104.0), (12, 1567.0), (10, 9727.0), (8, 64019.0), (6, -9975.0), (4, -45.0), (2, 146.0), (0, -5.0))

SUBBAND = 0x80000000
FLAT_LEVEL = 0.0015

# keyword -> value that switches the mutant on
MUTANTS = {
    "no_inversion_27": True,         # no frequency inversion in band 27
    "aa_one_more": True,             # alias boundary aa|aa+1 is mixed too
    "aa_skip_last": True,            # boundary 30|31 skipped when aa = 31
    "short_gt": True,                # short window where band > n_long
    "stop_gt": True,                 # stop window where band > n_long
    "swap_stop_31": True,            # stop and normal windows swapped in band 31
    "drop_overlap_31": True,         # band 31's overlap not carried into the next granule
    "swap_ch_31": True,              # band 31 of the two channels swapped
    "gwin_gain_7": 1 + 2.0 ** -10,   # one g_win entry of column pair 7 scaled
    "band_gain": (29, 1 + 2.0 ** -10),   # one band scaled
}


def flag_word(block_type, n_long, aa, nz=None, subband=False):
    """AFG_MP3_FLAGS(block_type, n_long, aa) [| AFG_MP3_NZ_BANDS(nz)] [| AFG_MP3_SUBBAND] (include/afg.h)."""
    w = int(block_type) | (int(n_long) << 8) | ((int(aa) + 1) << 16)
    if nz is not None:
        w |= (int(nz) + 1) << 24
    if subband:
        w |= SUBBAND
    return w


# ------------------------------------------------------------------------------------------------------- the stage ---
def _dct3_9(y):
    h, c1, c2, c3, c4, c5, c6, c7 = C9
    e0, e2, e4, e6, e8 = y[0], y[2], y[4], y[6], y[8]
    m0 = e0 + e6 * h
    e0 = e0 - e6
    m4 = (e4 + e2) * c1
    m2 = (e8 + e2) * c2
    e6 = (e4 - e8) * c3
    e4 = e4 + (e8 - e2)
    e2 = e0 - e4 * h
    y4 = e4 + e0
    e8 = m0 - m2 + e6
    e0 = m0 - m4 + m2
    e4 = m0 + m4 - e6
    o1, o3, o5, o7 = y[1], y[3], y[5], y[7]
    o3 = o3 * c4
    m0 = (o5 + o1) * c5
    m4 = (o5 - o7) * c6
    m2 = (o1 + o7) * c7
    o1 = (o1 - o5 - o7) * c4
    o5 = m0 - o3 - m2
    o7 = m4 - o3 - m0
    o3 = m4 + o3 - m2
    return [e4 - o7, e2 + o1, e0 - o3, e8 + o5, y4, e8 - o5, e0 + o3, e2 - o1, e4 + o7]


def _imdct36_core(t):
    """t[18] lines -> (sum[9], overlap[9]); the windowing with the previous overlap is the caller's."""
    co, si = [None] * 9, [None] * 9
    co[0] = -t[0]
    si[0] = t[17]
    for i in range(4):
        si[8 - 2 * i] = t[4 * i + 1] - t[4 * i + 2]
        co[1 + 2 * i] = t[4 * i + 1] + t[4 * i + 2]
        si[7 - 2 * i] = t[4 * i + 4] - t[4 * i + 3]
        co[2 + 2 * i] = -(t[4 * i + 3] + t[4 * i + 4])
    co, si = _dct3_9(co), _dct3_9(si)
    for i in (1, 3, 5, 7):
        si[i] = -si[i]
    s = [co[i] * TWID9[9 + i] + si[i] * TWID9[i] for i in range(9)]
    ov = [co[i] * TWID9[i] - si[i] * TWID9[9 + i] for i in range(9)]
    return s, ov


def _idct3(x0, x1, x2):
    m1 = x1 * C9[4]
    a1 = x0 - x2 * C9[0]
    return [a1 + m1, x0 + x2, a1 - m1]


def _imdct12_core(t, off):
    co = _idct3(-t[off], t[off + 6] + t[off + 3], t[off + 12] + t[off + 9])
    si = _idct3(t[off + 15], t[off + 12] - t[off + 9], t[off + 6] - t[off + 3])
    si[1] = -si[1]
    s = [co[i] * TWID3[3 + i] + si[i] * TWID3[i] for i in range(3)]
    ov = [co[i] * TWID3[i] - si[i] * TWID3[3 + i] for i in range(3)]
    return s, ov


def _imdct12_window(ovl, s):
    d = [None] * 6
    for i in range(3):
        d[i] = ovl[i] * TWID3[2 - i] - s[i] * TWID3[5 - i]
        d[5 - i] = ovl[i] * TWID3[5 - i] + s[i] * TWID3[2 - i]
    return d


def _hybrid(x, f, mut):
    """One channel of one stream: spectra x[G, 32, 18], flag words f[G] -> subband samples [G, 32, 18]."""
    bt = (f & 3).astype(np.int64)[:, None]
    n_long = ((f >> 8) & 0xff).astype(np.int64)[:, None]
    aa = ((f >> 16) & 0xff).astype(np.int64)[:, None] - 1
    sub = (f >> 31) != 0
    assert sub.all() or not sub.any(), "AFG_MP3_SUBBAND holds for every block of a stream or for none"
    if sub.all():
        return x.copy()
    band = np.arange(32)[None, :]

    # alias reduction: boundary b | b+1 for b < aa
    edge = band[:, :31]
    mix = edge < aa
    if mut.get("aa_one_more"):
        mix = edge <= aa
    if mut.get("aa_skip_last"):
        mix = mix & ~((aa == 31) & (edge == 30))
    mix = mix[:, :, None]
    up = x[:, 1:, 0:8]
    dn = x[:, :-1, 17:9:-1]                        # line 17 - i of the band below
    y = x.copy()
    y[:, 1:, 0:8] = np.where(mix, up * AA_CS - dn * AA_CA, up)
    y[:, :-1, 17:9:-1] = np.where(mix, up * AA_CA + dn * AA_CS, dn)

    t = np.moveaxis(y, 2, 0)                       # [18, G, 32]
    is_short = (bt == 2) & ((band > n_long) if mut.get("short_gt") else (band >= n_long))
    stop = (bt == 3) & ((band > n_long) if mut.get("stop_gt") else (band >= n_long))
    if mut.get("swap_stop_31"):
        stop = np.where(band == 31, ~stop, stop)

    sum36, ov36 = _imdct36_core(t)
    parts = [_imdct12_core(t, off) for off in range(3)]
    ov12 = _imdct12_window(parts[1][1], parts[2][0]) + parts[2][1]
    new_ov = np.stack([np.where(is_short, ov12[i], ov36[i]) for i in range(9)])        # [9, G, 32]
    ovl = np.zeros_like(new_ov)
    ovl[:, 1:] = new_ov[:, :-1]
    if mut.get("drop_overlap_31"):
        ovl[:, :, 31] = 0.0

    win = np.where(stop[None], MDCT_WINDOW[1][:, None, None], MDCT_WINDOW[0][:, None, None])   # [18, G, 32]
    long_out = [None] * 18
    for i in range(9):
        long_out[i] = ovl[i] * win[i] - sum36[i] * win[9 + i]
        long_out[17 - i] = ovl[i] * win[9 + i] + sum36[i] * win[i]
    short_out = [ovl[i] for i in range(6)] + _imdct12_window(ovl[6:9], parts[0][0]) + _imdct12_window(parts[0][1], parts[1][0])
    out = np.stack([np.where(is_short, short_out[i], long_out[i]) for i in range(18)])   # [18, G, 32]

    # frequency inversion: odd lines of odd bands
    odd = (np.arange(32) & 1).astype(bool)
    if mut.get("no_inversion_27"):
        odd[27] = False
    out[1::2] = np.where(odd, -out[1::2], out[1::2])
    return np.moveaxis(out, 0, 2)


def _dct2_32(x):
    """x[32] (subbands) -> V[32]."""
    t = [[None] * 8 for _ in range(4)]
    for i in range(8):
        x0, x1, x2, x3 = x[i], x[15 - i], x[16 + i], x[31 - i]
        t0 = x0 + x3
        t1 = x1 + x2
        t2 = (x1 - x2) * SEC[3 * i + 0]
        t3 = (x0 - x3) * SEC[3 * i + 1]
        t[0][i] = t0 + t1
        t[1][i] = (t0 - t1) * SEC[3 * i + 2]
        t[2][i] = t3 + t2
        t[3][i] = (t3 - t2) * SEC[3 * i + 2]
    for r in t:
        x0, x1, x2, x3, x4, x5, x6, x7 = r
        xt = x0 - x7; x0 = x0 + x7
        x7 = x1 - x6; x1 = x1 + x6
        x6 = x2 - x5; x2 = x2 + x5
        x5 = x3 - x4; x3 = x3 + x4
        x4 = x0 - x3; x0 = x0 + x3
        x3 = x1 - x2; x1 = x1 + x2
        r[0] = x0 + x1
        r[4] = (x0 - x1) * C8[0]
        x5 = x5 + x6
        x6 = (x6 + x7) * C8[0]
        x7 = x7 + xt
        x3 = (x3 + x4) * C8[0]
        x5 = x5 - x7 * C8[1]
        x7 = x7 + x5 * C8[2]
        x5 = x5 - x7 * C8[1]
        x0 = xt - x6; xt = xt + x6
        r[1] = (xt + x7) * C8[3]
        r[2] = (x4 + x3) * C8[4]
        r[3] = (x0 - x5) * C8[5]
        r[5] = (x0 + x5) * C8[6]
        r[6] = (x4 - x3) * C8[7]
        r[7] = (xt - x7) * C8[8]
    out = [None] * 32
    for i in range(7):
        out[4 * i + 0] = t[0][i]
        out[4 * i + 1] = t[2][i] + t[3][i] + t[3][i + 1]
        out[4 * i + 2] = t[1][i] + t[1][i + 1]
        out[4 * i + 3] = t[2][i + 1] + t[3][i] + t[3][i + 1]
    out[28] = t[0][7]
    out[29] = t[2][7] + t[3][7]
    out[30] = t[1][7]
    out[31] = t[3][7]
    return out


def _synthesis(s, mut):
    """Subband samples s[G, 32, 18] of one channel -> PCM [G*18, 32] (slot, sample), zero history before slot 0."""
    G = s.shape[0]
    T = G * 18
    v = np.stack(_dct2_32([s[:, b, :].reshape(T) for b in range(32)]), 1)      # V[t, q]
    p = np.concatenate([np.zeros((15, 32)), v])                                 # p[15 + t] = V of slot t
    win = G_WIN.copy()
    if "gwin_gain_7" in mut:
        win[14 - 7, 13] *= mut["gwin_gain_7"]
    wr = win[::-1]                                  # column pair i uses row 14 - i
    hi = p[:, 31:16:-1]                             # V[31 - i], i = 0..14
    lo = p[:, 1:16]                                 # V[1 + i]
    a = np.zeros((T, 15))
    b = np.zeros((T, 15))
    for k in range(8):
        w0, w1 = wr[:, 2 * k], wr[:, 2 * k + 1]
        vz = (lo if k & 1 else hi)[15 - k:15 - k + T]                           # slot t - k
        vy = (hi if k & 1 else lo)[k:k + T]                                     # slot t - 15 + k
        b += vz * w1 + vy * w0
        a += (vy * w1 - vz * w0) if k & 1 else (vz * w0 - vy * w1)
    pcm = np.zeros((T, 32))
    pcm[:, 15:0:-1] = a
    pcm[:, 17:32] = b
    # samples 0 and 16: z[m] = slot t - 15 + m, V[16] and V[0]
    z16 = [p[m:m + T, 16] for m in range(15)]
    z0 = [p[m:m + T, 0] for m in range(15)]
    c = PAIR0
    pcm[:, 0] = ((z16[14] - z16[0]) * c[0] + (z16[1] + z16[13]) * c[1] + (z16[12] - z16[2]) * c[2] + (z16[3] + z16[11]) * c[3]
                 + (z16[10] - z16[4]) * c[4] + (z16[5] + z16[9]) * c[5] + (z16[8] - z16[6]) * c[6] + z16[7] * c[7])
    pcm[:, 16] = sum(z0[m] * w for m, w in PAIR16)
    return pcm / 32768.0


def transform64(granules, channels, coef, flags, **mutant):
    """What afg_mp3_transform_hip computes, in float64: float64 [blocks * 576] in the layout of oraclelib.mp3_transform
    (per granule: slot, sample, channel).  Keywords: see MUTANTS."""
    unknown = set(mutant) - set(MUTANTS)
    assert not unknown, unknown
    coef = np.asarray(coef, F32).reshape(-1, 576).astype(np.float64)
    flags = np.asarray(flags, np.uint32)
    out = np.zeros(coef.shape[0] * 576)
    blk = 0
    for ng, nc in zip(map(int, granules), map(int, channels)):
        n = ng * nc
        if n:
            x = coef[blk:blk + n].reshape(ng, nc, 32, 18)
            f = flags[blk:blk + n].reshape(ng, nc)
            if "band_gain" in mutant:
                x = x.copy()
                x[:, :, mutant["band_gain"][0]] *= mutant["band_gain"][1]
            s = [_hybrid(x[:, c], f[:, c], mutant) for c in range(nc)]
            if mutant.get("swap_ch_31") and nc == 2:
                s[0][:, 31], s[1][:, 31] = s[1][:, 31].copy(), s[0][:, 31].copy()
            pcm = np.stack([_synthesis(s[c], mutant) for c in range(nc)], -1)   # [G*18, 32, nc]
            out[blk * 576:(blk + n) * 576] = pcm.reshape(-1)
        blk += n
    return out


# --------------------------------------------------------------------------------------------------- the error scale ---
def block_scale(coef, granules, channels):
    """float64 [blocks]: 2^-24 * (L[g] + L[g-1] + L[g-2]) of block (stream, g, channel), L = sum |line| of a granule."""
    L = np.abs(np.asarray(coef, F32).reshape(-1, 576).astype(np.float64)).sum(1)
    out = np.zeros_like(L)
    blk = 0
    for ng, nc in zip(map(int, granules), map(int, channels)):
        n = ng * nc
        l = L[blk:blk + n].reshape(ng, nc)
        acc = l.copy()
        acc[1:] += l[:-1]
        acc[2:] += l[:-2]
        out[blk:blk + n] = acc.reshape(-1) * 2.0 ** -24
        blk += n
    return out


def per_sample(block_values, granules, channels):
    """Spread one value per block (stream, g, channel) over that block's samples in the PCM layout: [blocks * 576]."""
    out = np.zeros(block_values.size * 576, block_values.dtype)
    blk = 0
    for ng, nc in zip(map(int, granules), map(int, channels)):
        n = ng * nc
        v = block_values[blk:blk + n].reshape(ng, 1, nc)
        out[blk * 576:(blk + n) * 576] = np.broadcast_to(v, (ng, 576, nc)).reshape(-1)
        blk += n
    return out


def per_block(sample_values, granules, channels, reduce=np.max):
    """The inverse view: reduce the samples of every block (stream, g, channel) of a PCM-layout array to one value."""
    out = np.zeros(sample_values.size // 576, sample_values.dtype)
    blk = 0
    for ng, nc in zip(map(int, granules), map(int, channels)):
        n = ng * nc
        if n:
            out[blk:blk + n] = reduce(sample_values[blk * 576:(blk + n) * 576].reshape(ng, 576, nc), axis=1).reshape(-1)
        blk += n
    return out


# ------------------------------------------------------------------------------------------------------ the input set ---
Case = namedtuple("Case", "name granules channels coef flags declared")
Case.__doc__ = """One batch: `flags` without AFG_MP3_NZ_BANDS; `declared` the same words with it (None: nothing to declare)."""

LONG = flag_word(0, 0, 31)
FLAG_COMBOS = ([(0, 0, aa) for aa in range(-1, 32)] + [(2, 0, -1), (2, 2, 1), (2, 4, 3)]
               + [(1, n, 31) for n in (0, 2, 4)] + [(3, n, 31) for n in (0, 2, 4)])


def _flat(rng, ng, nc):
    return (rng.standard_normal((ng, nc, 576)) * FLAT_LEVEL).astype(F32)


def _batch(name, streams, declare=False):
    """streams: list of (coef[G, C, 576] f32, flags[G, C]) -> Case."""
    granules = [c.shape[0] for c, _ in streams]
    channels = [c.shape[1] for c, _ in streams]
    coef = np.concatenate([c.reshape(-1) for c, _ in streams]).astype(F32)
    words = np.concatenate([np.asarray(f, np.uint32).reshape(-1) for _, f in streams])
    nz_bits = np.uint32(63 << 24)
    return Case(name, granules, channels, coef, words & ~nz_bits, words if declare else None)


def _flat_case(seed):
    streams = []
    for nc in (1, 2):
        for ng in (1, 2, 3, 5, 66, 131):
            rng = np.random.default_rng([seed, 1, nc, ng])
            streams.append((_flat(rng, ng, nc), np.full((ng, nc), LONG, np.uint32)))
    streams.append(streams.pop(0))                  # a mono stream ends the plane
    return _batch("flat", streams)


def _onehot_case(seed):
    streams = []
    for b in range(32):
        for nc in (2, 1):
            rng = np.random.default_rng([seed, 2, nc, b])
            c = np.zeros((4, nc, 32, 18), F32)
            full = _flat(rng, 4, nc).reshape(4, nc, 32, 18)
            c[:, 0, b] = full[:, 0, b]
            if nc == 2:
                c[:, 1, 31 - b] = full[:, 1, 31 - b]
            streams.append((c.reshape(4, nc, 576), np.full((4, nc), LONG, np.uint32)))
    return _batch("onehot", streams)


def _typed(n_long):
    """long, start, short, short, stop, long, long with the given n_long: a legal sequence."""
    return [LONG, flag_word(1, n_long, 31), flag_word(2, n_long, n_long - 1), flag_word(2, n_long, n_long - 1),
            flag_word(3, n_long, 31), LONG, LONG]


def _flags_case(seed):
    streams = []
    rng = np.random.default_rng([seed, 3])
    # long blocks with every aa_bands
    sweep = np.array([flag_word(0, 0, aa) for aa in range(-1, 32)] + [LONG], np.uint32)
    streams.append((_flat(rng, len(sweep), 1), sweep[:, None]))
    streams.append((_flat(rng, len(sweep), 2), np.stack([sweep, sweep[::-1]], 1)))
    # start / short / stop with n_long 0, 2, 4
    for n_long in (0, 2, 4):
        a, b = np.array(_typed(n_long), np.uint32), np.array(_typed((n_long + 2) % 6), np.uint32)
        streams.append((_flat(rng, len(a), 1), a[:, None]))
        streams.append((_flat(rng, len(a), 2), np.stack([a, b], 1)))
    # a constant cycle of start, short, short, stop, long; the second channel two granules behind and mixed (n_long 2)
    cyc0 = np.array([flag_word(1, 0, 31), flag_word(2, 0, -1), flag_word(2, 0, -1), flag_word(3, 0, 31), LONG] * 4, np.uint32)
    cyc1 = np.array([LONG, LONG] + [flag_word(1, 2, 31), flag_word(2, 2, 1), flag_word(2, 2, 1), flag_word(3, 2, 31), LONG] * 4,
                    np.uint32)[:len(cyc0)]
    streams.append((_flat(rng, len(cyc0), 2), np.stack([cyc0, cyc1], 1)))
    # subband samples (Layer I / II), all 32 subbands filled
    for nc in (2, 1):
        streams.append((_flat(rng, 5, nc), np.full((5, nc), flag_word(0, 0, 31, subband=True), np.uint32)))
    return _batch("flags", streams)


def _nzbands_case(seed):
    streams = []
    rng = np.random.default_rng([seed, 4])

    def stream(ng, nc, counts, words):
        c = _flat(rng, ng, nc).reshape(ng, nc, 32, 18)
        counts = np.broadcast_to(np.asarray(counts), (ng, nc))
        for g in range(ng):
            for ch in range(nc):
                c[g, ch, counts[g, ch]:] = 0.0       # +0.0
        w = np.broadcast_to(np.asarray(words, np.uint32).reshape(-1, 1), (ng, nc))
        streams.append((c.reshape(ng, nc, 576), w | ((counts.astype(np.uint32) + 1) << 24)))

    for i, n in enumerate((0, 1, 17, 31, 32)):
        stream(4, 1 + i % 2, n, [LONG] * 4)
    cyc = [LONG, LONG, flag_word(1, 0, 31), flag_word(2, 0, -1), flag_word(3, 0, 31)] * 14
    stream(70, 2, rng.integers(0, 33, (70, 2)), cyc)          # varies per granule and channel; more than 64 granules
    stream(9, 1, rng.integers(0, 33, (9, 1)), [LONG] * 9)
    return _batch("nzbands", streams, declare=True)


def fullband_cases(seed=2024):
    """The input set: four batches (flat, onehot, flags, nzbands), deterministic in `seed`.

    flat     all 576 lines N(0, 1) * FLAT_LEVEL, long blocks; 1, 2, 3, 5, 66 and 131 granules, mono and stereo, a mono stream last
    onehot   per subband b one stereo and one mono stream of 4 granules: only band b's 18 lines are nonzero, the stereo
             stream's second channel carries band 31 - b
    flags    flat spectra under every (block type, n_long, aa) of FLAG_COMBOS in legal sequences, a constant
             start/short/short/stop/long cycle that differs between the channels, and AFG_MP3_SUBBAND streams
    nzbands  flat spectra zeroed above a declared count of 0, 1, 17, 31, 32 subbands and above per-granule varying counts;
             `declared` carries AFG_MP3_NZ_BANDS
    """
    return [_flat_case(seed), _onehot_case(seed), _flags_case(seed), _nzbands_case(seed)]


# ------------------------------------------------------------------------------------------------------ the reference ---
Reference = namedtuple("Reference", "case oracle32 model64 scale ratio")
Reference.__doc__ = """Per case: the oracle's float32 PCM, the model's float64 PCM, the per-sample scale and, per block,
the largest |oracle32 - model64| / scale (0 where the scale is 0)."""


def ratio_per_block(got, ref, units=1.0):
    """Per block of ref.case: max over its samples of |got - model64| / (units * scale); blocks of zero scale give 0 if
    they are exactly zero and inf if not."""
    c = ref.case
    err = np.abs(np.asarray(got, np.float64) - ref.model64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.scale > 0, err / (units * ref.scale), np.where(err == 0, 0.0, np.inf))
    return per_block(r, c.granules, c.channels)


def measure(cases, oracle):
    """(references, R): `oracle` is oraclelib.mp3_transform.  R is the float32 reference's own rounding in units of
    the scale, the largest ratio over every block of every case."""
    refs = []
    for c in cases:
        o = oracle(c.granules, c.channels, c.coef, c.flags)
        m = transform64(c.granules, c.channels, c.coef, c.flags)
        ref = Reference(c, o, m, per_sample(block_scale(c.coef, c.granules, c.channels), c.granules, c.channels), None)
        refs.append(ref._replace(ratio=ratio_per_block(o, ref)))
    return refs, max(float(r.ratio.max()) for r in refs)
