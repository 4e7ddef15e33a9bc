"""A float64 model of the CELT transform seam (afg_celt_transform_hip), a named input set and a per-sample error scale.

`run` restates in numpy what the stage computes for one batch of channel sequences, from the definitions and not from the
kernels' factorisation:

    transform   per block the direct inverse-MDCT sum y[m] = imdct_scale * sum_k cos(pi / bs * (m + bs + 0.5) * (k + 0.5)) x[k]
                as a matrix product (`basis`: exact float64 cosines, the angle reduced as an integer multiple of pi / 4bs;
                the normalisation tests/test_oracle_celt.py::test_imdct15_half_matches_direct_sum establishes), short blocks
                read with stride `blocks`
    window      the 120-sample overlap of vector_fmul_window with the float32 table (oracle/celt_tables.h) as float64,
                overlap-added into a 2048-float history laid out as the state blob lays it out (buf + 1024 is the frame)
    filters     both transition stretches and the steady comb with the reference's period / gain bookkeeping (a transition
                whose two leading gains are zero leaves the samples untouched; a filter all of whose gains are zero adds
                exact zeros and is not read), the de-emphasis y[n] = x[n] + 0.85000610f * y[n-1] and the division by 32768
    state       `State`: the AFG_CELT_STATE_FLOATS blob as float64 (periods as numbers), carried in and out

All arithmetic is float64; what separates the float32 oracle (oracle/celt_transform.c) from this model is the oracle's own
rounding and nothing else.  tests/test_celt_model.py pins the model.

The error scale
---------------
Next to the signal the model walks an *envelope* through the same state machine: a value that bounds the magnitude of the
signal at every sample.  A block's direct sum is bounded by A = imdct_scale * sum |x[k]|; the window mixes a = previous
tail and b = new head as a w[119-k] -/+ b w[k], bounded by the same expression with both signs positive; the comb filters
and the de-emphasis are linear with coefficients that enter the envelope as absolute values.  So e[n] >= |signal[n]| at
every sample, by induction, and e decays behind a loud frame exactly as the filters' own memory does and no slower: the
comb's echoes and the 0.85^n tail of the de-emphasis are in it, nothing else is.  The scale is

    scale[n] = 2^-24 * e[n] + 2^-149      where e[n] > 0
    scale[n] = 0                          where e[n] == 0 (zero input from a zero state): the output is +-0, compared exactly

2^-24 * e[n] is half a float32 unit in the last place of the largest value the sample can take; 2^-149 is the float32
subnormal quantum -- the 0.85^n tail behind a loud frame reaches it within one 20 ms frame of silence, and no float32
result is closer to an arbitrary real than half of it.  The scale is computed from the records, the coefficients and this
model only.

The input set
-------------
`cases(level)`: named batches of a handful of frames per sequence, mono sequences and stereo pairs laid out on even / odd
indices as include/afg.h describes (an empty sequence behind an odd number of mono ones).  Legal geometries
(frame_size, blocks) are GEOMETRIES: one block of 120 .. 960 samples, or 2 / 4 / 8 blocks of 120 (blocks is 1, or
1 << duration when transient).  Families: spectrum, scale, postfilter, geometry, cuts; every case at both LEVELS.

Measured on the CPU (tests/test_celt_model.py prints them, run with -s):
    R, the largest |oracle32 - model64| / scale over the input set:           15.93
    (spectrum 15.3 / 15.9, scale 2.8 / 3.1, postfilter 0.65 / 0.61, geometry 0.80 / 0.64, cuts 0.61 / 0.70 at the two
    levels; the maximum is in the 0.85^n tail through a frame of zeros behind a one-hot frame)
    smallest relative perturbation of bin block/2 (one-hot frames) that leaves 4 * R * scale:   2^-17
The device tests bound every sample by 4 * R * scale with R recomputed from the oracle at run time.

The keyword switches of `run` (MUTANTS) each make the model wrong in one place; the bound has to catch every one.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

F32 = np.float32


def _t(*v):
    return np.array(v, F32).astype(np.float64)


# float32 table values (oracle/celt_tables.h, csrc/celt_tables.h) as float64
WINDOW = _t(
    6.7286966e-05, 0.00060551348, 0.0016815970, 0.0032947962, 0.0054439943, 0.0081276923,
    0.011344001, 0.015090633, 0.019364886, 0.024163635, 0.029483315, 0.035319905,
    0.041668911, 0.048525347, 0.055883718, 0.063737999, 0.072081616, 0.080907428,
    0.090207705, 0.099974111, 0.11019769, 0.12086883, 0.13197729, 0.14351214,
    0.15546177, 0.16781389, 0.18055550, 0.19367290, 0.20715171, 0.22097682,
    0.23513243, 0.24960208, 0.26436860, 0.27941419, 0.29472040, 0.31026818,
    0.32603788, 0.34200931, 0.35816177, 0.37447407, 0.39092462, 0.40749142,
    0.42415215, 0.44088423, 0.45766484, 0.47447104, 0.49127978, 0.50806798,
    0.52481261, 0.54149077, 0.55807973, 0.57455701, 0.59090049, 0.60708841,
    0.62309951, 0.63891306, 0.65450896, 0.66986776, 0.68497077, 0.69980010,
    0.71433873, 0.72857055, 0.74248043, 0.75605424, 0.76927895, 0.78214257,
    0.79463430, 0.80674445, 0.81846456, 0.82978733, 0.84070669, 0.85121779,
    0.86131698, 0.87100183, 0.88027111, 0.88912479, 0.89756398, 0.90559094,
    0.91320904, 0.92042270, 0.92723738, 0.93365955, 0.93969656, 0.94535671,
    0.95064907, 0.95558353, 0.96017067, 0.96442171, 0.96834849, 0.97196334,
    0.97527906, 0.97830883, 0.98106616, 0.98356480, 0.98581869, 0.98784191,
    0.98964856, 0.99125274, 0.99266849, 0.99390969, 0.99499004, 0.99592297,
    0.99672162, 0.99739874, 0.99796667, 0.99843728, 0.99882195, 0.99913147,
    0.99937606, 0.99956527, 0.99970802, 0.99981248, 0.99988613, 0.99993565,
    0.99996697, 0.99998518, 0.99999457, 0.99999859, 0.99999982, 1.0000000)
WINDOW2 = _t(
    4.5275357e-09, 3.66647e-07, 2.82777e-06, 1.08557e-05, 2.96371e-05, 6.60594e-05,
    0.000128686, 0.000227727, 0.000374999, 0.000583881, 0.000869266, 0.0012475,
    0.0017363, 0.00235471, 0.00312299, 0.00406253, 0.00519576, 0.00654601,
    0.00813743, 0.00999482, 0.0121435, 0.0146093, 0.017418, 0.0205957,
    0.0241684, 0.0281615, 0.0326003, 0.0375092, 0.0429118, 0.0488308,
    0.0552873, 0.0623012, 0.0698908, 0.0780723, 0.0868601, 0.0962664,
    0.106301, 0.11697, 0.12828, 0.140231, 0.152822, 0.166049,
    0.179905, 0.194379, 0.209457, 0.225123, 0.241356, 0.258133,
    0.275428, 0.293212, 0.311453, 0.330116, 0.349163, 0.368556,
    0.388253, 0.40821, 0.428382, 0.448723, 0.469185, 0.48972,
    0.51028, 0.530815, 0.551277, 0.571618, 0.59179, 0.611747,
    0.631444, 0.650837, 0.669884, 0.688547, 0.706788, 0.724572,
    0.741867, 0.758644, 0.774877, 0.790543, 0.805621, 0.820095,
    0.833951, 0.847178, 0.859769, 0.87172, 0.88303, 0.893699,
    0.903734, 0.91314, 0.921928, 0.930109, 0.937699, 0.944713,
    0.951169, 0.957088, 0.962491, 0.9674, 0.971838, 0.975832,
    0.979404, 0.982582, 0.985391, 0.987857, 0.990005, 0.991863,
    0.993454, 0.994804, 0.995937, 0.996877, 0.997645, 0.998264,
    0.998753, 0.999131, 0.999416, 0.999625, 0.999772, 0.999871,
    0.999934, 0.99997, 0.999989, 0.999997, 0.99999964, 1.0)
assert WINDOW.size == 120 and WINDOW2.size == 120
DEEMPH = float(F32(0.85000610))
TAPS = np.array([[0.3066406250, 0.2170410156, 0.1296386719], [0.4638671875, 0.2680664062, 0.0],
                 [0.7998046875, 0.1000976562, 0.0]], F32)                  # the three tapsets
GAIN_MAX, GAIN_MIN = F32(0.75), F32(0.09375)                                # 0.09375 * (1 .. 8)
NO_GAINS = np.zeros(3, F32)

STATE_FLOATS = 2064                                                        # AFG_CELT_STATE_FLOATS
GEOMETRIES = [(120, 1), (240, 1), (480, 1), (960, 1), (240, 2), (480, 4), (960, 8)]
FRAME_DTYPE = np.dtype([("coef_off", np.uint64), ("out_off", np.uint64), ("out_stride", np.uint32),
                        ("frame_size", np.uint16), ("blocks", np.uint8), ("pad", np.uint8),
                        ("pf_period_new", np.int32), ("pf_gains_new", np.float32, (3,)),
                        ("imdct_scale", np.float32), ("pad2", np.uint32)], align=True)
assert FRAME_DTYPE.itemsize == 48

# keyword -> value that switches the mutant on
MUTANTS = {
    "swap_bins": True,               # bins block/2 - 1 and block/2 of every block swapped
    "window_reversed": True,         # the window index reversed on the side that writes d[119 - k]
    "scale_ignored": True,           # imdct_scale taken as 1
    "period_plus_one": True,         # the steady comb reads one sample further back
    "gains_swapped": True,           # old and new gains swapped in the transitions
    "no_second_transition": True,    # frames above 120 samples skip their second transition stretch
    "deemph_frame_reset": True,      # the de-emphasis memory is not carried across a frame
    "deemph_cut_reset": True,        # the de-emphasis memory is zeroed where csrc/celt_walk.hip may cut a stream
    "block_stride": True,            # block 1 of a transient frame reads its bins one stride too wide
    "overlap_offset": True,          # the first window takes the previous tail from one float earlier in the history
    "bin_gain": 1 + 2.0 ** -10,      # bin block/2 scaled
}


@lru_cache(maxsize=None)
def basis(bs):
    """[m, k] = cos(pi / bs * (m + bs + 0.5) * (k + 0.5)), the angle reduced exactly: (2m + 2bs + 1)(2k + 1) mod 8bs."""
    m = np.arange(bs, dtype=np.int64)[:, None]
    k = np.arange(bs, dtype=np.int64)[None, :]
    q = ((2 * m + 2 * bs + 1) * (2 * k + 1)) % (8 * bs)
    return np.cos(np.pi * q.astype(np.float64) / (4 * bs))


@lru_cache(maxsize=None)
def _deemph_matrix(n):
    """(L, p): y = L @ x + p * m solves y[i] = x[i] + c * y[i-1] with y[-1] * c = m."""
    d = np.arange(n)[:, None] - np.arange(n)[None, :]
    L = np.where(d >= 0, DEEMPH ** np.maximum(d, 0).astype(np.float64), 0.0)
    return L, DEEMPH ** np.arange(n, dtype=np.float64)


def _deemph(x, m):
    """y[i] = x[i] + m, m = y[i] * c.  As a matrix product; sample by sample where a NaN is in it, which a product would
    spread over the samples in front of it."""
    if np.isnan(x).any() or np.isnan(m):
        y = np.empty(x.size)
        for i in range(x.size):
            y[i] = x[i] + m
            m = y[i] * DEEMPH
        return y
    L, p = _deemph_matrix(x.size)
    return L @ x + p * m


class State:
    """The carry state of one channel sequence as float64: `blob` in the layout of afg_celt_state (buf[2048], period,
    gains[3], old period, old gains[3], de-emphasis memory; the periods as numbers), `env` the envelope's history and
    de-emphasis memory in the same slots."""

    def __init__(self):
        self.blob = np.zeros(STATE_FLOATS)
        self.env = np.zeros(STATE_FLOATS)

    def copy(self):
        s = State()
        s.blob[:] = self.blob
        s.env[:] = self.env
        return s


def _comb(buf, lo, n, T, g):
    """celt_postfilter_apply on buf[lo, lo + n): everything a step of T - 2 samples reads is older than the step."""
    if g[0] == 0 or n <= 0:
        return
    for i0 in range(0, n, T - 2):
        i = np.arange(lo + i0, lo + min(i0 + T - 2, n))
        buf[i] += g[0] * buf[i - T] + g[1] * (buf[i - T - 1] + buf[i - T + 1]) + g[2] * (buf[i - T - 2] + buf[i - T + 2])


def _transition(buf, lo, T0, g_old, T1, g):
    """celt_postfilter_apply_transition on buf[lo, lo + 120): the old filter fades out by 1 - window2, the new one in."""
    if g[0] == 0 and g_old[0] == 0:
        return
    live0, live1 = bool(np.any(g_old != 0)), bool(np.any(g != 0))
    step = min([120] + [T - 2 for T, live in ((T0, live0), (T1, live1)) if live])
    for i0 in range(0, 120, step):
        k = np.arange(i0, min(i0 + step, 120))
        i = lo + k
        w = WINDOW2[k]
        acc = np.zeros(k.size)
        if live0:
            acc += (1.0 - w) * (g_old[0] * buf[i - T0] + g_old[1] * (buf[i - T0 - 1] + buf[i - T0 + 1])
                                + g_old[2] * (buf[i - T0 - 2] + buf[i - T0 + 2]))
        if live1:
            acc += w * (g[0] * buf[i - T1] + g[1] * (buf[i - T1 - 1] + buf[i - T1 + 1]) + g[2] * (buf[i - T1 - 2] + buf[i - T1 + 2]))
        buf[i] += acc


def _postfilter(blob, F, rec, mut, envelope=False):
    """celt_postfilter: the bookkeeping of the reference, on blob's history; the frame is blob[1024, 1024 + F).  The
    envelope takes the gains as absolute values."""
    def gains(lo):
        return np.abs(blob[lo:lo + 3]) if envelope else blob[lo:lo + 3].copy()

    def transition():
        T0, T1, g0, g1 = int(blob[2052]), int(blob[2048]), gains(2053), gains(2049)
        if mut.get("gains_swapped"):
            g0, g1 = g1, g0
        return T0, g0, T1, g1

    T0, g0, T1, g1 = transition()
    _transition(blob, 1024, T0, g0, T1, g1)
    blob[2052:2056] = blob[2048:2052]
    blob[2048] = float(rec["pf_period_new"])
    blob[2049:2052] = rec["pf_gains_new"].astype(np.float64)
    if F > 120:
        if not mut.get("no_second_transition"):
            T0, g0, T1, g1 = transition()
            _transition(blob, 1024 + 120, T0, g0, T1, g1)
        _comb(blob, 1024 + 240, F - 240, int(blob[2048]) + (1 if mut.get("period_plus_one") else 0), gains(2049))
        blob[2052:2056] = blob[2048:2052]
    blob[:1084] = blob[F:F + 1084].copy()


def _frame(st, rec, x, mut, cut):
    """One frame of one channel: returns (signal, envelope), frame_size values each, before the division by 32768."""
    F, B = int(rec["frame_size"]), int(rec["blocks"])
    bs = F // B
    assert (F, B) in GEOMETRIES, (F, B)
    scale = 1.0 if mut.get("scale_ignored") else float(rec["imdct_scale"])
    x = x.astype(np.float64)
    k = np.arange(60)
    for j in range(B):
        c = x[j::B].copy()
        if mut.get("block_stride") and j == 1:
            c = x[(1 + np.arange(bs) * (B + 1)) % F]
        if mut.get("swap_bins"):
            c[[bs // 2 - 1, bs // 2]] = c[[bs // 2, bs // 2 - 1]]
        if "bin_gain" in mut:
            c[bs // 2] *= mut["bin_gain"]
        lo = 1024 + j * bs
        st.blob[lo + 60:lo + 60 + bs] = scale * (basis(bs) @ c)
        st.env[lo + 60:lo + 60 + bs] = abs(float(rec["imdct_scale"])) * np.abs(x[j::B]).sum()
        wk, wr = WINDOW[k], WINDOW[119 - k]
        a = st.blob[lo + k - (1 if mut.get("overlap_offset") and j == 0 else 0)].copy()
        b = st.blob[lo + 119 - k].copy()
        st.blob[lo + k] = a * wr - b * wk
        st.blob[lo + 119 - k] = (a * wr + b * wk) if mut.get("window_reversed") else (a * wk + b * wr)
        a, b = st.env[lo + k].copy(), st.env[lo + 119 - k].copy()
        st.env[lo + k] = a * wr + b * wk
        st.env[lo + 119 - k] = a * wk + b * wr
    _postfilter(st.blob, F, rec, mut)
    _postfilter(st.env, F, rec, {}, envelope=True)
    if mut.get("deemph_frame_reset") or (mut.get("deemph_cut_reset") and cut):
        st.blob[2056] = 0.0
    y = _deemph(st.blob[1024 - F:1024], st.blob[2056])
    e = _deemph(st.env[1024 - F:1024], st.env[2056])
    st.blob[2056] = y[-1] * DEEMPH
    st.env[2056] = e[-1] * DEEMPH
    return y, e


def cut_points(seq):
    """Frames q of a sequence of records at which csrc/celt_walk.hip may start a segment (cut_warmup > 0), as {q: W}: the
    W frames before q hold at least 120 + 1026 samples, W <= 12, W < q, and records q - W - 1 .. q - 1 all install filters
    whose three gains are zero."""
    dead = [not np.any(r["pf_gains_new"] != 0) for r in seq]
    cuts = {}
    for q in range(2, len(seq)):
        total = 0
        for w in range(1, 13):
            if w >= q or not dead[q - w]:
                break
            total += int(seq[q - w]["frame_size"])
            if total >= 120 + 1026:
                if dead[q - w - 1]:
                    cuts[q] = w
                break
    return cuts


Result = namedtuple("Result", "out scale written states")
Result.__doc__ = """out: float64 [total], the stage's output; scale: float64 [total], the error scale; written: bool [total];
states: the carry states after the last frame, one per sequence."""


def run(rec_base, recs, coeffs, total, states=None, **mutant):
    """What afg_celt_transform_hip computes, in float64.  states: None (fresh decoders) or one State per sequence (not
    modified).  Keywords: see MUTANTS."""
    unknown = set(mutant) - set(MUTANTS)
    assert not unknown, unknown
    out, env, written = np.zeros(total), np.zeros(total), np.zeros(total, bool)
    coeffs = np.asarray(coeffs, F32)
    final = []
    for c in range(len(rec_base) - 1):
        st = states[c].copy() if states is not None else State()
        seq = recs[int(rec_base[c]):int(rec_base[c + 1])]
        cuts = cut_points(seq) if mutant.get("deemph_cut_reset") else {}
        for q, rec in enumerate(seq):
            F = int(rec["frame_size"])
            y, e = _frame(st, rec, coeffs[int(rec["coef_off"]):int(rec["coef_off"]) + F], mutant, q in cuts)
            at = int(rec["out_off"]) + np.arange(F) * int(rec["out_stride"])
            out[at], env[at], written[at] = y / 32768.0, e / 32768.0, True
        final.append(st)
    scale = np.where(env > 0, env * 2.0 ** -24 + 2.0 ** -149, 0.0)
    return Result(out, scale, written, final)


def ratio(got, res, units=1.0):
    """Per sample |got - model| / (units * scale); where the scale is 0 the sample has to be +-0: 0 if it is, inf if not."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - res.out)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(res.scale > 0, err / (units * res.scale), np.where(got == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


# ------------------------------------------------------------------------------------------------------ the input set ---
Case = namedtuple("Case", "name family rec_base recs coeffs total streams")
Case.__doc__ = """One batch.  streams: per stream (channels, index of its first sequence, frames); `family` names the group
the measured ratios are reported by."""

LEVELS = {"programme": 0.05, "native": 1.0}        # times the generators' native level (rms 1.8 of full scale, +5 dB)


def _frame_of(size, blocks, coef, period=0, gains=NO_GAINS, scale=1.0):
    coef = np.atleast_2d(np.asarray(coef, F32))
    assert coef.shape[1] == size and (size, blocks) in GEOMETRIES
    return dict(size=size, blocks=blocks, coef=coef, period=int(period), gains=np.asarray(gains, F32), scale=float(scale))


def shaped(rng, size, level, channels=1):
    """The spectrum of afgpu.synthetic.celt_batch: Gaussian lines falling 40 dB over the frame."""
    k = np.arange(size, dtype=np.float64)
    return (rng.standard_normal((channels, size)) * 2000.0 * level * 10.0 ** (-(k / size) * 2.0)).astype(F32)


def flat(rng, size, blocks, level, channels=1):
    """Gaussian lines of one level in every bin, at about the output level of `shaped`."""
    return (rng.standard_normal((channels, size)) * 1400.0 * level * (960.0 / (size // blocks)) ** 0.5).astype(F32)


def onehot(size, blocks, bin_, block, level, sign=1.0):
    c = np.zeros((1, size), F32)
    c[0, bin_ * blocks + block] = sign * 60000.0 * level
    return c


def build(name, family, streams):
    """streams: list of lists of frames (a frame's coef is [channels, size]).  Sequence order: the streams' channels in
    turn, an empty sequence in front of a stereo stream that would start on an odd index (and wherever `streams` holds
    None); output interleaved per stream."""
    recs, rec_base, coefs, info = [], [0], [], []
    coef_off = out_base = 0
    for frames in streams:
        if frames is None:
            rec_base.append(len(recs))
            continue
        C = frames[0]["coef"].shape[0]
        assert C in (1, 2) and all(f["coef"].shape[0] == C for f in frames)
        if C == 2 and (len(rec_base) - 1) % 2:
            rec_base.append(len(recs))
        info.append((C, len(rec_base) - 1, frames))
        starts = np.concatenate([[0], np.cumsum([f["size"] for f in frames])])
        for c in range(C):
            for i, f in enumerate(frames):
                coefs.append(f["coef"][c])
                recs.append((coef_off, out_base + int(starts[i]) * C + c, C, f["size"], f["blocks"], 0, f["period"],
                             tuple(f["gains"]), f["scale"], 0))
                coef_off += f["size"]
            rec_base.append(len(recs))
        out_base += int(starts[-1]) * C
    return Case(name, family, np.array(rec_base, np.uint64), np.array(recs, FRAME_DTYPE), np.concatenate(coefs), out_base, info)


def _spectrum_cases(seed, level):
    out = []
    for F, B in GEOMETRIES:
        bs = F // B
        rng = np.random.default_rng([seed, 1, F, B])
        zero = _frame_of(F, B, np.zeros((1, F), F32))
        streams = []
        bins = (0, 1, bs // 2 - 1, bs // 2, bs - 1)
        for i, b in enumerate(bins):                # one-hot, a frame of zeros, one-hot in another block with the other sign
            streams.append([_frame_of(F, B, onehot(F, B, b, i % B, level)), zero,
                            _frame_of(F, B, onehot(F, B, b, (i + 1) % B, level, -1.0))])
        # zeros from a zero state (+0 then -0 lines), then a flat frame: the exact-zero rule and its end
        streams.append([zero, _frame_of(F, B, -np.zeros((1, F), F32)), _frame_of(F, B, flat(rng, F, B, level))])
        streams.append([_frame_of(F, B, flat(rng, F, B, level, 2)), _frame_of(F, B, np.zeros((2, F), F32)),
                        _frame_of(F, B, flat(rng, F, B, level, 2))])
        streams.append([_frame_of(F, B, np.concatenate([onehot(F, B, 0, B - 1, level), onehot(F, B, bs - 1, 0, level)])),
                        _frame_of(F, B, np.zeros((2, F), F32)),
                        _frame_of(F, B, np.concatenate([onehot(F, B, bs - 1, B - 1, level), onehot(F, B, 0, 0, level)]))])
        out.append(build(f"spectrum-{F}x{B}", "spectrum", streams))
    return out


def _live(rng, size, blocks, level, C, period=0, gains=NO_GAINS, scale=1.0):
    return _frame_of(size, blocks, shaped(rng, size, level, C), period, gains, scale)


def _scale_cases(seed, level):
    rng = np.random.default_rng([seed, 2])
    g = GAIN_MAX * TAPS[0]
    streams = [
        [_live(rng, 960, 1, level, 1, scale=0.5) for _ in range(4)],                                   # long, downmixed
        [_live(rng, 960, 8, level, 1, scale=0.5) for _ in range(3)],                                   # transient
        [_live(rng, 480, 4, level, 1, 100, g, 0.5) for _ in range(3)],                                 # ... with a live filter
        [_live(rng, 960, 1, level, 1, scale=1.0), _live(rng, 960, 8, level, 1, scale=0.5),             # 0.5 and 1.0 mixed
         _live(rng, 480, 1, level, 1, scale=1.0), _live(rng, 120, 1, level, 1, scale=0.5), _live(rng, 240, 2, level, 1, scale=0.5)],
        [_frame_of(960, 1, onehot(960, 1, 0, 0, level), scale=0.5), _frame_of(960, 1, onehot(960, 1, 959, 0, level), scale=0.5)],
        [_live(rng, 960, 1, level, 2, scale=s) for s in (0.5, 1.0, 0.5)],                              # as a pair
    ]
    return [build("scale", "scale", streams)]


def _pf_stream(rng, level, C, geo, plan):
    """plan: per frame (period, gains); geo: per frame (size, blocks) or one geometry for all."""
    geo = geo if isinstance(geo, list) else [geo] * len(plan)
    return [_live(rng, F, B, level, C, T, g) for (F, B), (T, g) in zip(geo, plan)]


def _postfilter_cases(seed, level):
    rng = np.random.default_rng([seed, 3])
    top = [GAIN_MAX * TAPS[i] for i in range(3)]
    low = GAIN_MIN * TAPS[0]
    out = []
    # the shortest period: 13-sample steps
    out.append(build("pf-period15", "postfilter", [
        _pf_stream(rng, level, 1, (120, 1), [(15, top[0])] * 6), _pf_stream(rng, level, 2, (960, 1), [(15, top[2])] * 4),
        _pf_stream(rng, level, 1, (480, 4), [(15, top[1])] * 4)]))
    # the longest on 120-sample frames: the taps reach -T - 2 = 1024 samples back, the first float of the history; the
    # signal of frame 0 is under them from frame 8 on
    out.append(build("pf-period1022-120", "postfilter", [
        _pf_stream(rng, level, 1, (120, 1), [(1022, top[0])] * 12), _pf_stream(rng, level, 2, (120, 1), [(1022, top[2])] * 12)]))
    # period = frame size - 2, frame size, frame size + 2
    streams = []
    for F in (120, 480, 960):
        for T in (F - 2, F, F + 2):
            streams.append(_pf_stream(rng, level, 1, (F, 1), [(T, top[(T // 2) % 3])] * 4))
    streams.append(_pf_stream(rng, level, 2, (960, 1), [(958, top[0]), (960, top[1]), (962, top[2]), (960, low)]))
    out.append(build("pf-period-near-frame", "postfilter", streams))
    # old period != new period, both gains live: every transition cross-fades two different combs
    plan = [(100, top[0]), (333, low), (20, top[2]), (1022, top[1]), (15, top[0])]
    out.append(build("pf-change", "postfilter", [
        _pf_stream(rng, level, 2, (960, 1), plan), _pf_stream(rng, level, 1, (240, 2), plan), _pf_stream(rng, level, 1, (120, 1), plan),
        _pf_stream(rng, level, 1, (960, 8), plan[::-1])]))
    # on, off, on with the period kept (the gains are reset, the period is not)
    plan = [(200, top[1]), (200, NO_GAINS), (200, top[1]), (200, top[0]), (200, NO_GAINS), (200, low)]
    out.append(build("pf-on-off-on", "postfilter", [
        _pf_stream(rng, level, 2, (960, 1), plan), _pf_stream(rng, level, 1, (120, 1), plan), _pf_stream(rng, level, 1, (480, 1), plan)]))
    # each tapset at the largest gain
    streams = [_pf_stream(rng, level, 2, (960, 1), [(64, top[i])] * 4) for i in range(3)]
    streams += [_pf_stream(rng, level, 1, (120, 1), [(64, top[i])] * 6) for i in range(3)]
    out.append(build("pf-tapsets", "postfilter", streams))
    return out


def _geometry_cases(seed, level):
    rng = np.random.default_rng([seed, 4])
    g = GAIN_MAX * TAPS[0]
    out = []
    for name, pf in (("geometry", (0, NO_GAINS)), ("geometry-filtered", (100, g))):
        L, S, T = (960, 1), (120, 1), (240, 2)
        streams = [
            _pf_stream(rng, level, 2, [L, S, L], [pf] * 3), _pf_stream(rng, level, 1, [S, L, S], [pf] * 3),
            _pf_stream(rng, level, 2, [L, T, L, T], [pf] * 4), _pf_stream(rng, level, 1, [T, L, (480, 4), (960, 8), (240, 1)], [pf] * 5),
            _pf_stream(rng, level, 2, S, [pf] * 8), _pf_stream(rng, level, 1, S, [pf] * 8)]
        out.append(build(name, "geometry", streams))
    return out


# csrc/celt_walk.hip, cut_warmup: frame q is a cut when the W frames before it hold at least 120 + 1026 samples and records
# q - W - 1 .. q - 1 all install dead filters.  960-sample frames: W = 2, so the shortest idle run is 3 records; 120-sample
# frames: W = 10, 11 records.  CUT_CASES: name -> (frame size, idle records, period of the filter that comes back).
CUT_CASES = {
    "cut-960": (960, 3, 200), "nocut-960": (960, 2, 200), "cut-960-reach": (960, 3, 1022), "nocut-960-reach": (960, 2, 1022),
    "cut-120": (120, 11, 200), "nocut-120": (120, 10, 200), "cut-120-reach": (120, 11, 1022), "nocut-120-reach": (120, 10, 1022),
}


def _cut_cases(seed, level):
    out = []
    for i, (name, (F, idle, T)) in enumerate(CUT_CASES.items()):
        rng = np.random.default_rng([seed, 5, i])
        on, back = GAIN_MAX * TAPS[0], GAIN_MAX * TAPS[2]
        plan = [(300, on)] + [(300, NO_GAINS)] * idle + [(T, back)] * 2
        out.append(build(name, "cuts", [_pf_stream(rng, level, 2, (F, 1), plan), _pf_stream(rng, level, 1, (F, 1), plan)]))
    return out


@lru_cache(maxsize=None)
def cases(level="programme", seed=2025):
    """The input set at one of LEVELS, deterministic in `seed`; names carry no level."""
    lv = LEVELS[level]
    return tuple(_spectrum_cases(seed, lv) + _scale_cases(seed, lv) + _postfilter_cases(seed, lv) + _geometry_cases(seed, lv)
                 + _cut_cases(seed, lv))


def model_of(case, **mutant):
    return run(case.rec_base, case.recs, case.coeffs, case.total, **mutant)


def select(case, lo, hi):
    """Records [lo, hi) of every sequence of a case (fewer where a sequence is shorter): (rec_base, recs) of that chunk."""
    base, sel = [0], []
    for c in range(len(case.rec_base) - 1):
        b, n = int(case.rec_base[c]), int(case.rec_base[c + 1]) - int(case.rec_base[c])
        sel.append(np.arange(b + min(lo, n), b + min(hi, n)))
        base.append(base[-1] + sel[-1].size)
    return np.array(base, np.uint64), case.recs[np.concatenate(sel)].copy()
