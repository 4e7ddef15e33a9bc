"""QOA encoder (csrc/qoa_encode.hip) where it can go wrong with ordinary audio green: the float input conversion at and
beyond full scale, full-scale material for whole frames, ties between scalefactors, and every way two streams share a
wavefront.  Expected bytes always come from the CPU oracle (oraclelib.qoa_encode) on int16 PCM; where the input is float
the int16 PCM comes from `float_to_s16`, a float64 / int64 restatement of the conversion include/afg.h defines, which is
itself held to a hand-written table.  Every comparison is byte-exact over the whole file, and the output plane of every
launch starts as 0xA5 between two runs of guard bytes that must survive."""
import numpy as np
import pytest

import afgpu
import oraclelib
from test_qoa_encode_gpu import make_pcm

GUARD = 64
FRAME = 5120


# ------------------------------------------------------------------ the conversion (include/afg.h, "QOA encoder") ---
def float_to_s16(x):
    """v = 32768.5 + x * 32767 in double; t = trunc(v) when -2^31 - 1 < v < 2^31, else INT32_MIN (NaN included);
    the low 16 bits of t - 32768 in two's complement."""
    v = 32768.5 + np.asarray(x).astype(np.float64) * 32767.0
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    t = np.where(ok, np.trunc(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64)
    return ((((t - 32768) & 0xffff) ^ 0x8000) - 0x8000).astype(np.int16)


F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]
UP1 = np.nextafter(F32(1), F32(2))
# (value, the int16 the encoder must see), worked out by hand from the definition
SPECIALS = [
    (F32(1.0), 32767), (F32(-1.0), -32767),                      # v = 65535.5, 1.5
    (UP1, 32767), (-UP1, -32767),                                # v = 65535.504, 1.496
    (F32(1.0001), -32766), (F32(-1.0001), 32767),                # t = 65538 -> 32770 wraps; t = -1 -> -32769 wraps
    (F32(1.5), -16385), (F32(-1.5), 16386),                      # t = 81919, -16382
    (F32(2.0), -2), (F32(-2.0), 3),                              # t = 98302, -32765
    (F32(3.0), 32765), (F32(-3.0), -32764),                      # t = 131069, -65532
    (F32(65535.0), -32767), (F32(-65535.0), -32768),             # t = 2147418113, -2147352576: the last ones in range
    (F32(65537.0), 32767), (F32(-65537.0), -32766),              # v = 2147483647.5 (just inside), -2147418110.5
    (F32(1e6), -32768), (F32(-1e6), -32768),                     # from here on out of range: INT32_MIN - 32768 -> 0x8000
    (F32(1e9), -32768), (F32(-1e9), -32768),
    (F32(3e38), -32768), (F32(-3e38), -32768),
    (INF, -32768), (-INF, -32768), (NAN, -32768), (NEG_NAN, -32768),
    (F32(0.0), 0), (F32(-0.0), 0), (F32(1e-9), 0), (F32(-1e-9), 0),  # v = 32768.5 +- 0.00003
]
# (k + 0.5) / 32767 sits on the truncation boundary v = 32769 + k: the float32 nearest to it falls on either side
BOUNDARY_K = [0, 1, 2, 7, 100, 12345, 32766, -1, -2, -3, -8, -101, -12346, -32767]


def special_values():
    return np.array([v for v, _ in SPECIALS] + [F32((k + 0.5) / 32767.0) for k in BOUNDARY_K], np.float32)


def c1_streams():
    """A stereo stream of 5120 + 300 frames and a mono one of 41: noise at 0.3 RMS with every special value in the first
    frame, every one again in the second, and a few in the mono stream, its one-sample last slice included."""
    rng = np.random.default_rng(101)
    a = (rng.standard_normal((FRAME + 300, 2)) * 0.3).astype(np.float32)
    b = (rng.standard_normal((41, 1)) * 0.3).astype(np.float32)
    sp = special_values()
    flat = a.reshape(-1)
    flat[37 + (2 * FRAME // len(sp)) * np.arange(len(sp))] = sp                   # first frame: flat index < 10240
    flat[2 * FRAME + 5 + (590 // len(sp)) * np.arange(len(sp))] = sp[::-1]        # second frame: the last 600
    b[[0, 19, 20, 39, 40], 0] = [INF, F32(1.0001), F32(-1.5), NAN, F32(-1.0001)]
    return a, b


def test_restatement_reproduces_the_table_of_specials():
    vals = np.array([v for v, _ in SPECIALS], np.float32)
    want = [s for _, s in SPECIALS]
    assert float_to_s16(vals).tolist() == want
    assert float_to_s16(vals.astype(np.float64)).tolist() == want
    got = float_to_s16(np.array([F32((k + 0.5) / 32767.0) for k in BOUNDARY_K], np.float32)).astype(int)
    k = np.array(BOUNDARY_K)
    assert ((got == k) | (got == k + 1)).all(), got
    assert (got == k).any() and (got == k + 1).any()                              # both sides of the boundary occur
    a, b = c1_streams()
    for x in (a, b):
        assert np.isinf(x).any() and np.isnan(x).any()
    assert np.isin(special_values()[:len(SPECIALS)].view(np.uint32), a[:FRAME].view(np.uint32)).all()
    assert np.isin(special_values()[:len(SPECIALS)].view(np.uint32), a[FRAME:].view(np.uint32)).all()
    # in-range values keep the plain expression the earlier tests use
    x = np.linspace(-1, 1, 100001).astype(np.float32)
    assert np.array_equal(float_to_s16(x), (32768.5 + x.astype(np.float64) * 32767.0).astype(np.int64) - 32768)


# ------------------------------------------------------------------------------------------------- device helpers ---
def first_difference(got, want):
    got, want = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8)
    if got.size != want.size:
        return f"{got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else f"{bad.size} of {want.size} bytes differ, the first at offset {int(bad[0])}"


def encode_guarded(gpu, blocks, rate):
    """One launch over `blocks` (all int16 or all float32, [frames, channels] each).  The files abut in one output plane
    that starts as 0xA5 and lies between two guard runs; the input plane ends in samples no stream owns."""
    import torch
    dtype = blocks[0].dtype
    assert dtype in (np.int16, np.float32) and all(b.dtype == dtype for b in blocks)
    recs, n_in, n_out = afgpu.qoa_encode_layout([b.shape for b in blocks], rate)
    tail = np.full(16, 0x5555 if dtype == np.int16 else np.nan, dtype)
    d_in = torch.from_numpy(np.concatenate([b.reshape(-1) for b in blocks] + [tail])).to(gpu)
    d_all = torch.full((GUARD + n_out + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(gpu)
    if dtype == np.int16:
        afgpu.qoa_encode(len(recs), d_recs, d_all[GUARD:GUARD + n_out], d_pcm_i16=d_in)
    else:
        afgpu.qoa_encode(len(recs), d_recs, d_all[GUARD:GUARD + n_out], d_pcm_f32=d_in)
    torch.cuda.synchronize()
    out = d_all.cpu().numpy()
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n_out:] == 0xA5).all(), "guard bytes around the output plane"
    out = out[GUARD:GUARD + n_out]
    sizes = [afgpu.qoa_encoded_size(*b.shape) for b in blocks]
    assert sum(sizes) == n_out and [int(r["out_off"]) for r in recs] == np.cumsum([0] + sizes[:-1]).tolist()   # they abut
    return [out[int(r["out_off"]): int(r["out_off"]) + n] for r, n in zip(recs, sizes)]


def check_against_oracle(gpu, blocks, rate, pcm=None):
    """pcm: the int16 the encoder must see, when `blocks` are float."""
    got = encode_guarded(gpu, blocks, rate)
    for k, (b, g) in enumerate(zip(blocks if pcm is None else pcm, got)):
        want, _ = oraclelib.qoa_encode(b, rate)
        diff = first_difference(g, want)
        assert diff is None, f"stream {k} {b.shape}: {diff}"
    return got


def write_stream(x, rate, double, floats_first=0):
    """floats_first: frames written as floats before the rest goes as doubles (the host then converts what it queued)."""
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_QOA, rate, x.shape[1])
    assert not st.isError(), st.errorMessage()
    if floats_first:
        assert st.writeSamplesFloat(x[:floats_first]) == floats_first
        x = x[floats_first:]
    n = st.writeSamplesDouble(x.astype(np.float64)) if double else st.writeSamplesFloat(x)
    assert n == len(x) and not st.isError()
    data = st.finalizeAndGetEncodedResult()
    st.cleanUp()
    return data


# ------------------------------------------------------------------------------------ C1: float conversion edges ---
@pytest.mark.gpu
def test_float_input_at_and_beyond_full_scale(gpu):
    """The direct kernel call, the float write and the double write, each against the oracle.  While load_sample kept the
    unnarrowed int, the direct call's first stream differed from the oracle in 1930 of its 4424 bytes, the first at
    offset 441: the slice that holds the first sample beyond full scale."""
    a, b = c1_streams()
    pcm = [float_to_s16(a), float_to_s16(b)]
    check_against_oracle(gpu, [a, b], 48000, pcm)
    for x, s in zip((a, b), pcm):
        want, _ = oraclelib.qoa_encode(s, 48000)
        for double in (False, True):
            diff = first_difference(write_stream(x, 48000, double), want)
            assert diff is None, f"{'double' if double else 'float'} write {x.shape}: {diff}"
        diff = first_difference(write_stream(x, 48000, True, floats_first=len(x) // 2), want)
        assert diff is None, f"floats, then doubles {x.shape}: {diff}"


# -------------------------------------------------------------------------- C2: full-scale material, whole frames ---
def c2_streams():
    n = 2 * FRAME + 777
    t = np.arange(n)
    square = np.where((t[:, None] + np.array([0, 3])[None, :]) % 14 < 7, 32767, -32768).astype(np.int16)
    noise = np.random.default_rng(202).integers(-32768, 32768, (n, 2)).astype(np.int16)
    held = np.where((t // FRAME) % 2 == 0, -32768, 32767).astype(np.int16)[:, None].repeat(2, 1)
    return [square, noise, np.ascontiguousarray(held)]


@pytest.mark.gpu
@pytest.mark.parametrize("as_float", [False, True], ids=["int16", "float"])
def test_full_scale_material_for_whole_frames(gpu, as_float):
    pcm = c2_streams()
    assert all(p.min() == -32768 and p.max() == 32767 for p in (pcm[0], pcm[2])) and int(pcm[1].max()) - int(pcm[1].min()) > 65000
    if not as_float:
        check_against_oracle(gpu, pcm, 44100)
        return
    blocks = [(p / 32767.0).astype(np.float32) for p in pcm]
    for p, x in zip(pcm, blocks):
        assert np.array_equal(float_to_s16(x), p)                                 # the restatement gives s back
    check_against_oracle(gpu, blocks, 44100, pcm)


# ----------------------------------------------------------------------------------------------------- C3: ties ---
RECIPROCAL = np.array([65536, 9363, 3121, 1457, 781, 475, 311, 216, 156, 117, 90, 71, 57, 47, 39, 32], np.int64)
QUANT = np.array([7, 7, 7, 5, 5, 3, 3, 1, 0, 0, 2, 2, 4, 4, 6, 6, 6], np.int64)
DEQUANT_MAG = np.array([
    1, 3, 5, 7,  5, 18, 32, 49,  16, 53, 95, 147,  34, 113, 203, 315,  63, 210, 378, 588,  104, 345, 621, 966,
    158, 528, 950, 1477,  228, 760, 1368, 2128,  316, 1053, 1895, 2947,  422, 1405, 2529, 3934,
    548, 1828, 3290, 5117,  696, 2320, 4176, 6496,  868, 2893, 5207, 8099,  1064, 3548, 6386, 9933,
    1286, 4288, 7718, 12005,  1536, 5120, 9216, 14336], np.int64).reshape(16, 4)
DEQUANT = np.stack([DEQUANT_MAG, -DEQUANT_MAG], 2).reshape(16, 8)


def wrap32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def trial_errors(x):
    """x: int64 [N, n], the first slice (n <= 20 samples) of N channels.  The squared error of each of the 16
    scalefactors from the encoder's start state, [N, 16]: one slice trial of qoa.d:336-370 in wrapped 32-bit integers,
    without the early break, which only leaves a losing trial unfinished.  Used to choose inputs, never as a reference."""
    N, n = x.shape
    err = np.zeros((N, 16), np.int64)
    for sf in range(16):
        w = np.tile(np.array([0, 0, -(1 << 13), 1 << 14], np.int64), (N, 1))
        h = np.zeros((N, 4), np.int64)
        for j in range(n):
            predicted = wrap32((w * h).sum(1)) >> 13
            residual = x[:, j] - predicted
            q = wrap32(residual * RECIPROCAL[sf] + (1 << 15)) >> 16
            q = q + np.sign(residual) - np.sign(q)
            d = DEQUANT[sf, QUANT[np.clip(q, -8, 8) + 8]]
            rec = np.clip(predicted + d, -32768, 32767)
            err[:, sf] += (x[:, j] - rec) ** 2
            w = wrap32(w + np.where(h < 0, -(d >> 4)[:, None], (d >> 4)[:, None]))
            h = np.concatenate([h[:, 1:], rec[:, None]], 1)
    return err


def tied_scalefactors(x):
    """[N, 16] mask of the scalefactors that share the smallest error of each row of x; all False for a lone winner."""
    err = trial_errors(x)
    tied = err == err.min(1, keepdims=True)
    return tied & (tied.sum(1, keepdims=True) > 1)


def c3_streams():
    """Streams of 1 to 3 samples, 1 or 2 channels.  Returns (streams, per stream and channel the mask of tied scalefactors,
    all False where the winner stands alone)."""
    rng = np.random.default_rng(303)
    columns, masks = [], []                                                       # channels: [n] int64 and [16] bool
    for n in (1, 2, 3):
        if n == 1:
            x = np.arange(-32768, 32768, dtype=np.int64)[:, None]                 # every one-sample channel there is
        else:
            mag = np.minimum(10 ** rng.uniform(0, 4.52, (20000, n)), 32767)       # all loudnesses alike
            x = (mag * rng.choice([-1, 1], (20000, n))).astype(np.int64)
        tied = tied_scalefactors(x)
        rows = np.concatenate([np.flatnonzero(tied.any(1)), np.flatnonzero(~tied.any(1))[:40]])   # and some lone winners
        columns += [x[r] for r in rows]
        masks += [tied[r] for r in rows]
    streams, stream_masks = [], []
    for c, m in zip(columns, masks):                                              # every channel as a mono stream
        streams.append(c.astype(np.int16)[:, None])
        stream_masks.append([m])
    for n in (1, 2, 3):                                                           # and in stereo with a neighbour of its length
        same = [k for k, c in enumerate(columns) if len(c) == n]
        for k0, k1 in zip(same, same[1:] + same[:1]):
            streams.append(np.stack([columns[k0], columns[k1]], 1).astype(np.int16))
            stream_masks.append([masks[k0], masks[k1]])
    return streams, stream_masks


def has_gap(mask):
    sf = np.flatnonzero(mask)
    return len(sf) > 1 and sf[1] - sf[0] > 1


def test_tie_search_finds_ties_and_the_oracle_keeps_the_smallest():
    """The search meets its counts, and the oracle's winner is the smallest tied scalefactor of every tied slice: a
    kernel that resolved ties towards the larger one would write another scalefactor nibble into each of these slices."""
    streams, masks = c3_streams()
    flat = [m for ms in masks for m in ms]
    assert sum(m.any() for m in flat) >= 8
    assert sum(has_gap(m) for m in flat) >= 2
    assert all(1 <= s.shape[0] <= 3 and 1 <= s.shape[1] <= 2 for s in streams) and 200 <= len(streams) <= 1000
    for s, ms in zip(streams, masks):
        want, _ = oraclelib.qoa_encode(s, 44100)
        err = trial_errors(s.T.astype(np.int64))
        for c in range(s.shape[1]):
            sf = int(want[8 + 8 + 16 * s.shape[1] + 8 * c] >> 4)                  # the slice's top four bits
            assert sf == int(np.argmin(err[c]))                                   # the restatement agrees with the oracle
            if ms[c].any():
                assert sf == int(np.flatnonzero(ms[c])[0]) and sf != int(np.flatnonzero(ms[c])[-1])


@pytest.mark.gpu
def test_ties_go_to_the_smallest_scalefactor(gpu):
    streams, masks = c3_streams()
    tied = sum(m.any() for ms in masks for m in ms)
    gapped = sum(has_gap(m) for ms in masks for m in ms)
    assert tied >= 8 and gapped >= 2, (tied, gapped)
    check_against_oracle(gpu, streams, 44100)


# -------------------------------------------------------------------------------------------------- C4: packing ---
C4_SHAPES = [(100, 1), (50, 3),                 # narrow beside wide: one after the other because of the partner
             (60, 5), (FRAME + 1, 2),           # wide beside narrow
             (0, 2), (FRAME * 2 + 19, 1),       # an empty stream beside a long one
             (FRAME * 3, 2), (20, 2),           # three frames beside one slice: the short side idles for whole frames
             (0, 1), (0, 8),                    # two empty streams
             (21, 4)]                           # no partner, four channels wide


@pytest.mark.gpu
def test_wavefront_packing(gpu):
    rng = np.random.default_rng(404)
    blocks = [make_pcm(rng, n, c) for n, c in C4_SHAPES]
    got = check_against_oracle(gpu, blocks, 44100)
    for b, g in zip(blocks, got):
        if len(b) == 0:                         # an empty stream still owes its file header, and nothing else
            assert g.tobytes() == b"qoaf" + bytes(4)
    back = check_against_oracle(gpu, blocks[::-1], 44100)[::-1]                   # every stream changes partner
    for g, r in zip(got, back):
        assert np.array_equal(g, r)
