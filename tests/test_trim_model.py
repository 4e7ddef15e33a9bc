"""tests/trim_model.py against arithmetic that does not share its order: the region against math.fsum powers of explicitly
centred frames and librosa.effects.trim's index arithmetic, the blocks' powers against math.fsum, and the corner cases of the
definition in include/afg.h."""
import math

import numpy as np
import pytest

import trim_model as tm

U64 = 2.0 ** -53
SHAPES = [(2048, 512), (400, 200), (10, 5), (64, 64)]            # (frame_length, hop): k = 4, 2, 2, 1


def independent(x, prm):
    """(begin, end without the margins, P, thr): frame f is the frame_length samples centred on sample f * hop (k == 1: the
    hop samples from f * hop on), cut to the signal; its power the exactly rounded sum of the squares of all rows; the region
    as librosa.effects.trim has it -- nonzero = flatnonzero(non_silent); start = frames_to_samples(nonzero[0], hop);
    end = min(length, frames_to_samples(nonzero[-1] + 1, hop))"""
    rows, valid = x.shape
    hop, fl = prm["hop"], prm["frame_length"]
    n_frames = -(-valid // hop)
    P = []
    for f in range(n_frames):
        lo, hi = (f * hop, (f + 1) * hop) if fl == hop else (f * hop - fl // 2, f * hop + fl // 2)
        lo, hi = max(lo, 0), min(hi, valid)
        P.append(math.fsum(float(v) * float(v) for r in range(rows) for v in x[r, lo:hi]))
    if prm["reference"] == tm.REF_ABS:
        thr = prm["ratio"] * prm["abs_power"] * (rows * fl)
    else:
        thr = prm["ratio"] * max(P, default=0.0)
    nonzero = [f for f, p in enumerate(P) if p > thr]
    if not nonzero:
        return 0, 0, P, thr
    return nonzero[0] * hop, min(valid, (nonzero[-1] + 1) * hop), P, thr


def signals(rng, valid):
    """name -> [rows, valid] float32"""
    t = np.arange(valid)
    tone = np.sin(2 * np.pi * 0.013 * t) * 0.5
    a, b = valid // 4 + 3, valid - valid // 3 - 7
    burst = np.zeros(valid)
    burst[a:b] = tone[a:b]
    floor = rng.standard_normal(valid) * 1e-4
    fade = tone * np.clip(np.minimum(t - valid * 0.2, valid * 0.85 - t) / (valid * 0.25), 0.0, 1.0) ** 4
    two = np.zeros(valid)
    g0, g1 = valid // 2 - valid // 12, valid // 2 + valid // 12
    two[valid // 6:g0] = tone[valid // 6:g0]
    two[g1:valid - valid // 5] = 0.25 * tone[g1:valid - valid // 5]
    return {"burst in silence": burst[None], "burst on a noise floor": (burst + floor)[None], "fade": (fade + floor)[None],
            "two bursts": two[None], "anti-phase stereo": np.stack([burst, -burst]),
            "three rows": np.stack([burst + floor, 0.5 * burst, rng.standard_normal(valid) * 1e-4])}


@pytest.mark.parametrize("frame_length,hop", SHAPES)
def test_regions_equal_the_independent_statement(frame_length, hop):
    rng = np.random.default_rng(frame_length + hop)
    valid = 13 * frame_length + hop // 2 + 1 if frame_length <= 400 else 5 * frame_length + 333
    for lead, trail, top_db in ((0, 0, 60.0), (hop + 1, 2 * hop + 3, 30.0)):
        prm = tm.params(top_db, frame_length, hop, lead=lead, trail=trail)
        for name, x in signals(rng, valid).items():
            x = x.astype(np.float32)
            b, e, P, thr = independent(x, prm)
            # a condition on the inputs: no frame within a relative 1e-6 of the threshold, so that the order of a sum cannot decide
            assert thr > 0 and all(abs(p - thr) > 1e-6 * thr for p in P), name
            begin, end, ref, S, mine = tm.region(x, prm)
            assert (begin, end) == (max(b - lead, 0), min(valid, e + trail)), name
            assert 0 < b < e < valid and begin < end, name       # every signal has silence at both ends
            assert abs(ref - max(P)) <= 1e-12 * max(P)
            assert all(abs(m - p) <= 1e-12 * max(P) for m, p in zip(mine, P))


def test_block_powers_are_within_the_bound_of_recursive_summation():
    """any order of n float64 adds is within (n - 1) u sum|x| of the exact sum (Higham, Accuracy and Stability, 4.2); the
    squares of float32 are exact in float64"""
    rng = np.random.default_rng(5)
    for rows, valid, hop in ((1, 1, 512), (1, 700, 512), (2, 2049, 512), (3, 1000, 200), (2, 333, 5), (1, 130, 64), (1, 200000, 65536)):
        x = (rng.standard_normal((rows, valid)) * 10.0 ** rng.integers(-3, 3, (rows, valid))).astype(np.float32)
        S = tm.block_powers(x, hop)
        assert S.size == -(-valid // hop)
        for j, s in enumerate(S):
            part = [float(v) for v in x[:, j * hop:(j + 1) * hop].ravel()]
            exact = math.fsum(v * v for v in part)
            assert abs(s - exact) <= len(part) * U64 * exact, (rows, valid, hop, j)
    # the order shows: a plain running sum over a block gives other bits somewhere
    x = (rng.standard_normal((1, 4096)) * 10.0 ** rng.integers(-3, 3, (1, 4096))).astype(np.float32)
    S = tm.block_powers(x, 512)
    plain = [float(np.add.accumulate(x[0, j * 512:(j + 1) * 512].astype(np.float64) ** 2)[-1]) for j in range(8)]
    assert plain != [float(s) for s in S]


def spike(valid, at, rows=1):
    x = np.zeros((rows, valid), np.float32)
    x[:, at] = 1.0
    return x


def test_corner_cases():
    prm = tm.params(60.0, 2048, 512)
    # all silent: no frame above 0 * ratio
    begin, end, ref, S, P = tm.region(np.zeros((2, 5000), np.float32), prm)
    assert (begin, end) == (0, 0) and ref == 0 and not np.signbit(ref) and S.size == 10 and (P == 0).all()
    # no samples at all
    assert tm.region(np.zeros((1, 0), np.float32), prm)[:3] == (0, 0, 0.0)
    # all loud
    assert tm.region(np.full((1, 5000), 0.25, np.float32), prm)[:2] == (0, 5000)
    # one loud sample at index 0: block 0 lies in frames 0 .. k / 2; at valid - 1: block n_blocks - 1 in frames n_blocks - k / 2 ..
    assert tm.region(spike(5000, 0), prm)[:2] == (0, 3 * 512)
    assert tm.region(spike(5000, 4999), prm)[:2] == (8 * 512, 5000)
    assert tm.region(spike(5000, 4999), tm.params(60.0, 512, 512))[:2] == (9 * 512, 5000)      # k = 1: block f alone
    assert tm.region(spike(5000, 1024), tm.params(60.0, 512, 512))[:2] == (1024, 1536)
    for case in (spike(5000, 0), spike(5000, 4999), spike(5000, 1024, rows=3)):
        for p in (prm, tm.params(60.0, 512, 512), tm.params(60.0, 10, 5)):
            assert tm.region(case, p)[:2] == independent(case, p)[:2]
    # valid < hop and valid < frame_length: one frame, or a few short ones
    assert tm.region(spike(300, 7), prm)[:2] == (0, 300)
    assert tm.region(spike(1500, 1400), prm)[:2] == (512, 1500) == independent(spike(1500, 1400), prm)[:2]
    assert tm.region(spike(1500, 1400), tm.params(60.0, 1024, 512))[:2] == (1024, 1500)
    # lead and trail are clamped to the signal
    x = spike(5000, 2600)                                        # block 5: frames 4 .. 7 -> [2048, 4096)
    assert tm.region(x, prm)[:2] == (2048, 4096)
    assert tm.region(x, tm.params(60.0, 2048, 512, lead=48, trail=4))[:2] == (2000, 4100)
    assert tm.region(x, tm.params(60.0, 2048, 512, lead=2047, trail=903))[:2] == (1, 4999)
    assert tm.region(x, tm.params(60.0, 2048, 512, lead=2048, trail=904))[:2] == (0, 5000)
    assert tm.region(x, tm.params(60.0, 2048, 512, lead=2049, trail=905))[:2] == (0, 5000)
    assert tm.region(x, tm.params(60.0, 2048, 512, lead=2 ** 32 - 1, trail=2 ** 32 - 1))[:2] == (0, 5000)


def test_nan_and_infinity():
    prm = tm.params(60.0, 1024, 512)                             # k = 2: frame f is blocks f - 1 and f
    x = np.full((1, 5120), 0.5, np.float32)
    x[0, :1024] = 0.0
    x[0, 1030] = np.nan                                          # block 2: frames 2 and 3 are NaN, hence silent
    begin, end, ref, S, P = tm.region(x, prm)
    assert np.isnan(S[2]) and np.isnan(P[2]) and np.isnan(P[3]) and not np.isnan(np.delete(P, [2, 3])).any()
    assert (begin, end) == (4 * 512, 5120) and ref == 1024 * 0.25
    assert tm.region(np.full((1, 700), np.nan, np.float32), prm)[:3] == (0, 0, 0.0)      # nothing but NaN: a NaN never wins
    # an infinity: the reference is infinite, and no power is above ratio * inf
    x[0, 1030] = np.inf
    begin, end, ref, _, _ = tm.region(x, prm)
    assert (begin, end) == (0, 0) and ref == np.inf
    # ... but above an absolute threshold it is
    begin, end, ref, _, _ = tm.region(x, tm.params(20.0, 1024, 512, reference=tm.REF_ABS, abs_power=1.0))
    assert (begin, end) == (1024, 5120) and ref == np.inf


def test_absolute_reference():
    """threshold = ratio * abs_power * (rows * frame_length): a frame is loud when its mean square per sample is above
    ratio * abs_power"""
    x = np.zeros((2, 6000), np.float32)
    x[:, 2048:4096] = 0.1                                        # mean square 0.01 where a frame is full
    x[:, :2048] = 0.001
    for top_db, want in ((19.0, (0, 0)), (21.0, (3072, 3584)), (50.0, (1536, 5120)), (61.0, (1024, 5120))):
        prm = tm.params(top_db, 2048, 512, reference=tm.REF_ABS, abs_power=1.0)
        got = tm.region(x, prm)
        assert got[:2] == want == independent(x, prm)[:2], top_db
        assert got[2] == max(got[4])                            # ref_power is P_ref in this mode too
    # abs_power scales it: 20 dB below 0.1 is 30 dB below 1
    a = tm.region(x, tm.params(20.0, 2048, 512, reference=tm.REF_ABS, abs_power=0.1))[:2]
    assert a == tm.region(x, tm.params(30.0, 2048, 512, reference=tm.REF_ABS, abs_power=1.0))[:2] != (0, 0)


def test_output_and_layout():
    rng = np.random.default_rng(3)
    prm = tm.params(60.0, 10, 5)
    plane = rng.standard_normal(400).astype(np.float32)
    plane[20:60] = 0
    plane[100:160] = 0
    plane[220:260] = 0
    g = np.zeros(3, tm.GROUP_DTYPE)
    g[0] = (20, 3, 100, 50, 0, 0, 2, 100, 3, 30)                 # rows 20 .. 119 and 120 .. 219; loud in [60, 100) and [160, 220)
    g[1] = (0, 160, 0, 0, 0, 0, 1, 0, 1, 7)                      # no samples: a zero slab
    g[2] = (220, 170, 0, 0, 0, 0, 1, 150, 1, 200)
    assert tm.layout(g, prm) == (20 + 0 + 30, 3 + 1 + 1)
    assert g["first_block"].tolist() == [0, 20, 20] and g["first_tile"].tolist() == [0, 3, 4]
    out0 = np.full(400, 9.0, np.float32)
    out, regions, powers = tm.trim(plane, out0, g, prm)
    assert powers.size == 50
    assert (regions[0]["begin"], regions[0]["end"]) == (40, 100) and (regions[1]["begin"], regions[1]["end"], regions[1]["ref_power"]) == (0, 0, 0)
    assert (regions[2]["begin"], regions[2]["end"]) == (40, 150)
    assert (out[3:33] == plane[60:90]).all() and (out[53:83] == plane[160:190]).all() and (out[103:133] == 0).all()      # cut at out_frames; a row without input
    assert (out[160:167] == 0).all()
    assert (out[170:280] == plane[260:370]).all() and (out[280:370] == 0).all() and not np.signbit(out[280:370]).any()
    touched = np.zeros(400, bool)
    for a, b in ((3, 33), (53, 83), (103, 133), (160, 167), (170, 370)):
        touched[a:b] = True
    assert (out[~touched] == 9.0).all()
