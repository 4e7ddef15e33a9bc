"""Pins tests/mp3_model.py -- the float64 model of the MP3 transform stage, its input set and its error scale -- on the CPU,
and proves that the bound the device tests use (tests/test_mp3_fullband_gpu.py) can fail.

    R       = max over every block of the input set of |oracle32 - model64| / scale: the float32 reference's own rounding
    bound   = |got - model64| <= 4 * R * scale for every sample, R recomputed here from the oracle, never from a device

Every mutant of mp3_model.MUTANTS, rounded to float32, has to leave that bound in at least one block.  Measured values (printed
by the tests, run with -s): R = 23.8 (flat 1.84, onehot 23.8, flags 1.26, nzbands 2.81); the smallest relative perturbation of
one band (band 29 of the one-hot streams) that is still caught is 2^-16."""
import numpy as np
import pytest

import mp3_model
import oraclelib


@pytest.fixture(scope="module")
def measured():
    return mp3_model.measure(mp3_model.fullband_cases(), oraclelib.mp3_transform)


def test_model_against_oracle(measured):
    refs, R = measured
    for ref in refs:
        dead = ref.scale == 0
        assert (ref.oracle32[dead] == 0).all() and (ref.model64[dead] == 0).all(), f"{ref.case.name}: output without input"
        assert np.isfinite(ref.ratio).all(), ref.case.name
        print(f"{ref.case.name}: {ref.ratio.size} blocks, {int(dead.sum()) // 576} silent, "
              f"largest |oracle32 - model64| / scale = {ref.ratio.max():.4g}")
    print(f"R = {R:.4g}")
    assert np.isfinite(R) and R > 0


def test_float32_rounding_of_the_model_is_inside_the_bound(measured):
    """The control of the mutant test: the unmutated model, rounded to float32, passes."""
    refs, R = measured
    for ref in refs:
        assert ratio(ref, ref.model64.astype(np.float32), R).max() <= 1.0, ref.case.name


def ratio(ref, got, R):
    return mp3_model.ratio_per_block(got, ref, 4 * R)


@pytest.mark.parametrize("name", sorted(mp3_model.MUTANTS))
def test_bound_catches_mutant(measured, name):
    refs, R = measured
    worst, where = 0.0, None
    for ref in refs:
        c = ref.case
        got = mp3_model.transform64(c.granules, c.channels, c.coef, c.flags, **{name: mp3_model.MUTANTS[name]}).astype(np.float32)
        r = ratio(ref, got, R)
        if r.max() > worst:
            worst, where = float(r.max()), (c.name, int(r.argmax()))
        print(f"{name}: {c.name}: {int((r > 1).sum())} of {r.size} blocks outside 4 * R * scale, worst {r.max():.4g}")
    assert worst > 1.0, f"mutant {name} survives: worst block {where} at {worst:.3g} of the bound"


def test_smallest_band_perturbation_caught(measured):
    """Band 29 scaled by 1 + eps: by linearity the mutant is model + eps * (response to band 29 alone)."""
    refs, R = measured
    ref = next(r for r in refs if r.case.name == "onehot")
    c = ref.case
    resp = mp3_model.transform64(c.granules, c.channels, c.coef, c.flags, band_gain=(29, 2.0)) - ref.model64
    caught = [k for k in range(8, 26) if ratio(ref, (ref.model64 + 2.0 ** -k * resp).astype(np.float32), R).max() > 1.0]
    assert caught == list(range(8, max(caught) + 1))
    print(f"smallest relative perturbation of band 29 caught: 2^-{max(caught)}")
    assert max(caught) >= 14, "the issue expects it well below 2^-10"


def test_input_properties(measured):
    refs, _ = measured
    by_name = {r.case.name: r for r in refs}
    assert sorted(by_name) == ["flags", "flat", "nzbands", "onehot"]
    for name in ("flat", "onehot", "flags"):
        energy = (by_name[name].case.coef.reshape(-1, 32, 18).astype(np.float64) ** 2).sum((0, 2))
        assert (energy > 0).all(), f"{name}: subbands {np.flatnonzero(energy == 0)} carry nothing"
    # one-hot: exactly one band per block
    hot = (by_name["onehot"].case.coef.reshape(-1, 32, 18) != 0).any(2)
    assert (hot.sum(1) == 1).all() and set(np.argmax(hot, 1)) == set(range(32))
    # flat: the stream lengths, mono and stereo, a mono stream last
    c = by_name["flat"].case
    assert sorted(zip(c.channels, c.granules)) == sorted((nc, ng) for nc in (1, 2) for ng in (1, 2, 3, 5, 66, 131))
    assert c.channels[-1] == 1
    # flags: every listed (block type, n_long, aa) occurs, and subband streams
    f = by_name["flags"].case.flags
    seen = {(int(w & 3), int((w >> 8) & 0xff), int((w >> 16) & 0xff) - 1) for w in f if not w >> 31}
    assert set(mp3_model.FLAG_COMBOS) <= seen, set(mp3_model.FLAG_COMBOS) - seen
    assert (f >> 31).any()
    # nzbands: the counts, the zeros above them, the declaration
    c = by_name["nzbands"].case
    counts = ((c.declared >> 24) & 63).astype(int) - 1
    assert {0, 1, 17, 31, 32} <= set(counts) and len(set(counts)) > 20 and ((c.flags >> 24) & 63 == 0).all()
    lines = c.coef.reshape(-1, 32, 18)
    for blk, n in enumerate(counts):
        assert not lines[blk, n:].any() and not np.signbit(lines[blk, n:]).any()
        assert n == 0 or lines[blk, n - 1].any()
    # level
    for name in ("flat", "flags"):
        rms = float(np.sqrt(np.mean(by_name[name].oracle32.astype(np.float64) ** 2)))
        print(f"{name}: PCM rms {rms:.4g} at level {mp3_model.FLAT_LEVEL}")
        assert 0.03 <= rms <= 0.1


def test_block_scale_definition():
    granules, channels = [3, 2], [2, 1]
    coef = np.arange(8 * 576, dtype=np.float32).reshape(8, 576) % 7 - 3
    L = np.abs(coef.astype(np.float64)).sum(1)
    want = np.array([L[0], L[1], L[0] + L[2], L[1] + L[3], L[0] + L[2] + L[4], L[1] + L[3] + L[5], L[6], L[6] + L[7]]) * 2.0 ** -24
    assert (mp3_model.block_scale(coef.reshape(-1), granules, channels) == want).all()
    s = mp3_model.per_sample(want, granules, channels)
    assert (s[:1152].reshape(576, 2) == want[:2]).all() and (s[6 * 576:7 * 576] == want[6]).all()
    assert (mp3_model.per_block(s, granules, channels) == want).all()
