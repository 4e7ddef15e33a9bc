"""tests/mix_model.py against independent statements of the same things: its energies against math.fsum within the bound of
recursive summation, its gain against a float64 restatement of torchaudio.functional.add_noise's lines, the SNR its float32
gain achieves against a bound derived here from that rounding, and its wrap indexing against numpy's own."""
import math

import numpy as np
import pytest

import afgpu
import mix_model as mm

F32, F64 = np.float32, np.float64
SNRS = (-5.0, 0.0, 20.0)


@pytest.fixture(scope="module")
def group():
    """three rows of 2 * 4096 + 5 samples of mixed magnitude and the looping noise under them"""
    rng = np.random.default_rng(811)
    valid = 2 * 4096 + 5
    x = (rng.standard_normal((3, valid)) * 10.0 ** rng.integers(-3, 2, (3, valid))).astype(F32)
    clip = (0.1 * rng.standard_normal(5000)).astype(F32)
    z = np.stack([mm.noise_under(clip, 4321, valid)] * 3)
    return x, z


def exact_energy(a):
    return math.fsum(float(v) * float(v) for v in np.asarray(a, F32).ravel())      # (a float32 squared is exact in float64)


def test_energies_lie_within_the_recursive_summation_bound(group):
    u = 2.0 ** -53
    for a in group:
        n = a.size
        got, want = float(mm.energy(a)), exact_energy(a)
        bound = (n - 1) * u / (1 - (n - 1) * u) * want           # any order of n - 1 rounded additions of positive terms
        print(f"energy {got!r}: off by {abs(got - want):.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound
    assert mm.energy(np.zeros((2, 5), F32)) == 0 and np.isnan(mm.energy(np.array([[1.0, np.nan]], F32)))
    assert mm.energy(np.array([[np.inf, 1.0]], F32)) == np.inf


@pytest.mark.parametrize("snr", SNRS)
def test_the_gain_is_torchaudios(group, snr):
    """torchaudio.functional.add_noise: original_snr_db = 10 (log10 Es - log10 En); scale = 10 ** ((original_snr_db - snr) / 20)"""
    x, z = group
    es, en = mm.energy(x), mm.energy(z)
    mine = float(mm.gain64(es, en, mm.ratio(snr)))
    snr0 = 10.0 * (math.log10(float(es)) - math.log10(float(en)))
    theirs = 10.0 ** ((snr0 - snr) / 20.0)
    print(f"snr {snr}: gain {mine!r}, torchaudio's lines {theirs!r}, relative {abs(mine - theirs) / theirs:.3e}")
    assert abs(mine - theirs) <= 1e-9 * theirs


@pytest.mark.parametrize("snr", SNRS)
def test_the_achieved_snr_is_within_the_float32_roundings_reach(group, snr):
    """The record's gain g is the float64 gain G rounded once to float32: |g - G| <= 2^-24 G (G is far inside float32's
    normal range here).  G itself is three rounded float64 operations -- a division and a product under a square root, which
    halves their relative errors, and the root: at most 2^-53 + 2^-53 -- and the ratio is pow's value, taken as within 2 ulp
    (2^-52 relative, halved by the root).  So g = G0 (1 + d) with G0 the real-number gain of the model's energies and
    |d| <= D = 2^-24 + 2^-50, and the SNR achieved over those energies, 10 log10(Es / (g^2 En)), differs from snr by
    20 log10(1 + d): at most 20 log10(1 + D) dB, plus 1e-12 for this test's own float64 logarithms."""
    x, z = group
    es, en = mm.energy(x), mm.energy(z)
    st = mm.group_stats(x, z, mm.SNR, mm.ratio(snr))
    D = 2.0 ** -24 + 2.0 ** -50
    bound = 20.0 * math.log10(1.0 + D) + 1e-12
    g = float(st["gain"])
    achieved = 10.0 * math.log10(float(es) / (g * g * float(en)))
    print(f"snr {snr}: achieved {achieved!r}, off by {abs(achieved - snr):.3e} dB, bound {bound:.3e} dB")
    assert st["flags"] == 0 and g > 0
    assert abs(achieved - snr) <= bound
    assert st["gain"].dtype == F32 and st["gain"] == F32(mm.gain64(es, en, mm.ratio(snr)))


def test_wrap_indexing_is_numpys():
    rng = np.random.default_rng(5)
    for N in (1, 2, 3, 5, 63, 64, 4095, 4096, 4097, 10000):
        clip = rng.standard_normal(N).astype(F32)
        for start in (0, 1 % N, N // 2, N - 1):
            for count in (0, 1, 3, 4097, 2 * 4096 + 5):
                got = mm.noise_under(clip, start, count)
                want = np.take(clip, start + np.arange(count), mode="wrap")
                assert got.dtype == F32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (N, start, count)
    assert mm.noise_index(2 ** 32 - 2, 4, 2 ** 32 - 1).tolist() == [2 ** 32 - 2, 0, 1, 2]     # no 32-bit sum in the way


def test_degenerate_groups_and_the_apply():
    x = np.array([[1.0, -2.0, 0.5]], F32)
    z = np.array([[0.25, 0.5, -1.0]], F32)
    r = mm.ratio(0.0)
    assert r == 1.0
    for xs, zs, why in ((x * 0, z, mm.SILENT_SIGNAL), (x, z * 0, mm.SILENT_NOISE), (x * 0, z * 0, mm.SILENT_SIGNAL | mm.SILENT_NOISE),
                        (np.array([[np.nan, 1, 1]], F32), z, mm.ENERGY_NOT_FINITE), (x, np.array([[np.inf, 1, 1]], F32), mm.ENERGY_NOT_FINITE),
                        (x * 0, np.array([[np.nan, 1, 1]], F32), mm.SILENT_SIGNAL | mm.ENERGY_NOT_FINITE)):
        st = mm.group_stats(xs, zs, mm.SNR, r)
        assert st["flags"] == why and st["gain"] == 0, why
        assert (mm.apply(xs, zs, st["gain"]).view(np.uint32) == xs.view(np.uint32)).all()
    big, small = np.full((1, 3), 1e30, F32), np.full((1, 3), 1e-30, F32)
    st = mm.group_stats(big, small, mm.SNR, r)                   # a gain past float32's range
    assert st["flags"] == mm.GAIN_NOT_FINITE and st["gain"] == 0 and np.isfinite(st["signal_energy"]) and np.isfinite(st["noise_energy"])
    st = mm.group_stats(x, z, mm.GAIN, gain=0.5)                 # the gain as given, the energies still measured
    assert st["gain"] == 0.5 and st["flags"] == 0 and st["signal_energy"] == 5.25 and st["noise_energy"] == 1.3125
    assert mm.apply(x, z, 0.5).tolist() == [[1.125, -1.75, 0.0]]
    # the product is rounded before the sum: a fused multiply-add gives other bits
    a, b, g = F32(-1.0), F32(1.0 + 2.0 ** -12), F32(1.0 + 2.0 ** -12)      # g b = 1 + 2^-11 + 2^-24: the last term is lost to the rounding
    fused = F32(F64(a) + F64(g) * F64(b))
    assert mm.apply(np.array([a]), np.array([b]), g)[0] == F32(a + F32(g * b)) != fused
    assert mm.apply(np.array([np.inf], F32), np.array([-np.inf], F32), 1.0).view(np.uint32)[0] == 0x7fc00000
    assert mm.group_stats(np.zeros((2, 0), F32), np.zeros((2, 0), F32), mm.SNR, r).tobytes() == bytes(24)


def test_the_ratio_is_the_librarys():
    for snr in (-40.0, -5.0, 0.0, 3.0, 20.0, 100.0):
        mine, theirs = float(mm.ratio(snr)), afgpu.mix_ratio(snr)
        assert abs(mine - theirs) <= 4 * np.spacing(theirs), snr
    assert afgpu.mix_ratio(0.0) == 1.0 and afgpu.mix_ratio(10.0) == 0.1 and afgpu.mix_ratio(-20.0) == 100.0
