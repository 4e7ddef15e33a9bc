"""tests/convolve_model.py against numpy and scipy in float64, its ranges against numpy's modes, its fused multiply-add against
exact rational arithmetic, and its bound constant against afg_convolve_bound."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal

import afgpu
import convolve_model as cm

TAPS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2048, 2049, 5000]
FRAMES = [1, 2, 1023, 1024, 1025, 2049, 3 * 1024 + 7]


def case(taps, frames):
    rng = np.random.default_rng(taps * 7919 + frames)
    h = (rng.standard_normal(taps) * np.exp(-np.arange(taps) / (0.3 * taps + 1))).astype(np.float32)
    return rng.standard_normal(frames).astype(np.float32), h


@pytest.mark.parametrize("taps", TAPS)
def test_the_model_against_numpy_and_scipy(taps):
    for frames in FRAMES:
        x, h = case(taps, frames)
        y = cm.line64(x, h)
        x64, h64 = x.astype(np.float64), h.astype(np.float64)
        scale = np.convolve(np.abs(x64), np.abs(h64))
        assert y.shape == scale.shape
        assert (np.abs(y - np.convolve(x64, h64)) <= 1e-12 * scale).all()
        assert (np.abs(y - scipy.signal.fftconvolve(x64, h64)) <= 1e-12 * scale.max()).all()


def test_full_and_same_are_numpys_modes():
    for taps, frames in ((1, 1), (2, 5), (3, 5), (4, 4), (64, 100), (65, 100), (129, 300), (1025, 1100)):      # numpy's "same" is centred on the longer side: frames >= taps
        x, h = case(taps, frames)
        x64, h64, y = x.astype(np.float64), h.astype(np.float64), cm.line64(x, h)
        for mode in ("full", "same"):
            first, count = cm.mode_range(mode, frames, taps)
            want = np.convolve(x64, h64, mode)
            assert count == len(want)
            assert np.allclose(y[first:first + count], want, rtol=0, atol=1e-12 * np.abs(want).max())
    assert cm.mode_range("head", 10, 5, 4) == (4, 10)


def test_the_fused_multiply_add_is_correctly_rounded():
    rng = np.random.default_rng(5)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, n) * 2.0 ** -rng.integers(20, 50, n))).astype(np.float32)   # near cancellation and ties
    c[::7] = (rng.standard_normal(len(c[::7])) * 2.0 ** rng.integers(-30, 30, len(c[::7]))).astype(np.float32)
    got = cm.fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                            # (float(Fraction) rounds once, to 53 bits: a candidate only)
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)
    z = cm.fma32(np.array([-1.0, 1.0, -1.0], np.float32), np.array([0.0, -0.0, 0.0], np.float32), np.array([0.0, 0.0, -0.0], np.float32))
    assert list(np.signbit(z)) == [False, False, True]


def test_the_direct_restatement_is_the_definition_up_to_rounding():
    for taps, frames in ((1, 5), (3, 2), (64, 200), (128, 300)):
        x, h = case(taps, frames)
        first, count = cm.mode_range("full", frames, taps)
        got = cm.direct32(x, h, first, count).astype(np.float64)
        scale = np.convolve(np.abs(x.astype(np.float64)), np.abs(h.astype(np.float64)))
        assert (np.abs(got - cm.line64(x, h)) <= taps * cm.U * scale).all()
    assert not np.signbit(cm.direct32(np.zeros(4, np.float32), -np.ones(3, np.float32), 0, 6)).any()


def test_the_bound_constant():
    prm = afgpu.convolve_params()
    for taps in (1, 128, 129, 1024, 1025, 2048, 2049, 5000, 65535, 65536):
        assert afgpu.convolve_bound(prm, taps) == cm.bound_c(taps) == 6 * 96 + 2 * -(-taps // 1024) + 11
    assert cm.bound_c(1) == 589 and cm.bound_c(65536) == 715
    for taps in (0, 65537):
        with pytest.raises(afgpu.AfgError, match="taps"):
            afgpu.convolve_bound(prm, taps)
    with pytest.raises(afgpu.AfgError, match="direct_max"):
        afgpu.convolve_bound(afgpu.convolve_params(129), 5)


def test_s_and_the_interval():
    x = np.zeros(1500, np.float32)
    x[[0, 1023, 1024, 1499]] = [1, -1, 1, -1]
    h = np.zeros(2048, np.float32)
    h[[0, 1023, 1024, 2047]] = [1, -1, -1, 1]
    S = cm.s_blocks(x, h)
    # A_x = 2, 4, 2, 0 ...; A_h = 2, 2
    assert list(S) == [4.0, 12.0, 12.0, 4.0]
    lo, hi, mid = cm.interval(x, h, 1000, 100)
    assert np.allclose(hi - mid, cm.bound_c(2048) * cm.U * np.where(np.arange(1000, 1100) < 1024, 4.0, 12.0))
    assert mid[23] == x[1023] * h[0] + x[0] * h[1023]
