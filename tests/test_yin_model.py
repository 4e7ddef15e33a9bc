"""tests/yin_model.py against itself and against librosa's formulas: on integer-valued periodic rows every d is an exact
integer, so the float32 chains and the chunked float64 sums must give what an order-free evaluation gives, bit for bit; on
harmonic tones the float32 model chooses the lag the float64 paper definition chooses wherever that decides with a margin,
and the pitch of a clean tone lies within 1.5 samples of its period.  No GPU."""
import numpy as np
import pytest

import yin_model as ym

RATE = 16000.0


def periodic(rng, period, n, top=8):
    """an integer-valued row of period `period`, |x| <= top"""
    return np.resize(rng.integers(-top, top + 1, period), n).astype(np.float32)


@pytest.mark.parametrize("shape", [(64, 32, 16, 2, 31), (100, 37, 33, 3, 17), (1024, 512, 160, 32, 320), (4096, 2048, 1024, 1, 2047)],
                         ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("pad_mode", [ym.PAD_REFLECT, ym.PAD_ZERO], ids=["reflect", "zero"])
def test_integer_rows_agree_with_the_order_free_truth_bit_for_bit(shape, pad_mode):
    N, W, hop, tau_min, tau_max = shape
    rng = np.random.default_rng(N + pad_mode)
    p = ym.params(RATE, N, W, hop, tau_min, tau_max, 0.1, 1, pad_mode)
    for period in (max(3, tau_min + 1), max(5, tau_max // 3), tau_max + 7):
        x = periodic(rng, period, N + 3 * hop + 5)
        F = ym.n_frames(len(x), p)
        assert F >= 3
        planes, taus, d = ym.yin32(x, p, F)
        want, wtaus, d64, _ = ym.yin64(x, p, F, round32=True)
        assert d64.max() < 2 ** 24 and (d64 == np.round(d64)).all()
        assert (d.astype(np.float64) == d64).all()
        assert (taus == wtaus).all()
        assert (planes.view(np.uint32) == want.view(np.uint32)).all()
        # a whole period inside the range and a frame that is not silent: d' is exactly 0 there, a trough under the threshold
        inside = [f for f in range(F) if tau_min <= period < tau_max and d64[f, period] == 0 and d64[f, 1:period].sum() > 0]
        for f in inside:
            assert taus[f] <= period and planes[1, f] < p.threshold
        if tau_min < period < tau_max // 2:
            assert inside


def tone(f_true, n, rng=None, noise=0.0):
    t = np.arange(n, dtype=np.float64) / RATE
    x = sum(a * np.sin(2.0 * np.pi * k * f_true * t + 0.3 * k) for k, a in ((1, 1.0), (2, 0.5), (3, 0.33), (4, 0.25)))
    if rng is not None:
        x = x + noise * rng.standard_normal(n)
    return (0.25 * x).astype(np.float32)


TONES = np.arange(60.0, 450.0, 13.7)                            # no integer period at 16 kHz among them


def test_harmonic_tones_choose_the_float64_lag_and_find_the_period(capsys):
    """f_true 60 .. 450 Hz, the fundamental and 3 partials, lightly noised (seed 7, 1e-3 of the fundamental), frames of 1024
    with W 512 and lags 32 .. 320 (50 .. 500 Hz), no centring: every frame is whole tone"""
    assert not any(abs(RATE / f - round(RATE / f)) < 1e-3 for f in TONES)
    p = ym.params(RATE, 1024, 512, 256, *ym.lags(RATE, 50.0, 500.0, 1024, 512), 0.1, 0, ym.PAD_ZERO)
    assert (p.tau_min, p.tau_max) == (32, 320)
    rng = np.random.default_rng(7)
    gamma = (p.win_length + 2) * 2.0 ** -24                      # a float32 sum of W non-negative terms
    frames = skipped = 0
    worst = 0.0
    for f_true in TONES:
        x = tone(f_true, 4096, rng, 1e-3)
        F = ym.n_frames(len(x), p)
        _, taus, _ = ym.yin32(x, p, F)
        _, taus64, _, dp64 = ym.yin64(x, p, F)
        for f in range(F):
            frames += 1
            if not ym.decided(dp64[f], taus64[f], p, 4.0 * gamma):
                skipped += 1
                continue
            assert taus[f] == taus64[f], (f_true, f, taus[f], taus64[f])
        clean = tone(f_true, 4096)
        planes, _, _ = ym.yin32(clean, p, F)
        period = RATE / f_true
        assert p.tau_min + 1 < period < p.tau_max - 1
        err = np.abs(RATE / planes[0].astype(np.float64) - period)
        assert (err < 1.5).all(), (f_true, err.max())
        assert (planes[1] < p.threshold).all()                   # voiced
        worst = max(worst, float(err.max()))
    with capsys.disabled():
        print(f"\nyin model: {frames} frames, {skipped} below the margin; largest period error on clean tones {worst:.4f} samples")
    assert skipped <= 0.02 * frames


def test_lag_helper_is_librosas():
    # librosa.yin: min_period = int(np.floor(sr / fmax)); max_period = min(int(np.ceil(sr / fmin)), frame_length - win_length - 1)
    assert ym.lags(22050, 65.40639132514966, 2093.004522404789, 2048, 1024) == (10, 338)      # C2 .. C7, the docstring's example
    assert ym.lags(16000, 50, 500, 1024, 512) == (32, 320)
    assert ym.lags(16000, 50, 500, 2048, 1024) == (32, 320)
    assert ym.lags(16000, 20, 500, 1024, 512) == (32, 511)      # capped at N - W - 1
    assert ym.lags(44100, 440, 441, 2048, 1024) == (100, 101)
    assert ym.lags(8000, 80, 400, 512, 256) == (20, 100)


def test_silent_and_constant_frames_need_no_case():
    p = ym.params(RATE, 64, 32, 16, 2, 31)
    for x in (np.zeros(200, np.float32), np.full(200, 0.37, np.float32)):
        planes, taus, _ = ym.yin32(x, ym.params(RATE, 64, 32, 16, 2, 31, center=0), 5)
        assert (taus == 2).all() and (planes[0] == np.float32(RATE / 2)).all() and (planes[1] == 1.0).all()
    x = np.zeros(200, np.float32)
    x[100] = np.nan
    planes, _, _ = ym.yin32(x, p, ym.n_frames(200, p))
    hit = ((ym.frame_index(p, planes.shape[1]) == 100).any(axis=1))
    assert hit.any() and not hit.all()
    assert (planes.view(np.uint32)[:, hit] == ym.NAN_WORD).all() and np.isfinite(planes[:, ~hit]).all()
