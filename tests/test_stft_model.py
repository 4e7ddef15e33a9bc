"""tests/stft_model.py's intervals are sound: the float64 value lies inside its own interval for every kind and shape the
device tests use, the intervals are not degenerate on noise, numpy's rfft of the windowed frames is the spectrum64 the
intervals are built on, and a correct float32 transform (torch.fft.rfft on the CPU) lies inside all four."""
import numpy as np
import pytest
import torch

import melspec_fft_model as fm
import melspec_model as mm
import stft_model as sm

# n_fft, win_length, hop, center: test_stft_gpu.py's
SHAPES = [(400, 400, 160, True), (512, 400, 128, True), (16, 16, 1, True), (60, 45, 7, True), (250, 250, 100, True), (75, 75, 25, True),
          (2048, 2048, 2048, False), (1875, 1500, 625, True), (2025, 2025, 2025, False)]
KINDS = [(sm.COMPLEX, 0.0), (sm.MAGNITUDE, 0.0), (sm.POWER, 0.0), (sm.LOG10, 0.0), (sm.LOG10, 1e-3)]
KIND_IDS = ["complex", "magnitude", "power", "log10-0", "log10-1e-3"]


def windowed(x, n_fft, win, hop, center, pad_mode, n_frames, dtype):
    """[n_frames, n_fft]: the frames times the window, zero outside it"""
    fr = mm.frames_of(np.ascontiguousarray(x, np.float32).astype(dtype), n_fft, win, hop, center, pad_mode, n_frames)
    w = fm.fft_tables64(n_fft, win)[0] if dtype == np.float64 else fm.fft_tables32(n_fft, win)[:win]
    full = np.zeros((n_frames, n_fft), dtype)
    n_lo = (n_fft - win) // 2
    full[:, n_lo:n_lo + win] = fr * w[None, :]
    return full


def noise(shape, pad_mode):
    n_fft, win, hop, center = shape
    rng = np.random.default_rng(n_fft + pad_mode)
    x = (rng.standard_normal(6 * n_fft + 3) * 0.5).astype(np.float32)
    return x, min(mm.max_frames(len(x), n_fft, hop, center), 40)


@pytest.mark.parametrize("pad_mode", [mm.PAD_REFLECT, mm.PAD_ZERO], ids=["reflect", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_the_float64_value_lies_inside_an_interval_that_is_not_degenerate(shape, pad_mode):
    n_fft, win, hop, center = shape
    x, nf = noise(shape, pad_mode)
    assert nf >= 5
    for kind, floor in KINDS:
        lo, hi, mid = sm.interval(kind, x, n_fft, win, hop, center, pad_mode, nf, floor)
        assert lo.shape == hi.shape == mid.shape == (n_fft // 2 + 1, nf) + ((2,) if kind == sm.COMPLEX else ())
        assert np.isfinite(lo).all() and np.isfinite(hi).all()
        assert (lo <= mid).all() and (mid <= hi).all()
        assert (hi > lo).all()                                                       # noise: E_f > 0 in every frame


@pytest.mark.parametrize("pad_mode", [mm.PAD_REFLECT, mm.PAD_ZERO], ids=["reflect", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_rfft_of_the_windowed_frames_is_spectrum64_and_a_float32_fft_lies_inside(shape, pad_mode):
    n_fft, win, hop, center = shape
    x, nf = noise(shape, pad_mode)
    re64, im64, E = fm.spectrum64(x, n_fft, win, hop, center, pad_mode, nf)
    z = np.fft.rfft(windowed(x, n_fft, win, hop, center, pad_mode, nf, np.float64), axis=1).T
    # two float64 evaluations of the same sums: far inside E_f (B u A_f against about 2^-53 n_fft A_f)
    assert (np.abs(z.real - re64) <= 1e-6 * E).all() and (np.abs(z.imag - im64) <= 1e-6 * E).all()
    z32 = torch.fft.rfft(torch.from_numpy(windowed(x, n_fft, win, hop, center, pad_mode, nf, np.float32)), dim=1).numpy().T
    assert z32.dtype == np.complex64
    re, im = np.ascontiguousarray(z32.real), np.ascontiguousarray(z32.imag)
    p = re * re + im * im
    assert p.dtype == np.float32
    for kind, floor in KINDS:
        lo, hi, mid = sm.interval(kind, x, n_fft, win, hop, center, pad_mode, nf, floor)
        if kind == sm.COMPLEX:
            y = np.stack([re, im], axis=-1)
        elif kind == sm.MAGNITUDE:
            y = np.sqrt(p)
        elif kind == sm.POWER:
            y = p
        else:
            y = np.log10(np.fmax(p, np.float32(floor if floor else 1e-10)).astype(np.float64)).astype(np.float32)
        assert sm.outside(y, lo, hi).size == 0, sm.KIND_NAMES[kind]


def test_a_wrong_transform_leaves_every_interval():
    """the intervals are tight enough to see a frame one sample off"""
    n_fft, win, hop = 400, 400, 160
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(2000) * 0.5).astype(np.float32)
    z = torch.fft.rfft(torch.from_numpy(windowed(np.roll(x, 1), n_fft, win, hop, True, mm.PAD_REFLECT, 8, np.float32)), dim=1).numpy().T
    re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    p = re * re + im * im
    for kind, y in ((sm.COMPLEX, np.stack([re, im], axis=-1)), (sm.MAGNITUDE, np.sqrt(p)), (sm.POWER, p), (sm.LOG10, np.log10(p))):
        lo, hi, _ = sm.interval(kind, x, n_fft, win, hop, True, mm.PAD_REFLECT, 8)
        assert sm.outside(y, lo, hi).size > 0


def test_silence_and_nan():
    x = np.zeros(1000, np.float32)
    for kind, floor in KINDS:
        lo, hi, mid = sm.interval(kind, x, 400, 400, 160, True, mm.PAD_ZERO, 5, floor)
        if kind == sm.LOG10:
            assert (lo < sm.floor_value(floor)).all() and (hi > sm.floor_value(floor)).all() and (mid == sm.floor_value(floor)).all()
        else:
            assert (mid == 0).all() and (lo <= 0).all() and (hi >= 0).all() and (hi - lo <= 1e-44).all()
    x = np.ones(1000, np.float32)
    x[500] = np.nan
    hit = np.isnan(mm.frames_of(x, 400, 400, 160, True, mm.PAD_ZERO, 7)).any(axis=1)
    assert 0 < hit.sum() < 7
    for kind in (sm.COMPLEX, sm.MAGNITUDE, sm.POWER):
        lo, hi, _ = sm.interval(kind, x, 400, 400, 160, True, mm.PAD_ZERO, 7)
        assert np.isnan(lo[:, hit]).all() and np.isfinite(lo[:, ~hit]).all() and np.isfinite(hi[:, ~hit]).all()
    assert sm.comps(sm.COMPLEX) == 2 and [sm.comps(k) for k in (sm.MAGNITUDE, sm.POWER, sm.LOG10)] == [1, 1, 1]
