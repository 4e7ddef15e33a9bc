"""tests/istft_model.py, the float64 definition of the inverse STFT stage, against torch.istft in float64 on the CPU and
against the input of the forward definition (melspec_fft_model.spectrum64): both within 1e-9 of the largest |sample| -- float64
sums of at most 2048 terms agree to some 1e-13, the margin is for other BLAS orders.  And the imaginary parts the definition
ignores: a NaN there changes nothing."""
import numpy as np
import pytest
import torch

import istft_model as im
import melspec_fft_model as fm

# n_fft, win_length, hop (all centred)
SHAPES = [(400, 400, 160), (1024, 1024, 256), (2048, 2048, 512), (400, 300, 100), (75, 60, 20), (30, 30, 15), (16, 16, 4)]
IDS = [f"{a}-{b}-{c}" for a, b, c in SHAPES]
FRAMES = 7
PAD_REFLECT = 0


def torch_istft(re, imag, n_fft, win, hop, length):
    spec = torch.from_numpy(np.asarray(re, np.float64) + 1j * np.asarray(imag, np.float64))
    window = torch.from_numpy(im.window64(win))
    return torch.istft(spec, n_fft, hop_length=hop, win_length=win, window=window, center=True, length=length).numpy()


def noise_row(shape, rng):
    n_fft, win, hop = shape
    return rng.standard_normal(hop * (FRAMES - 1)).astype(np.float32)         # FRAMES frames when centred


@pytest.mark.parametrize("short", [0, 3], ids=["natural", "3-short"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_model_agrees_with_torch_istft_and_returns_the_forward_definitions_input(shape, short):
    n_fft, win, hop = shape
    rng = np.random.default_rng(n_fft + hop)
    x = noise_row(shape, rng)
    re, imag, _ = fm.spectrum64(x, n_fft, win, hop, True, PAD_REFLECT, FRAMES)
    length = hop * (FRAMES - 1) - short
    got = im.istft64(re, imag, n_fft, win, hop, True, 0, length)
    top = np.abs(x).max()
    print(f"{shape}: |model - input| {np.abs(got - x[:length]).max():.3g}, |model - torch.istft| {np.abs(got - torch_istft(re, imag, n_fft, win, hop, length)).max():.3g}")
    assert np.abs(got - x[:length].astype(np.float64)).max() <= 1e-9 * top
    assert np.abs(got - torch_istft(re, imag, n_fft, win, hop, length)).max() <= 1e-9 * top


@pytest.mark.parametrize("short", [0, 3], ids=["natural", "3-short"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_model_agrees_with_torch_istft_on_spectra_that_are_no_signals_stft(shape, short):
    n_fft, win, hop = shape
    rng = np.random.default_rng(n_fft + hop + 1)
    re, imag = rng.standard_normal((2, im.n_bins(n_fft), FRAMES))
    length = hop * (FRAMES - 1) - short
    got = im.istft64(re, imag, n_fft, win, hop, True, 0, length)
    want = torch_istft(re, imag, n_fft, win, hop, length)
    print(f"{shape}: |model - torch.istft| {np.abs(got - want).max():.3g} of {np.abs(want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(400, 400, 160), (75, 60, 20), (16, 16, 4)], ids=["400-400-160", "75-60-20", "16-16-4"])
def test_a_nan_in_an_ignored_imaginary_part_changes_nothing(shape):
    n_fft, win, hop = shape
    rng = np.random.default_rng(5)
    re, imag = rng.standard_normal((2, im.n_bins(n_fft), FRAMES))
    length = hop * (FRAMES - 1)
    lo, hi, mid = im.interval(re, imag, n_fft, win, hop, True, 0, length)
    other = imag.copy()
    other[im.real_only(n_fft)] = np.nan
    other[0, 2] = np.inf
    lo2, hi2, mid2 = im.interval(re, other, n_fft, win, hop, True, 0, length)
    assert np.array_equal(mid, mid2) and np.array_equal(lo, lo2) and np.array_equal(hi, hi2)
    assert np.isfinite(mid).all() and (hi > lo).all()
    # a NaN that is read reaches exactly the window span of its frame
    other = imag.copy()
    other[3, 2] = np.nan
    mid3 = im.istft64(re, other, n_fft, win, hop, True, 0, length)
    n_lo, pad = (n_fft - win) // 2, n_fft // 2
    t = np.arange(length) + pad
    under = (t >= 2 * hop + n_lo) & (t < 2 * hop + n_lo + win)
    assert np.isnan(mid3[under]).all() and np.array_equal(mid3[~under], mid[~under])
