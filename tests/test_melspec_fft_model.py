"""tests/melspec_fft_model.py's bound and interval admit a correct float32 transform: a float32 FFT on the CPU
(torch.fft.rfft) of the windowed frames stays inside E_f, and its power through the float32 bank inside the mel interval."""
import numpy as np
import pytest
import torch

import melspec_fft_model as fm
import melspec_model as mm

# n_fft, win_length, hop, n_mels, center
SHAPES = [(400, 400, 160, 80, True), (512, 400, 128, 23, True), (16, 16, 1, 1, True), (60, 45, 7, 5, True), (250, 250, 100, 17, True),
          (2048, 2048, 2048, 256, False)]
SAMPLERATE = 16000


def rfft32(x, n_fft, win, hop, center, pad_mode, n_frames):
    """(re, im) float32 [n_bins, n_frames] of the frames times the float32 window, by a float32 FFT"""
    fr = mm.frames_of(np.ascontiguousarray(x, np.float32), n_fft, win, hop, center, pad_mode, n_frames)
    w = fm.fft_tables32(n_fft, win)[:win]
    full = np.zeros((n_frames, n_fft), np.float32)
    n_lo = (n_fft - win) // 2
    full[:, n_lo:n_lo + win] = fr * w[None, :]
    z = torch.fft.rfft(torch.from_numpy(full), dim=1).numpy()
    assert z.dtype == np.complex64
    return np.ascontiguousarray(z.real.T), np.ascontiguousarray(z.imag.T)


@pytest.mark.parametrize("pad_mode", [mm.PAD_REFLECT, mm.PAD_ZERO], ids=["reflect", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}-{s[3]}")
def test_a_float32_fft_lies_inside_the_bound_and_the_interval(shape, pad_mode):
    n_fft, win, hop, n_mels, center = shape
    assert fm.supported(n_fft)
    rng = np.random.default_rng(n_fft + pad_mode)
    x = (rng.standard_normal(6 * n_fft + 3) * 0.5).astype(np.float32)
    nf = mm.max_frames(len(x), n_fft, hop, center)
    assert nf >= 5
    nf = min(nf, 40)
    re64, im64, E = fm.spectrum64(x, n_fft, win, hop, center, pad_mode, nf)
    re, im = rfft32(x, n_fft, win, hop, center, pad_mode, nf)
    worst = max(float((np.abs(re - re64) / E).max()), float((np.abs(im - im64) / E).max()))
    print(f"n_fft {n_fft}: float32 rfft uses {worst:.4f} of E_f ({worst * fm.bound_b(n_fft):.3f} u A_f)")
    assert worst <= 1.0
    bank = mm.filters64(SAMPLERATE, n_fft, n_mels).astype(np.float32)
    mel = bank @ (re * re + im * im)
    assert mel.dtype == np.float32
    lo, hi, mid = fm.power_interval(x, bank, n_fft, win, hop, center, pad_mode, nf)
    assert (lo <= mid).all() and (mid <= hi).all()
    assert fm.outside(mel, lo, hi).size == 0
    for floor in (0.0, 1e-3):
        a, b = fm.log_interval(lo, hi, floor)
        y = np.log10(np.fmax(mel, np.float32(floor if floor else 1e-10)).astype(np.float64)).astype(np.float32)
        assert fm.outside(y, a, b).size == 0


def test_an_indexing_error_breaks_the_bound():
    """the bound is tight enough to see a transform that is wrong: one twiddle step off, or the window one sample off"""
    n_fft, win, hop = 400, 400, 160
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(2000) * 0.5).astype(np.float32)
    re64, im64, E = fm.spectrum64(x, n_fft, win, hop, True, mm.PAD_REFLECT, 8)
    re, im = rfft32(np.roll(x, 1), n_fft, win, hop, True, mm.PAD_REFLECT, 8)
    assert (np.abs(re - re64) > E).any()


def test_the_table_and_the_sizes_the_path_takes():
    t = fm.fft_tables32(400, 400)
    assert t.dtype == np.float32 and t.size == 400 + 800 and t[0] == 0.0 and t[400] == 1.0 and t[401] == 0.0
    assert t[200] == 1.0 and t[400 + 2 * 100] == np.float32(np.cos(np.pi / 2)) and t[400 + 2 * 100 + 1] == -1.0
    assert [n for n in (16, 17, 60, 75, 77, 250, 400, 480, 512, 800, 960, 1024, 2047, 2048, 2049, 15) if fm.supported(n)] == \
        [16, 60, 75, 250, 400, 480, 512, 800, 960, 1024, 2048]
    assert fm.bound_b(400) == 80 and fm.bound_b(16) == 40 and fm.bound_b(2048) == 96
