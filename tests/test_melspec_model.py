"""tests/melspec_model.py against itself and against torch.stft: the exact float32 fmaf, the float32 chains within the derived
chain bound of the float64 definition, the float64 power spectrum against torch.stft in float64, and the filter bank's
properties.  No GPU."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import torch

import melspec_model as mm

# (a, b, c) as float32 words on which float32(a * b + c) through float64 rounds twice and lands one ulp off: found by a
# search over a in [1, 2), b next to 2^-24 / a, c = 1 -- the exact sum lies just above the float32 tie 1 + 2^-24, float64
# rounds it onto the tie, and the tie then goes to even
DOUBLE_ROUNDED = [(0x3f872155, 0x33727df7, 0x3f800000, 0x3f800001), (0x3ff2bc63, 0x3306fe95, 0x3f800000, 0x3f800001),
                  (0x3f9a7e1c, 0x335419cb, 0x3f800000, 0x3f800001), (0x3fb19ab0, 0x33388006, 0x3f800000, 0x3f800001),
                  (0x3fba067d, 0x333025e6, 0x3f800000, 0x3f800001), (0x3f945e8a, 0x335cdab5, 0x3f800000, 0x3f800001)]


def f32(words):
    return np.array(words, np.uint32).view(np.float32)


def libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    return libm.fmaf


def test_fmaf32_is_libms_fmaf():
    fmaf = libm_fmaf()
    rng = np.random.default_rng(3)
    n = 20000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = rng.standard_normal(n).astype(np.float32)
    # cancelling triples: c next to -a * b
    c[::2] = (-(a[::2].astype(np.float64) * b[::2]).astype(np.float32) * (1 + rng.integers(-3, 4, n // 2) * 2.0 ** -23)).astype(np.float32)
    # tiny and huge scales: subnormal results, overflow
    s = (2.0 ** rng.integers(-140, 64, n)).astype(np.float32)
    a[1::4] *= s[1::4]
    c[1::4] *= s[1::4]
    a[7::1000], b[7::1000] = 3e38, 4.0
    got = mm.fmaf32(a, b, c)
    want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert mm.same_bits(got, want).size == 0
    assert ((np.abs(got) < 1.1e-38) & (got != 0)).any() and np.isinf(got).any()              # subnormal results and overflow were among them


def test_the_plain_float64_detour_rounds_twice():
    fmaf = libm_fmaf()
    for wa, wb, wc, wr in DOUBLE_ROUNDED:
        a, b, c = f32([wa]), f32([wb]), f32([wc])
        assert mm.fmaf32(a, b, c).view(np.uint32)[0] == wr
        assert np.float32(fmaf(float(a[0]), float(b[0]), float(c[0]))).view(np.uint32) == wr
        assert mm.naive_fma32(a, b, c).view(np.uint32)[0] != wr


SHAPES = [(400, 400, 160, True, mm.PAD_REFLECT), (512, 400, 128, True, mm.PAD_ZERO), (16, 16, 1, True, mm.PAD_REFLECT),
          (256, 255, 100, False, mm.PAD_REFLECT), (64, 1, 64, False, mm.PAD_ZERO)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_float32_chains_stay_within_the_chain_bound(shape):
    """|re - re64| <= (K + 2) 2^-24 sum |x_n C[n][k]| with K = win_length: K fmaf roundings of relative size 2^-24 each on
    partial sums no larger than sum |x C|, one more for the basis entry's own rounding to float32 (the float64 side keeps
    the float64 basis), and one of slack for the second-order terms (K^2 2^-48) and the float64 side's own error."""
    n_fft, win, hop, center, mode = shape
    rng = np.random.default_rng(n_fft + hop)
    x = (rng.standard_normal(3 * n_fft + 37) * 0.3).astype(np.float32)
    C64, S64 = mm.basis64(n_fft, win)
    Cf, Sf = C64.astype(np.float32), S64.astype(np.float32)
    nf = mm.max_frames(len(x), n_fft, hop, center)
    assert nf >= 2
    fr = mm.frames_of(x, n_fft, win, hop, center, mode, nf)
    re32, im32 = mm.chain32(fr, Cf).T.astype(np.float64), mm.chain32(fr, Sf).T.astype(np.float64)
    re64, im64, _, ac, as_ = mm.power64(x, C64, S64, n_fft, win, hop, center, mode, nf)
    bound = (win + 2) * 2.0 ** -24
    assert (np.abs(re32 - re64) <= bound * ac + 1e-45).all()
    assert (np.abs(im32 - im64) <= bound * as_ + 1e-45).all()
    if win > 1:
        assert np.abs(re64).max() > 0.1


@pytest.mark.parametrize("n_fft,hop", [(400, 160), (512, 128), (16, 1), (1024, 256)])
def test_float64_power_spectrum_is_torch_stft(n_fft, hop):
    rng = np.random.default_rng(n_fft)
    x = rng.standard_normal(4 * n_fft + 11)
    C64, S64 = mm.basis64(n_fft, n_fft)
    nf = mm.max_frames(len(x), n_fft, hop, True)
    _, _, p, _, _ = mm.power64(x, C64, S64, n_fft, n_fft, hop, True, mm.PAD_REFLECT, nf)
    st = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                    center=True, pad_mode="reflect", return_complex=True)
    want = (st.real ** 2 + st.imag ** 2).numpy()
    assert want.shape == p.shape == (n_fft // 2 + 1, nf)
    assert np.abs(p - want).max() <= 1e-12 * np.abs(want).max()


def test_a_short_window_is_centred_like_torchs():
    n_fft, win, hop = 512, 400, 128
    x = np.random.default_rng(5).standard_normal(3000)
    C64, S64 = mm.basis64(n_fft, win)
    nf = mm.max_frames(len(x), n_fft, hop, True)
    _, _, p, _, _ = mm.power64(x, C64, S64, n_fft, win, hop, True, mm.PAD_REFLECT, nf)
    st = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                    center=True, pad_mode="reflect", return_complex=True)
    want = (st.real ** 2 + st.imag ** 2).numpy()
    assert np.abs(p - want).max() <= 1e-12 * np.abs(want).max()


def test_filter_bank_properties():
    for sr, n_fft, n_mels, scale in ((16000, 400, 80, mm.SCALE_SLANEY), (16000, 400, 80, mm.SCALE_HTK), (22050, 1024, 128, mm.SCALE_SLANEY),
                                     (8000, 512, 23, mm.SCALE_HTK)):
        w = mm.filters64(sr, n_fft, n_mels, scale=scale, norm=mm.NORM_SLANEY)
        assert w.shape == (n_mels, n_fft // 2 + 1) and (w >= 0).all()
        # a Slaney-normalised triangle has area 1 over Hz; the bins sample it every df = sr / n_fft, and the rectangle rule on
        # a triangle of base B and height 2 / B errs by at most the height times df at each of its three corners
        df = sr / n_fft
        f = mm.mel_points(sr, n_mels, scale=scale)
        area = w.sum(1) * df
        assert (np.abs(area - 1.0) <= 3 * df * 2.0 / (f[2:] - f[:-2])).all()
        plain = mm.filters64(sr, n_fft, n_mels, scale=scale, norm=mm.NORM_NONE)
        assert plain.max() <= 1.0 and np.allclose(plain * (2.0 / (f[2:] - f[:-2]))[:, None], w, rtol=1e-15, atol=0)
    # the closed forms
    assert float(mm.hz_to_mel(0.0, mm.SCALE_SLANEY)) == 0.0 and float(mm.hz_to_mel(1000.0, mm.SCALE_SLANEY)) == 15.0
    assert abs(float(mm.hz_to_mel(8000.0, mm.SCALE_SLANEY)) - (15.0 + 27.0 * np.log(8.0) / np.log(6.4))) < 1e-13
    assert float(mm.hz_to_mel(0.0, mm.SCALE_HTK)) == 0.0
    assert abs(float(mm.hz_to_mel(1000.0, mm.SCALE_HTK)) - 2595.0 * np.log10(1.0 + 1000.0 / 700.0)) < 1e-12
    assert abs(float(mm.hz_to_mel(8000.0, mm.SCALE_HTK)) - 2595.0 * np.log10(1.0 + 8000.0 / 700.0)) < 1e-12
    for scale in (mm.SCALE_SLANEY, mm.SCALE_HTK):
        for hz in (0.0, 1000.0, 8000.0):
            assert abs(float(mm.mel_to_hz(mm.hz_to_mel(hz, scale), scale)) - hz) <= 1e-9
    # Whisper's bank: no empty row
    w = mm.filters64(16000, 400, 80)
    assert w.shape == (80, 201) and (w.max(1) > 0).all() and (w.astype(np.float32).max(1) > 0).all()
