"""tests/fbank_model.py -- the float64 definition of the Kaldi-compatible filter-bank stage (include/afg.h: afg_fbank_hip) --
against a float64 restatement of torchaudio.compliance.kaldi.fbank's own steps written here (and against torchaudio itself
where it is installed), and its pieces against brute force: frame counts, the mirror, the windows, the bank.  No GPU."""
import math

import numpy as np
import pytest
import torch

import afgpu
import fbank_model as fm

WINDOW_NAMES = {fm.POVEY: "povey", fm.HAMMING: "hamming", fm.HANNING: "hanning", fm.BLACKMAN: "blackman", fm.RECTANGULAR: "rectangular"}


def kaldi_strided(x, ws, hop, snip_edges):
    """torchaudio's _get_strided: the flipped-copy construction"""
    N = x.numel()
    if snip_edges:
        if N < ws:
            return torch.empty((0, ws), dtype=x.dtype)
        m = 1 + (N - ws) // hop
    else:
        rev = torch.flip(x, [0])
        m = (N + hop // 2) // hop
        pad = ws // 2 - hop // 2
        if pad > 0:
            x = torch.cat((rev[-pad:], x, rev), dim=0)
        else:
            x = torch.cat((x[-pad:], rev), dim=0)
    return x.as_strided((m, ws), (hop, 1))


def kaldi_fbank(x, samplerate, prm, window_type, low_freq, high_freq, blackman_coeff=0.42):
    """torchaudio.compliance.kaldi.fbank's steps in float64 (no dither, no VTLN, no subtract_mean), on an already scaled row"""
    eps = torch.tensor(torch.finfo(torch.float32).eps, dtype=torch.float64)
    ws, hop, n_fft = prm.win_length, prm.hop, prm.n_fft
    fr = kaldi_strided(x, ws, hop, prm.snip_edges).clone()
    if prm.remove_dc:
        fr = fr - fr.mean(dim=1, keepdim=True)

    def log_energy(t):
        e = torch.max(t.pow(2).sum(1), eps).log()
        return e if prm.energy_floor == 0.0 else torch.max(e, torch.tensor(math.log(prm.energy_floor), dtype=torch.float64))

    if prm.raw_energy:
        energy = log_energy(fr)
    if prm.preemph != 0.0:
        off = torch.nn.functional.pad(fr.unsqueeze(0), (1, 0), mode="replicate").squeeze(0)
        fr = fr - prm.preemph * off[:, :-1]
    a = 2.0 * math.pi * torch.arange(ws, dtype=torch.float64) / (ws - 1)
    win = {fm.POVEY: torch.hann_window(ws, periodic=False, dtype=torch.float64).pow(0.85),
           fm.HAMMING: torch.hamming_window(ws, periodic=False, alpha=0.54, beta=0.46, dtype=torch.float64),
           fm.HANNING: torch.hann_window(ws, periodic=False, dtype=torch.float64),
           fm.BLACKMAN: blackman_coeff - 0.5 * torch.cos(a) + (0.5 - blackman_coeff) * torch.cos(2 * a),
           fm.RECTANGULAR: torch.ones(ws, dtype=torch.float64)}[window_type]
    fr = fr * win.unsqueeze(0)
    if n_fft != ws:
        fr = torch.nn.functional.pad(fr, (0, n_fft - ws))
    if not prm.raw_energy:
        energy = log_energy(fr)
    spec = torch.fft.rfft(fr).abs()
    if prm.use_power:
        spec = spec.pow(2.0)
    # get_mel_banks
    nyquist = 0.5 * samplerate
    if high_freq <= 0.0:
        high_freq += nyquist
    mel = lambda f: 1127.0 * torch.log(1.0 + torch.as_tensor(f, dtype=torch.float64) / 700.0)
    delta = (mel(high_freq) - mel(low_freq)) / (prm.n_mels + 1)
    b = torch.arange(prm.n_mels, dtype=torch.float64).unsqueeze(1)
    left, centre, right = mel(low_freq) + b * delta, mel(low_freq) + (b + 1.0) * delta, mel(low_freq) + (b + 2.0) * delta
    mk = mel(samplerate / n_fft * torch.arange(n_fft // 2, dtype=torch.float64)).unsqueeze(0)
    bins = torch.max(torch.zeros(1, dtype=torch.float64), torch.min((mk - left) / (centre - left), (right - mk) / (right - centre)))
    bins = torch.nn.functional.pad(bins, (0, 1))
    out = spec @ bins.T
    if prm.use_log:
        out = torch.max(out, eps).log()
    if prm.use_energy:
        out = torch.cat((out, energy.unsqueeze(1)) if prm.htk_compat else (energy.unsqueeze(1), out), dim=1)
    return out.numpy()


CASES = [dict(), dict(snip_edges=0), dict(win_length=200, hop=80, n_mels=15, use_energy=1), dict(snip_edges=0, use_energy=1, raw_energy=0, htk_compat=1),
         dict(use_power=0, use_log=0, preemph=0.0), dict(remove_dc=0, use_log=0, use_energy=1, energy_floor=0.5),
         dict(win_length=64, hop=100, n_mels=17, snip_edges=0), dict(win_length=400, n_fft=400, n_mels=40, snip_edges=0)]


@pytest.mark.parametrize("window_type", sorted(WINDOW_NAMES), ids=lambda w: WINDOW_NAMES[w])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_model_is_kaldis_fbank(case, window_type):
    prm = fm.params(**CASES[case])
    rng = np.random.default_rng(case)
    x = (rng.standard_normal(2000) * 0.25 + 0.1).astype(np.float32)
    N = len(x)
    F = fm.n_frames(N, prm.win_length, prm.hop, prm.snip_edges)
    assert F > 3
    w = fm.window64(window_type, prm.win_length)
    W = fm.filters64(16000, prm.n_fft, prm.n_mels, 20.0, -400.0)
    got = fm.values64(x, prm, w, W, F)
    want = kaldi_fbank(torch.from_numpy(x.astype(np.float64)), 16000.0, prm, window_type, 20.0, -400.0)
    assert got.shape == want.shape == (F, fm.cols_of(prm))
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    lo, hi, mid = fm.intervals(x, prm, w.astype(np.float32), W.astype(np.float32), F)
    assert (lo <= mid).all() and (mid <= hi).all()
    assert np.abs(mid - got).max() <= 1e-5 * max(1.0, np.abs(got).max())      # (the float32 tables against the float64 ones)


def test_the_model_is_torchaudios_fbank():
    ta = pytest.importorskip("torchaudio")
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4000) * 3000.0).astype(np.float32)
    for kw in (dict(), dict(snip_edges=0, use_energy=1), dict(use_power=0, htk_compat=1, use_energy=1, raw_energy=0)):
        prm = fm.params(**kw)
        want = ta.compliance.kaldi.fbank(torch.from_numpy(x.astype(np.float64))[None, :], dither=0.0, energy_floor=0.0, num_mel_bins=prm.n_mels,
                                         snip_edges=bool(prm.snip_edges), use_energy=bool(prm.use_energy), raw_energy=bool(prm.raw_energy),
                                         htk_compat=bool(prm.htk_compat), use_power=bool(prm.use_power)).numpy()
        F = fm.n_frames(len(x), prm.win_length, prm.hop, prm.snip_edges)
        got = fm.values64(x, prm, fm.window64(fm.POVEY, 400), fm.filters64(16000, 512, prm.n_mels, 20.0, 0.0), F)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("snip_edges", [1, 0])
@pytest.mark.parametrize("ws,hop", [(400, 160), (64, 100), (25, 10), (2, 1), (7, 7)])
def test_frame_counts_against_brute_force(ws, hop, snip_edges):
    prm = afgpu.fbank_params(ws, hop, max(16, fm.n_fft_of(ws)), snip_edges=bool(snip_edges))
    for N in range(0, 3 * ws + 1):
        if snip_edges:                                           # whole windows that fit
            want = sum(1 for f in range(N + 1) if f * hop + ws <= N)
        else:                                                    # frames whose first half hop, rounded up, lies inside the row
            want = sum(1 for f in range(N + 1) if f * hop + (hop + 1) // 2 <= N)
        assert fm.n_frames(N, ws, hop, snip_edges) == want, N
        assert afgpu.fbank_frames(prm, N) == want, N


@pytest.mark.parametrize("ws,hop", [(400, 160), (200, 80), (64, 100), (25, 10), (1200, 480)])
def test_the_mirror_is_the_flipped_copy_construction(ws, hop):
    pad = fm.pad_of(ws, hop, 0)
    assert pad == ws // 2 - hop // 2
    for N in (ws, ws + hop, 2 * ws - 1, 3 * ws + 7):             # (the construction needs the padded row to hold every frame)
        x = torch.arange(N, dtype=torch.float64)
        want = kaldi_strided(x, ws, hop, 0).numpy().astype(np.int64)
        got = fm.frame_index(N, ws, hop, 0, fm.n_frames(N, ws, hop, 0))
        assert got.shape == want.shape and (got == want).all(), N
    assert list(fm.mirror(np.arange(-4, 8), 3)) == [2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]         # more than one fold on each side


def test_the_windows():
    for ws in (2, 25, 400):
        assert np.allclose(fm.window64(fm.HANNING, ws), torch.hann_window(ws, periodic=False, dtype=torch.float64).numpy(), atol=1e-15)
        assert np.allclose(fm.window64(fm.HAMMING, ws), torch.hamming_window(ws, periodic=False, dtype=torch.float64).numpy(), atol=1e-15)
        assert np.allclose(fm.window64(fm.BLACKMAN, ws), torch.blackman_window(ws, periodic=False, dtype=torch.float64).numpy(), atol=1e-15)
        assert np.allclose(fm.window64(fm.POVEY, ws), torch.hann_window(ws, periodic=False, dtype=torch.float64).pow(0.85).numpy(), atol=1e-15)
        assert (fm.window64(fm.RECTANGULAR, ws) == 1.0).all()
        for wt in WINDOW_NAMES:
            n_fft = max(16, fm.n_fft_of(ws))
            t = afgpu.fbank_tables(wt, ws, n_fft)
            assert t.dtype == np.float32 and (t.view(np.uint32) == fm.tables32(wt, ws, n_fft).view(np.uint32)).all()
            assert (afgpu.fbank_tables(WINDOW_NAMES[wt], ws, n_fft) == t).all()
            if ws <= n_fft:
                assert (t[ws:] == afgpu.mel_fft_tables(n_fft, ws)[ws:]).all()       # the twiddles are the FFT mel path's


@pytest.mark.parametrize("shape", [(16000, 512, 23, 20.0, 0.0), (16000, 512, 80, 20.0, -400.0), (8000, 256, 15, 0.0, 0.0), (16000, 400, 40, 100.0, 7600.0),
                                   (44100, 2048, 128, 20.0, 0.0)], ids=str)
def test_the_bank(shape):
    sr, n_fft, n_mels, low, high = shape
    W = fm.filters64(sr, n_fft, n_mels, low, high)
    got = afgpu.fbank_filters(sr, n_fft, n_mels, low, high)
    assert got.shape == W.shape == (n_mels, n_fft // 2 + 1)
    assert (got.view(np.uint32) == W.astype(np.float32).view(np.uint32)).all()
    assert (W >= 0).all() and (got[:, n_fft // 2].view(np.uint32) == 0).all()
    hi = high + sr / 2.0 if high <= 0 else high
    delta = (fm.mel_of(hi) - fm.mel_of(low)) / (n_mels + 1)
    mk = fm.mel_of(np.arange(n_fft // 2 + 1) * sr / n_fft)
    for m in range(n_mels):
        centre = fm.mel_of(low) + (m + 1) * delta
        inside = np.flatnonzero(W[m] > 0)
        if inside.size:                                          # the peak is the bin nearest the centre on the weight's own scale
            k = int(np.argmax(W[m]))
            assert abs(mk[k] - centre) <= np.abs(mk[inside] - centre).min() + 1e-12
            assert (mk[inside] > centre - delta - 1e-9).all() and (mk[inside] < centre + delta + 1e-9).all()


def test_a_sine_on_a_bin_centre_lands_in_its_filter():
    prm = fm.params(n_mels=40, preemph=0.0, use_log=0)
    k = 64                                                       # 2000 Hz at 16 kHz / 512
    # one period of the transform's length in the frame: the window is shorter, so the line is the window's main lobe at bin k
    x = np.sin(2.0 * np.pi * k * np.arange(4000) / 512.0).astype(np.float32)
    W = fm.filters64(16000, 512, 40, 20.0, 0.0)
    y = fm.values64(x, prm, fm.window64(fm.POVEY, 400), W, fm.n_frames(4000, 400, 160, 1))
    best = int(np.argmax(W[:, k]))
    assert (np.argmax(y, axis=1) == best).all()
    assert (y[:, best] > 100.0 * np.delete(y, [best - 1, best, best + 1], axis=1).max(axis=1)).all()
