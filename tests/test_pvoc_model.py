"""tests/pvoc_model.py against what a phase vocoder must do, against a float64 torch restatement of torchaudio's lines, and
afg_pvoc_out_frames against the count by brute force.  No device."""
import math

import numpy as np
import pytest
import torch

import afgpu
import pvoc_model as pm

RATES = [1.0, 0.5, 2.0, 1.25, 0.8, 1.0 / 3.0, 1.1, 0.9, 64.0, 1.0 / 64.0, 3.0]


def random_spec(rng, n_bins, f):
    mag = rng.uniform(0.5, 2.0, (n_bins, f))
    ang = rng.uniform(-np.pi, np.pi, (n_bins, f))
    return (mag * np.cos(ang)).astype(np.float32), (mag * np.sin(ang)).astype(np.float32)


def test_rate_one_returns_the_input():
    rng = np.random.default_rng(1)
    for n_fft, hop in ((16, 4), (30, 7), (64, 16)):
        re, im = random_spec(rng, n_fft // 2 + 1, 57)
        yr, yi, m = pm.model(re, im, n_fft, hop, 1.0)
        assert yr.shape == re.shape
        scale = np.hypot(re.astype(np.float64), im.astype(np.float64))
        assert (np.abs(yr.astype(np.float64) - re) <= 1e-12 * scale).all() and (np.abs(yi.astype(np.float64) - im) <= 1e-12 * scale).all()


@pytest.mark.parametrize("rate", [0.5, 0.8, 1.25, 3.0])
def test_a_stationary_bin_keeps_its_frequency(rate):
    n_fft, hop, f, A, psi = 64, 16, 200, 1.5, 0.3
    for k, off in ((5, 0.0), (9, 0.3), (20, -0.45), (3, 0.5 - 1e-3)):          # centred, off centre, and with an odd wrap (hop k / n_fft + off hop / n_fft)
        nu = (k + off) / n_fft                                               # cycles per sample
        fr = np.arange(f)
        re = np.zeros((n_fft // 2 + 1, f), np.float64)
        im = np.zeros_like(re)
        re[k], im[k] = A * np.cos(psi + 2 * np.pi * nu * hop * fr), A * np.sin(psi + 2 * np.pi * nu * hop * fr)
        re32, im32 = re.astype(np.float32), im.astype(np.float32)
        yr, yi, m = pm.model(re32, im32, n_fft, hop, rate)
        t = np.arange(yr.shape[1])
        keep = pm.steps(f, rate)[1] + 1 < f                                  # (the last step fades into the zero frame)
        want_r, want_i = A * np.cos(psi + 2 * np.pi * nu * hop * t), A * np.sin(psi + 2 * np.pi * nu * hop * t)
        # the float32 inputs carry 2^-24 of angle each, and t of them add up
        tol = A * (2.0 ** -22) * (t + 2)
        assert (np.abs(yr[k].astype(np.float64) - want_r)[keep] <= tol[keep]).all(), (k, off)
        assert (np.abs(yi[k].astype(np.float64) - want_i)[keep] <= tol[keep]).all(), (k, off)
        assert (yr[np.arange(re.shape[0]) != k] == 0).all()


def torch_phase_vocoder(spec, rate, phase_advance):
    """torchaudio.functional.phase_vocoder's lines, in float64.  Its time_steps = torch.arange(0, frames, rate) are taken as the
    definition's single rounded products t * rate: torch.arange evaluates in vector pieces that round differently, and at rates
    such as 1 / 3 a floor then picks another frame pair -- the reason the definition pins the product down."""
    time_steps = torch.from_numpy(pm.steps(spec.size(-1), rate)[0])
    alphas = time_steps % 1.0
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    s0 = spec.index_select(-1, time_steps.long())
    s1 = spec.index_select(-1, (time_steps + 1).long())
    angle_0, angle_1, norm_0, norm_1 = s0.angle(), s1.angle(), s0.abs(), s1.abs()
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return mag, phase_acc


@pytest.mark.parametrize("rate", [0.8, 1.25, 0.5, 1.0 / 3.0, 1.1, 2.0])
def test_the_model_agrees_with_torchaudios_lines_in_float64(rate):
    rng = np.random.default_rng(3)
    for n_fft, hop in ((16, 4), (64, 16), (400, 160)):
        n_bins, f = n_fft // 2 + 1, 61
        re, im = random_spec(rng, n_bins, f)
        spec = torch.complex(torch.from_numpy(re.astype(np.float64)), torch.from_numpy(im.astype(np.float64)))
        adv = torch.linspace(0, math.pi * hop, n_bins, dtype=torch.float64)[..., None]
        mag, ph = torch_phase_vocoder(spec, rate, adv)
        yr, yi, m = pm.model(re, im, n_fft, hop, rate)
        assert tuple(mag.shape) == yr.shape
        mag, ph = mag.numpy(), ph.numpy()
        assert np.abs(m.astype(np.float64) - mag).max() <= 1e-9
        assert np.abs(yr.astype(np.float64) - mag * np.cos(ph)).max() <= 1e-9 and np.abs(yi.astype(np.float64) - mag * np.sin(ph)).max() <= 1e-9


@pytest.mark.parametrize("rate", RATES + [0.999999999, 1.000000001, 63.99999, 1.0 / 63.5], ids=lambda r: f"{r:.9g}")
def test_out_frames_is_the_count_by_brute_force(rate):
    for f in range(1, 301):
        t = np.arange(int(f / rate) + 70, dtype=np.float64)
        want = int((t * np.float64(rate) < f).sum())
        assert afgpu.pvoc_out_frames(f, rate) == want == pm.out_frames(f, rate), (f, rate)
    for bad in ((0, 1.0), ((1 << 24) + 1, 1.0), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf")), (5, 1.0 / 65), (5, 64.5)):
        with pytest.raises(afgpu.AfgError):
            afgpu.pvoc_out_frames(*bad)
    assert afgpu.pvoc_out_frames(1 << 24, 1.0 / 64) == 1 << 30
