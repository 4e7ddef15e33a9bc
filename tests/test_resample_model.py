"""tests/resample_model.py on its own (no GPU, no library): the float32 restatement against the float64 definition, the
filter's accuracy on a sine and at DC for the rate pairs a corpus mixes, and equal rates."""
import numpy as np
import pytest

import resample_model as rm

PAIRS = [(44100, 16000), (48000, 16000), (44100, 48000), (8000, 16000), (22050, 16000)]
WIDTHS = [17, 19, 7, 7, 9]


def test_widths_of_the_named_pairs():
    assert [rm.shape(a, b)[2] for a, b in PAIRS] == WIDTHS
    assert rm.shape(44100, 16000)[:2] == (441, 160) and rm.shape(16000, 16000)[:3] == (1, 1, 0)


@pytest.mark.parametrize("pair", PAIRS + [(96000, 8000)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_float32_sum_stays_within_the_forward_bound(pair):
    """the float32 sum of K = 2 W rounded products is within (K + 2) * 2^-24 * sum |h_k x_k| of the float64 sum of the same
    terms (a term passes through one product rounding and at most K add roundings of 2^-24 each), on random rows"""
    rng = np.random.default_rng(pair[0] + pair[1])
    M, L, W, _ = rm.shape(*pair)
    h = rm.taps32(*pair)
    for n_in, n_out, f0 in ((3000, 2000, 0), (500, 700, 123), (40, 300, -5)):
        x = rng.standard_normal(n_in).astype(np.float32)
        got = rm.resample32(x, h, M, L, W, n_out, f0).astype(np.float64)
        want = rm.resample64(x, h, M, L, W, n_out, f0)
        bound = (2 * W + 2) * 2.0 ** -24 * rm.abs_sum64(x, h, M, L, W, n_out, f0)
        assert (np.abs(got - want) <= bound).all(), float(np.max(np.abs(got - want) - bound))
        assert np.abs(want).max() > 0.1


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_a_sine_comes_out_as_the_sine_at_the_new_rate(pair):
    """1 kHz, amplitude 0.5, in float64 against the analytic sine: 4e-4 away from the ends (2.9e-4 was the worst measured)"""
    a, b = pair
    M, L, W, _ = rm.shape(a, b)
    n_in = a // 5
    x = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n_in) / a)
    n_out = n_in * b // a
    y = rm.resample64(x, rm.taps64(a, b), M, L, W, n_out)
    want = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n_out) / b)
    edge = 2 * W * b // a + 2 * W + 2
    err = np.abs(y - want)[edge:n_out - edge]
    print(pair, "max error", float(err.max()))
    assert err.size > 1000 and err.max() <= 4e-4


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_dc_gain_of_every_phase(pair):
    gain = rm.taps64(*pair).sum(1)
    print(pair, "DC gain off by", float(np.abs(gain - 1).max()))
    assert np.abs(gain - 1).max() <= 1e-3


def test_equal_rates_are_the_identity_on_bit_patterns():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)          # NaNs with payloads, infinities, -0, denormals
    x[:4] = [0x7fc0dead, 0xff800000, 0x80000000, 0x00000001]
    y = rm.resample32(x.view(np.float32), None, 1, 1, 0, 600, -20)
    assert (y.view(np.uint32)[20:520] == x).all() and (y.view(np.uint32)[:20] == 0).all() and (y.view(np.uint32)[520:] == 0).all()
    one = rm.mix(x.view(np.float32)[None, :])
    assert (one.view(np.uint32) == x).all()
    t = rm.tensor([{"status": 0, "pcm": x.view(np.float32).reshape(-1, 1), "channels": 1, "samplerate": 16000.0, "frames": 500}], 2, 510, 16000)
    assert (t[0, 0].view(np.uint32)[:500] == x).all() and (t.view(np.uint32)[0, 0, 500:] == 0).all() and (t.view(np.uint32)[0, 1] == 0).all()


def test_the_mix_is_the_mean_in_row_order():
    rows = np.float32([[1e8, 1, -3], [1, 1e8, 1], [-1e8, -1e8, 2]])
    want = [np.float32(np.float32(np.float32(1e8) + np.float32(1)) + np.float32(-1e8)) / np.float32(3),
            np.float32(np.float32(np.float32(1) + np.float32(1e8)) + np.float32(-1e8)) / np.float32(3), np.float32(0)]
    assert rm.mix(rows).tolist() == [float(v) for v in want]
