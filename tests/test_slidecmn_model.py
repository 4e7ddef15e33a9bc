"""The numpy model of the sliding-window normalisation (tests/slidecmn_model.py, include/afg.h) on the CPU: its error against
the same definition evaluated exactly, its agreement with torchaudio.functional.sliding_window_cmn, the window rule against a
table written out by hand, and the n == 1 and floor options.

Error against exact arithmetic.  The exact value takes the window's sums, the mean and the variance as fractions and the
square root and the quotient in 60 decimal digits.  With u = 2^-53, A the window's sum of |x| and B its sum of x^2, the model's
float64 value in front of its last rounding differs from it to first order by at most
    e_mean = u ((n - 1) A / n + |mean|)                                   the sum in any order, then the division
    without norm_vars:  e_mean + u |y|                                    the subtraction
    with norm_vars:     (e_mean + u |d|) rs + |y| (e_var / (2 var) + 3 u),  e_var = u ((n - 1) B / n + 2 m2 + 3 mm) + 2 |mean| e_mean
(d = x - mean, rs = var^-1/2; S2 / n, mean * mean and their difference round once each; the square root, the reciprocal and the
product are the 3 u), and the rounding to float32 adds half an ulp.  The test asserts 1.05 times that bound per element and
prints the largest error it met, in float32 ulps of the exact value; DESIGN.md 3.27 quotes the figures.  The one-pass variance
is Kaldi's, and on a DC offset it is the term e_var / var that grows: the definition's own property, not the order's."""
import os
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slidecmn_model as model

getcontext().prec = 60
U = 2.0 ** -53


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def _exact(x, cmn_window, min_cmn_window, center, norm_vars):
    """Per element: (exact y as Decimal, the first-order bound of the float64 error)."""
    n_frames, cols = x.shape
    fx = [[Fraction(float(v)) for v in row] for row in x]
    ys, bounds = np.empty(x.shape, object), np.empty(x.shape)
    for t in range(n_frames):
        ws, we = model.window(t, n_frames, cmn_window, min_cmn_window, center)
        n = we - ws
        for c in range(cols):
            col = [fx[j][c] for j in range(ws, we)]
            s1, s2 = sum(col), sum(v * v for v in col)
            a, b = float(sum(abs(v) for v in col)), float(s2)
            mean = s1 / n
            d = fx[t][c] - mean
            e_mean = U * ((n - 1) * a / n + abs(float(mean)))
            if not norm_vars:
                ys[t, c], bounds[t, c] = _dec(d), e_mean + U * abs(float(d))
                continue
            if n == 1:
                ys[t, c], bounds[t, c] = Decimal(0), 0.0
                continue
            var = s2 / n - mean * mean
            var = max(var, Fraction(model.FLOOR))
            rs = 1 / _dec(var).sqrt()
            y = _dec(d) * rs
            m2, mm = b / n, float(mean * mean)
            e_var = U * ((n - 1) * b / n + 2 * m2 + 3 * mm) + 2 * abs(float(mean)) * e_mean
            ys[t, c] = y
            bounds[t, c] = (e_mean + U * abs(float(d))) * float(rs) + abs(float(y)) * (e_var / (2 * float(var)) + 3 * U)
    return ys, bounds


def _inputs(kind, rng, n_frames, cols):
    if kind == "noise":
        return rng.standard_normal((n_frames, cols)).astype(np.float32)
    if kind == "dc":
        return (rng.standard_normal((n_frames, cols)) + 1e4).astype(np.float32)
    return rng.integers(-1000, 1001, (n_frames, cols)).astype(np.float32)


@pytest.mark.parametrize("kind", ["noise", "dc", "integers"])
@pytest.mark.parametrize("center,norm_vars,cmn_window,min_cmn_window", [(True, True, 300, 100), (False, False, 600, 100),
                                                                         (False, True, 70, 40), (True, False, 33, 1)])
def test_model_error_against_exact_arithmetic(kind, center, norm_vars, cmn_window, min_cmn_window):
    rng = np.random.default_rng(len(kind) * 100 + cmn_window)
    x = _inputs(kind, rng, 130, 3)
    got = model.sliding_cmn(x, cmn_window, min_cmn_window, center, norm_vars)
    ys, bounds = _exact(x, cmn_window, min_cmn_window, center, norm_vars)
    worst = 0.0
    for t in range(x.shape[0]):
        for c in range(x.shape[1]):
            y = ys[t, c]
            once = np.float32(float(y))                          # (60 digits to float64 to float32: the exact value rounded once,
            ulp = float(np.spacing(np.abs(once)))                #  but for a double rounding no value here comes near)
            err = abs(float(Decimal(float(got[t, c])) - y))
            worst = max(worst, err / ulp)
            assert err <= 0.5 * ulp + 1.05 * bounds[t, c] + 1e-300, (t, c, err / ulp)
            if kind == "integers":
                assert got[t, c].view(np.uint32) == once.view(np.uint32), (t, c)
    print(f"slidecmn model, {kind}, center {center}, norm_vars {norm_vars}, window {cmn_window}: largest error {worst:.4f} float32 ulp")


def _torchaudio_f64(x, cmn_window, min_cmn_window, center, norm_vars):
    """torchaudio.functional.sliding_window_cmn's own lines for one [frames, cols] slab, in float64: running sums that take the
    frame leaving the window off and add the one entering it, no variance floor."""
    x = x.astype(np.float64)
    n_frames, cols = x.shape
    out = np.zeros_like(x)
    cur_sum, cur_sumsq = np.zeros(cols), np.zeros(cols)
    last_start, last_end = -1, -1
    for t in range(n_frames):
        if center:
            start = t - cmn_window // 2
            end = start + cmn_window
        else:
            start = t - cmn_window
            end = t + 1
        if start < 0:
            end -= start
            start = 0
        if not center:
            if end > t:
                end = max(t + 1, min_cmn_window)
        if end > n_frames:
            start -= end - n_frames
            end = n_frames
            if start < 0:
                start = 0
        if last_start == -1:
            part = x[start:end - start]
            cur_sum += part.sum(0)
            if norm_vars:
                cur_sumsq += np.cumsum(part ** 2, 0)[-1]
        else:
            if start > last_start:
                cur_sum -= x[last_start]
                if norm_vars:
                    cur_sumsq -= x[last_start] ** 2
            if end > last_end:
                cur_sum += x[last_end]
                if norm_vars:
                    cur_sumsq += x[last_end] ** 2
        frames = end - start
        last_start, last_end = start, end
        out[t] = x[t] - cur_sum / frames
        if norm_vars:
            if frames == 1:
                out[t] = 0.0
            else:
                variance = cur_sumsq / frames
                variance = variance - cur_sum ** 2 / (frames * frames)
                out[t] *= variance ** -0.5
    return out


TA_CASES = [(n, w, m, center, nv) for n in (40, 150) for (w, m) in ((30, 10), (30, 60), (300, 100), (300, 200), (64, 1))
            for center in (False, True) for nv in (False, True)]


@pytest.mark.parametrize("n_frames,cmn_window,min_cmn_window,center,norm_vars", TA_CASES)
def test_model_agrees_with_torchaudios_lines(n_frames, cmn_window, min_cmn_window, center, norm_vars):
    """Noise of standard deviation 2: the windows of two frames or more have variances far above the 1e-10 floor, so the floor
    the definition has and torchaudio lacks plays no part."""
    rng = np.random.default_rng(n_frames * 1000 + cmn_window)
    x = (rng.standard_normal((n_frames, 4)) * 2.0 + 0.5).astype(np.float32)
    got = model.sliding_cmn_f64(x, cmn_window, min_cmn_window, center, norm_vars)
    want = _torchaudio_f64(x, cmn_window, min_cmn_window, center, norm_vars)
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("n_frames,cmn_window,min_cmn_window,center,norm_vars", TA_CASES)
def test_model_agrees_with_torchaudio_itself(n_frames, cmn_window, min_cmn_window, center, norm_vars):
    torch = pytest.importorskip("torch")
    F = pytest.importorskip("torchaudio.functional")
    rng = np.random.default_rng(n_frames * 1000 + cmn_window)
    x = (rng.standard_normal((n_frames, 4)) * 2.0 + 0.5).astype(np.float32)
    got = model.sliding_cmn(x, cmn_window, min_cmn_window, center, norm_vars)
    want = F.sliding_window_cmn(torch.from_numpy(x), cmn_window, min_cmn_window, center, norm_vars).numpy()
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


# (ws, we) of t = 0 .. 4 for N = 5, worked out by hand from the rule in include/afg.h
WINDOW_TABLE = {
    # center, cmn_window, min_cmn_window
    (True, 3, 1): [(0, 3), (0, 3), (1, 4), (2, 5), (2, 5)],
    (True, 3, 4): [(0, 3), (0, 3), (1, 4), (2, 5), (2, 5)],     # (min_cmn_window plays no part when centred)
    (True, 4, 1): [(0, 4), (0, 4), (0, 4), (1, 5), (1, 5)],
    (True, 4, 4): [(0, 4), (0, 4), (0, 4), (1, 5), (1, 5)],
    (False, 3, 1): [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5)],    # (cmn_window + 1 frames once the slab has them)
    (False, 3, 4): [(0, 4), (0, 4), (0, 4), (0, 4), (1, 5)],
    (False, 4, 1): [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)],
    (False, 4, 4): [(0, 4), (0, 4), (0, 4), (0, 4), (0, 5)],
}


@pytest.mark.parametrize("key", sorted(WINDOW_TABLE))
def test_window_rule_against_the_hand_table(key):
    center, cmn_window, min_cmn_window = key
    assert [model.window(t, 5, cmn_window, min_cmn_window, center) for t in range(5)] == WINDOW_TABLE[key]


def test_window_stays_inside_the_slab():
    for n in (1, 2, 5, 33, 70):
        for w in (1, 2, 3, 32, 33, 600):
            for m in (1, 4, 100):
                for center in (False, True):
                    last = (0, 0)
                    for t in range(n):
                        ws, we = model.window(t, n, w, m, center)
                        assert 0 <= ws < we <= n and ws >= last[0] and we >= last[1]
                        last = (ws, we)


def test_a_window_of_one_frame_gives_zero_with_norm_vars_and_the_difference_without():
    x = np.array([[3.0, -2.0], [5.0, 7.0], [1.0, 1.0]], np.float32)
    # causal, min_cmn_window 1: frame 0 has the window (0, 1)
    y = model.sliding_cmn(x, 2, 1, False, True)
    assert (y[0].view(np.uint32) == 0).all() and (y[1:] != 0).all()
    y = model.sliding_cmn(x, 2, 1, False, False)
    assert (y[0].view(np.uint32) == 0).all()                     # x - x / 1 = +0
    # a slab of one frame: every mode has n == 1
    one = np.array([[4.0, -0.0]], np.float32)
    for center in (False, True):
        assert (model.sliding_cmn(one, 300, 100, center, True).view(np.uint32) == 0).all()


def test_the_variance_floor():
    # a constant column: var is 0 (or a rounding residue below 1e-10) and becomes 1e-10; y = (x - mean) * 1e5
    x = np.full((40, 1), 0.1, np.float32)
    y = model.sliding_cmn(x, 8, 1, True, True)
    assert np.isfinite(y).all() and np.abs(y).max() <= 1e-3
    # a column that leaves its mean by 1e-6: var = 1e-12 is floored, so y = +-1e-6 * 1e5 and not +-1
    x = np.tile(np.array([[1e-6], [-1e-6]], np.float32), (20, 1))
    y = model.sliding_cmn(x, 8, 1, True, True)
    assert np.allclose(np.abs(y), 0.1, rtol=1e-5)
    # just above the floor nothing is clamped: +-1e-4 has var 1e-8
    x = np.tile(np.array([[1e-4], [-1e-4]], np.float32), (20, 1))
    y = model.sliding_cmn(x, 8, 1, True, True)
    assert np.allclose(np.abs(y), 1.0, rtol=1e-5)
    # a NaN variance stays NaN and comes out as the one quiet NaN
    x = np.ones((10, 1), np.float32)
    x[4, 0] = np.nan
    y = model.sliding_cmn(x, 4, 1, True, True)
    nan = np.isnan(y[:, 0])
    assert (y.view(np.uint32)[nan] == 0x7fc00000).all()
    assert list(nan) == [model.window(t, 10, 4, 1, True)[0] <= 4 < model.window(t, 10, 4, 1, True)[1] for t in range(10)]
