"""tests/normalize_model.py against arithmetic that does not share its order: the sums against math.fsum, the standard mode's
output against the mean and variance it promises, the dynamic-range mode against Whisper's own expression."""
import math

import numpy as np

import normalize_model as nm

U32 = 2.0 ** -24                                                 # unit roundoff of float32
U64 = 2.0 ** -53


def mixed(rng, n):
    """float32 of mixed magnitude and sign, so that the order of a summation shows in its last bits"""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)


def test_sums_are_within_the_bound_of_recursive_summation():
    """any order of n float64 adds is within (n - 1) u sum|x| of the exact sum (Higham, Accuracy and Stability, 4.2); the
    squares of float32 are exact in float64, so the same holds for them"""
    rng = np.random.default_rng(11)
    for rows, valid in ((1, 1), (1, 255), (1, 4096), (2, 4097), (3, 2 * 4096 + 5)):
        x = mixed(rng, rows * valid).reshape(rows, valid)
        s, q = nm.group_sums(x)
        flat = [float(v) for v in x.ravel()]
        exact_s, exact_q = math.fsum(flat), math.fsum(v * v for v in flat)
        assert abs(s - exact_s) <= len(flat) * U64 * math.fsum(abs(v) for v in flat)
        assert abs(q - exact_q) <= len(flat) * U64 * exact_q
        st = nm.group_stats(x, nm.params(nm.NONE))
        assert st["sum"] == s and st["sumsq"] == q and st["count"] == len(flat)
        assert st["min"] == x.min() and st["max"] == x.max() and st["offset"] == 0 and st["scale"] == 1


def test_the_order_of_the_tiles_shows_in_the_bits():
    rng = np.random.default_rng(12)
    x = mixed(rng, 5 * 4096).reshape(1, -1)
    a, b = nm.group_sums(x), nm.group_sums(x, tile_order=[4, 3, 2, 1, 0])
    assert a != b and abs(a[0] - b[0]) <= 5 * 4096 * U64 * float(np.abs(x.astype(np.float64)).sum())


def test_min_and_max_leave_nan_out_and_order_the_zeros():
    x = np.array([0.0, np.nan, -0.0, 0.0], np.float32)
    mn, mx = nm.min_max(x)
    assert mn == 0 and np.signbit(mn) and mx == 0 and not np.signbit(mx)
    assert nm.min_max(np.array([np.nan], np.float32)) == (np.inf, -np.inf)
    st = nm.group_stats(np.array([[1.0, np.nan, -3.0]], np.float32), nm.params(nm.PEAK, target=0.5))
    assert st["min"] == -3 and st["max"] == 1 and np.isnan(st["sum"]) and np.isnan(st["sumsq"])
    assert st["scale"] == np.float32(0.5) / np.float32(3.0)
    zero = nm.group_stats(np.zeros((2, 7), np.float32), nm.params(nm.RMS))
    assert zero["scale"] == 1 and zero["offset"] == 0 and zero["count"] == 14


def test_standard_mode_gives_zero_mean_and_unit_variance_within_float32_rounding():
    """y = fl(fl(x - o) * s) with o = fl32(mean) and s = fl32(1 / sd), sd = sqrt(var + eps).  With z = (x - mean) / sd the exact
    result, y = z + err and |err| <= a |z| + b, where a = 3.01 u covers the two roundings of the apply and that of s, and
    b = 1.01 u |mean| / sd the rounding of o (u = 2^-24; the data are far from underflow).  mean(z) = 0 and
    mean(z^2) = rho = var / (var + eps) <= 1, so mean|z| <= 1 and
        |mean(y)|    <= a + b
        |var(y) - 1| <= (1 - rho) + 2 a + 2 b + 2 a^2 + 2 b^2 + (a + b)^2
    The mean and var the mode used are float64 results of `count` adds: c = count 2^-52 mean(x^2) / (var + eps) is added to
    both for that."""
    rng = np.random.default_rng(13)
    for rows, valid, shift, eps in ((1, 1000, 0.0, 0.0), (2, 4097, 3.0, 0.0), (1, 2 * 4096 + 5, -0.25, 1e-5), (3, 255, 100.0, 1e-3)):
        x = (rng.standard_normal((rows, valid)) * 0.3 + shift).astype(np.float32)
        prm = nm.params(nm.STANDARD, eps=eps)
        st = nm.group_stats(x, prm)
        y = nm.apply(x, st, prm)
        assert y.dtype == np.float32 and y.shape == x.shape
        n = x.size
        mean, m2 = float(st["sum"]) / n, float(st["sumsq"]) / n
        var = max(m2 - mean * mean, 0.0)
        e = float(np.float32(eps)) if eps else float(np.float32(1e-7))
        sd = math.sqrt(var + e)
        a, b, c = 3.01 * U32, 1.01 * U32 * abs(mean) / sd, n * 2.0 ** -52 * m2 / (var + e)
        flat = [float(v) for v in y.ravel()]
        y_mean = math.fsum(flat) / n
        y_var = math.fsum(v * v for v in flat) / n - y_mean * y_mean
        print(f"rows {rows} valid {valid}: |mean| {abs(y_mean):.3g} (bound {a + b + c:.3g}), |var - 1| {abs(y_var - 1):.3g}")
        assert abs(y_mean) <= a + b + c
        assert abs(y_var - 1.0) <= e / (var + e) + 2 * a + 2 * b + 2 * a * a + 2 * b * b + (a + b) ** 2 + c
        assert st["offset"] == np.float32(mean) and st["scale"] == np.float32(1.0 / sd)


def test_dynamic_range_mode_is_whispers_expression():
    rng = np.random.default_rng(14)
    x = np.log10(np.maximum(rng.standard_normal((80, 301)) ** 2 * 10.0 ** rng.integers(-12, 2, (80, 301)), 1e-10)).astype(np.float32)
    prm = nm.params(nm.DYNAMIC_RANGE, **nm.WHISPER)
    st = nm.group_stats(x.reshape(1, -1), prm)
    y = nm.apply(x, st, prm)
    want = (np.maximum(x, x.max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
    assert want.dtype == np.float32 and nm.same_bits(y, want).size == 0
    assert (x < x.max() - 8).any() and st["offset"] == x.max() - np.float32(8) and st["scale"] == np.float32(0.25)
    nan = x.copy()
    nan[3, 5] = np.nan                                           # a NaN sample takes the floor
    assert nm.apply(nan, st, prm)[3, 5] == (st["offset"] + np.float32(4)) * np.float32(0.25)


def test_peak_and_rms_reach_their_target():
    rng = np.random.default_rng(15)
    x = (rng.standard_normal((2, 5000)) * 0.1).astype(np.float32)
    for mode, measure in ((nm.PEAK, lambda y: np.abs(y).max()), (nm.RMS, lambda y: math.sqrt(float((y.astype(np.float64) ** 2).mean())))):
        prm = nm.params(mode, target=0.5)
        y = nm.apply(x, nm.group_stats(x, prm), prm)
        assert abs(measure(y) - 0.5) <= 0.5 * 4 * U32            # the roundings of r, scale and the product


def test_normalize_touches_the_valid_elements_only_and_layout_counts_tiles():
    rng = np.random.default_rng(16)
    plane = mixed(rng, 3 * 6000)
    groups = np.zeros(3, nm.GROUP_DTYPE)
    groups["in_off"] = groups["out_off"] = [0, 6000, 12000]
    groups["stride"] = [0, 3000, 6000]
    groups["rows"] = [1, 2, 1]
    groups["valid"] = [4097, 2999, 0]
    assert nm.layout(groups) == 2 + 2 + 0 and groups["first_tile"].tolist() == [0, 2, 4]
    sentinel = np.full(plane.size, np.nan, np.float32)
    out, stats = nm.normalize(plane, sentinel, groups, nm.params(nm.PEAK))
    written = ~np.isnan(out)
    want = np.zeros(plane.size, bool)
    want[:4097] = want[6000:6000 + 2999] = want[9000:9000 + 2999] = True
    assert (written == want).all() and stats["count"].tolist() == [4097, 2 * 2999, 0] and stats[2].tobytes() == bytes(40)
    for valid, tiles in ((0, 0), (1, 1), (4096, 1), (4097, 2)):
        g = np.zeros(1, nm.GROUP_DTYPE)
        g["rows"], g["valid"] = 1, valid
        assert nm.layout(g) == tiles
    assert nm.valid_length(3001, 0, 8000, 16000, 4000) == 4000 and nm.valid_length(1000, 0, 8000, 16000, 4000) == 2000
    assert nm.valid_length(9000, 0, 44100, 16000, 4000) == -(-9000 * 160 // 441) and nm.valid_length(5, 5, 8000, 16000, 10) == 0
