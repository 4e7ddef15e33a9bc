"""The phase-vocoder time stretch of include/afg.h (afg_pvoc_hip), evaluated sequentially in numpy.longdouble, and the interval
the device result is held to.  The steps go through the rounded double product fl(t * rate), as the definition has them;
everything per bin runs over long double (64-bit significand on x86) from the float32 inputs.  Only the phase modulo 2 pi
reaches the result, so the model adds the bin's advance w_k reduced by whole turns -- 2 pi ((hop k) mod n_fft) / n_fft, exact
in integers -- which keeps |ph_t| <= 2 pi t and the model's own error near 2^-64 * 2 pi t: under 1e-4 of the interval."""
import numpy as np

LD = np.longdouble
PI = np.arctan2(LD(0), LD(-1))
TWO_PI = 2 * PI
K_A, K_P = 2, 52                                                 # AFG_PVOC_KA, AFG_PVOC_KP
U, V = 2.0 ** -24, 2.0 ** -53


def steps(n_frames, rate):
    """(s_t, i_t, a_t) for every t >= 0 with s_t = fl(t * rate) < n_frames"""
    rate = np.float64(rate)
    n = int(np.ceil(n_frames / rate)) + 2
    s = np.arange(n, dtype=np.float64) * rate                    # one rounded product each
    s = s[s < n_frames]
    i = np.floor(s)
    return s, i.astype(np.int64), s - i


def out_frames(n_frames, rate):
    return len(steps(n_frames, rate)[0])


def bracket(t):
    """K_A u + K_P v pi (t + 1): E_t = m_t * bracket(t)"""
    return K_A * U + K_P * V * np.pi * (np.asarray(t, dtype=np.float64) + 1.0)


def model(re, im, n_fft, hop, rate, bins=None):
    """re, im: float32 [n_bins, n_frames].  Returns (y_re, y_im, m) as long double [len(bins), out_frames]"""
    n_bins, n_frames = re.shape
    assert n_bins == n_fft // 2 + 1
    bins = np.arange(n_bins) if bins is None else np.asarray(bins)
    s, i, a = steps(n_frames, rate)
    a = a.astype(LD)[None, :]
    zr = np.zeros((len(bins), 1), LD)
    xr = np.concatenate([re[bins].astype(LD), zr], axis=1)       # frame n_frames: (+0, +0)
    xi = np.concatenate([im[bins].astype(LD), zr], axis=1)
    with np.errstate(all="ignore"):
        th = np.arctan2(xi, xr)
        mag = np.sqrt(xr * xr + xi * xi)
        adv = [(hop * int(k)) % n_fft for k in bins]             # w_k modulo 2 pi, exact
        w = (TWO_PI * np.array(adv, dtype=LD) / LD(n_fft))[:, None]
        d = th[:, i + 1] - th[:, i] - w
        p = d - TWO_PI * np.round(d / TWO_PI) + w
        ph = th[:, :1] + np.concatenate([zr, np.cumsum(p, axis=1)[:, :-1]], axis=1)      # exclusive, in step order
        m = a * mag[:, i + 1] + (1 - a) * mag[:, i]
        return m * np.cos(ph), m * np.sin(ph), m


def share(got_re, got_im, y_re, y_im, m):
    """the largest |delivered - model| / E_t over both components (0 where m_t = 0 and the delivered value is a zero);
    inf where a component is outside every interval (not finite, or non-zero at m_t = 0)"""
    t = np.arange(m.shape[1])
    E = m * bracket(t).astype(LD)[None, :]
    worst = 0.0
    with np.errstate(all="ignore"):
        for got, want in ((got_re, y_re), (got_im, y_im)):
            err = np.abs(got.astype(LD) - want)
            zero = m == 0
            if zero.any() and (got[zero] != 0).any():
                return float("inf")
            r = np.where(zero, LD(0), err / np.where(zero, LD(1), E))
            if not np.isfinite(r.astype(np.float64)).all():
                return float("inf")
            worst = max(worst, float(r.max())) if r.size else worst
    return worst
