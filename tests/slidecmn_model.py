"""The sliding-window mean and variance normalisation of include/afg.h ("Sliding-window cepstral mean and variance
normalisation"), restated in numpy: Kaldi's window, the float64 sums in chunks of 32 frames in the header's order, the output.
Every operation is one IEEE float64 operation of numpy, so the device result must equal this one bit for bit."""
import numpy as np

CHUNK = 32
FLOOR = 1e-10
QNAN = np.uint32(0x7fc00000)


def window(t, n_frames, cmn_window, min_cmn_window, center):
    """(ws, we) of frame t of a slab of n_frames frames: Kaldi's SlidingWindowCmnInternal, quirks included."""
    if center:
        ws = t - cmn_window // 2
        we = ws + cmn_window
    else:
        ws = t - cmn_window
        we = t + 1
    if ws < 0:
        we -= ws
        ws = 0
    if not center and we > t:
        we = max(t + 1, min_cmn_window)
    if we > n_frames:
        ws -= we - n_frames
        we = n_frames
        ws = max(ws, 0)
    return ws, we


def _chunk_scans(v):
    """pre and suf of every frame ([N, cols] float64 each) for values v [N, cols] float64."""
    n = v.shape[0]
    pre, suf = np.empty_like(v), np.empty_like(v)
    for c0 in range(0, n, CHUNK):
        c1 = min(c0 + CHUNK, n)
        acc = np.zeros(v.shape[1])
        for j in range(c0, c1):
            acc = acc + v[j]
            pre[j] = acc
        acc = np.zeros(v.shape[1])
        for j in range(c1 - 1, c0 - 1, -1):
            acc = acc + v[j]
            suf[j] = acc
    return pre, suf


def window_sums(x, cmn_window, min_cmn_window, center):
    """(S1, S2, n) per frame for x [N, cols] float32: float64 arrays [N, cols] and the window lengths [N]."""
    x = np.asarray(x, np.float32)
    n_frames, cols = x.shape
    d = x.astype(np.float64)
    vals = (d, d * d)                                            # (the square of a float32 is exact in float64)
    scans = [_chunk_scans(v) for v in vals]
    out = [np.empty((n_frames, cols)), np.empty((n_frames, cols))]
    cnt = np.empty(n_frames, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n_frames):
            ws, we = window(t, n_frames, cmn_window, min_cmn_window, center)
            cnt[t] = we - ws
            a, b = ws // CHUNK, (we - 1) // CHUNK
            for k, (v, (pre, suf)) in enumerate(zip(vals, scans)):
                if a == b:
                    acc = np.zeros(cols)
                    for j in range(ws, we):
                        acc = acc + v[j]
                else:
                    acc = suf[ws].copy()
                    for ch in range(a + 1, b):
                        acc = acc + pre[min(ch * CHUNK + CHUNK, n_frames) - 1]
                    acc = acc + pre[we - 1]
                out[k][t] = acc
    return out[0], out[1], cnt


def sliding_cmn_f64(x, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """The output in float64, in front of the last step (the rounding to float32): [N, cols]."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        s1, s2, cnt = window_sums(x, cmn_window, min_cmn_window, center)
        n = cnt.astype(np.float64)[:, None]
        mean = s1 / n
        d = x.astype(np.float64) - mean
        if not norm_vars:
            return d
        m2 = s2 / n
        mm = mean * mean
        var = m2 - mm
        var = np.where(var < FLOOR, FLOOR, var)                  # (a NaN compares false and stays)
        rs = 1.0 / np.sqrt(var)
        y = d * rs
        y[cnt == 1] = 0.0
        return y


def sliding_cmn(x, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """The stage's output for a slab x [N, cols] float32 (frames first, whatever the layout in memory): float32 [N, cols],
    every NaN the positive quiet one."""
    x = np.asarray(x, np.float32)
    if x.shape[0] == 0:
        return x.copy()
    with np.errstate(all="ignore"):
        y = sliding_cmn_f64(x, cmn_window, min_cmn_window, center, norm_vars).astype(np.float32)
    bits = y.view(np.uint32).copy()
    bits[np.isnan(y)] = QNAN
    return bits.view(np.float32)
