"""numpy model of the YIN pitch stage of include/afg.h (afg_yin_hip): the float32 restatement of the definition, step by
step in the stated arithmetic order (yin32: what the device must deliver bit for bit), and a plain float64 "paper"
definition (yin64: direct sums, a sequential cumulative sum, the same selection rule) with the margin by which it decides."""
from types import SimpleNamespace

import numpy as np

from melspec_model import fmaf32

PAD_REFLECT, PAD_ZERO = 0, 1
CHUNK = 16
NAN_WORD = 0x7fc00000


def params(samplerate=16000.0, frame_length=1024, win_length=None, hop=None, tau_min=32, tau_max=320, threshold=0.1, center=1, pad_mode=PAD_ZERO):
    win_length = frame_length // 2 if win_length is None else win_length
    hop = frame_length // 4 if hop is None else hop
    return SimpleNamespace(samplerate=float(samplerate), frame_length=frame_length, win_length=win_length, hop=hop, tau_min=tau_min,
                           tau_max=tau_max, threshold=np.float32(threshold), center=int(center), pad_mode=pad_mode)


def lags(samplerate, fmin, fmax, frame_length, win_length):
    """librosa.yin's lines: min_period = floor(sr / fmax), max_period = min(ceil(sr / fmin), frame_length - win_length - 1)"""
    return int(np.floor(samplerate / fmax)), min(int(np.ceil(samplerate / fmin)), frame_length - win_length - 1)


def n_frames(in_frames, p):
    num = in_frames + 2 * (p.frame_length // 2 if p.center else 0) - p.frame_length
    return 0 if num < 0 else 1 + num // p.hop


def frame_index(p, frames):
    """[frames, W + tau_max]: the row index of every sample a frame reads, before the padding rule"""
    pad = p.frame_length // 2 if p.center else 0
    return (np.arange(frames, dtype=np.int64) * p.hop)[:, None] + (np.arange(p.win_length + p.tau_max, dtype=np.int64) - pad)[None, :]


def frames_of(x, p, frames):
    """[frames, W + tau_max]: samples 0 .. W - 1 + tau_max of every frame, reflected or +0.0f outside the row"""
    x = np.asarray(x)
    idx = frame_index(p, frames)
    if p.pad_mode == PAD_REFLECT:
        assert frames == 0 or not p.center or len(x) > p.frame_length // 2
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= len(x), 2 * (len(x) - 1) - idx, idx)
    ok = (idx >= 0) & (idx < len(x))
    if len(x) == 0:
        return np.zeros(idx.shape, x.dtype)
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], x.dtype.type(0))


def difference32(fr, W, tau_max):
    """step 1: d[f, tau], tau = 0 .. tau_max: the fmaf chain over j = 0 .. W - 1 from +0.0f of e = float32(x_j - x_(j+tau))"""
    fr = np.asarray(fr, np.float32)
    acc = np.zeros((fr.shape[0], tau_max + 1), np.float32)
    with np.errstate(all="ignore"):
        for j in range(W):
            e = fr[:, j:j + 1] - fr[:, j:j + tau_max + 1]
            acc = fmaf32(e, e, acc)
    return acc


def difference64(fr, W, tau_max):
    """the direct sums in float64 (exact for integer samples, whatever the order)"""
    fr = np.asarray(fr, np.float64)
    out = np.zeros((fr.shape[0], tau_max + 1))
    for tau in range(tau_max + 1):
        e = fr[:, :W] - fr[:, tau:tau + W]
        out[:, tau] = (e * e).sum(axis=1)
    return out


def cmnd_chunked(d):
    """step 2 on float32 d[f, 0 .. tau_max]: float32 d'[f, 0 .. tau_max] (column 0 unused, 1.0f)"""
    F, T = d.shape[0], d.shape[1] - 1
    C = -(-T // CHUNK)
    dd = np.zeros((F, C * CHUNK))
    dd[:, :T] = d[:, 1:].astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.add.accumulate(dd.reshape(F, C, CHUNK), axis=2)   # sequential inside a chunk
        B = np.zeros((F, C))
        for c in range(1, C):
            B[:, c] = B[:, c - 1] + p[:, c - 1, -1]
        s = (B[:, :, None] + p).reshape(F, C * CHUNK)[:, :T]
        tau = np.arange(1, T + 1, dtype=np.float64)[None, :]
        q = (dd[:, :T] * tau / np.where(s == 0, 1.0, s)).astype(np.float32)
    out = np.ones((F, T + 1), np.float32)
    out[:, 1:] = np.where(s == 0, np.float32(1.0), q)
    return out


def cmnd_sequential(d):
    """the paper's d' in float64: d(tau) tau / sum_(1..tau) d, 1 where the sum is 0"""
    d = np.asarray(d, np.float64)
    s = np.add.accumulate(d[:, 1:], axis=1)
    tau = np.arange(1, d.shape[1], dtype=np.float64)[None, :]
    out = np.ones(d.shape)
    with np.errstate(all="ignore"):
        out[:, 1:] = np.where(s == 0, 1.0, d[:, 1:] * tau / np.where(s == 0, 1.0, s))
    return out


def choose(dp, tau_min, tau_max, threshold):
    """step 3, one frame: tau*"""
    for tau in range(tau_min, tau_max + 1):
        if not dp[tau] < threshold or tau_min == tau_max or tau == tau_max:
            continue
        if dp[tau] < dp[tau + 1] if tau == tau_min else (dp[tau] < dp[tau - 1] and dp[tau] <= dp[tau + 1]):
            return tau
    return tau_min + int(np.argmin(dp[tau_min:tau_max + 1]))    # the first that attains the minimum


def refine(dp, ts, tau_min, tau_max, samplerate):
    """step 4, one frame: float32 f0"""
    shift = 0.0
    if tau_min < ts < tau_max:
        a, b, c = (np.float64(dp[ts - 1]), np.float64(dp[ts]), np.float64(dp[ts + 1]))
        with np.errstate(all="ignore"):
            A = (c + a) - 2.0 * b
            B = (c - a) * 0.5
            if abs(B) < abs(A):
                shift = -B / A
    return np.float32(samplerate / (np.float64(ts) + shift))


def finish(dp, p):
    """steps 3 to 5 on d'[f, 0 .. tau_max] (float32 or float64): (planes [2, f] float32, tau* [f], 0 where the frame is NaN)"""
    F = dp.shape[0]
    planes = np.zeros((2, F), np.float32)
    taus = np.zeros(F, np.int64)
    for f in range(F):
        if np.isnan(dp[f, 1:]).any():
            planes.view(np.uint32)[:, f] = NAN_WORD
            continue
        taus[f] = choose(dp[f], p.tau_min, p.tau_max, p.threshold)
        planes[0, f] = refine(dp[f], taus[f], p.tau_min, p.tau_max, p.samplerate)
        planes[1, f] = dp[f, taus[f]]
    return planes, taus


def yin32(x, p, frames):
    """the definition as the device computes it: (planes [2, frames] float32, tau*, d [frames, tau_max + 1] float32)"""
    fr = frames_of(np.ascontiguousarray(x, np.float32), p, frames)
    d = difference32(fr, p.win_length, p.tau_max)
    planes, taus = finish(cmnd_chunked(d), p)
    return planes, taus, d


def yin64(x, p, frames, round32=False):
    """the paper's definition in float64: (planes, tau*, d, d'); round32: d' rounded to float32 as include/afg.h delivers it,
    the one rounding the definition has when d and its sums are exact"""
    fr = frames_of(np.asarray(x, np.float64), p, frames)
    d = difference64(fr, p.win_length, p.tau_max)
    dp = cmnd_sequential(d)
    if round32:
        dp = dp.astype(np.float32)
    planes, taus = finish(dp, p)
    return planes, taus, d, dp


def decided(dp, ts, p, rel):
    """one frame of the float64 definition: True when every comparison the selection makes on the way to tau* -- d' against
    the threshold first, a lag's neighbours only where it is below, or the minimum against every other lag -- differs by more
    than rel * max(|operands|)"""
    far = lambda a, b: abs(a - b) > rel * max(abs(a), abs(b))
    thr = float(p.threshold)
    found = False
    for tau in range(p.tau_min, p.tau_max + 1):
        if not far(dp[tau], thr):
            return False
        if not dp[tau] < thr or p.tau_min == p.tau_max or tau == p.tau_max:
            continue
        if not far(dp[tau], dp[tau + 1]) or (tau > p.tau_min and not far(dp[tau], dp[tau - 1])):
            return False
        if tau == ts:
            found = True
            break
    if found:
        return True
    others = np.delete(dp[p.tau_min:p.tau_max + 1], ts - p.tau_min)
    return all(far(dp[ts], o) for o in others)
