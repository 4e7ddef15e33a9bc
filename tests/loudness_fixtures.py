"""The groups the loudness tests measure, per sample rate, and the model's results for them (tests/loudness_model.py), computed
once per rate: test_loudness_model.py checks that none of their gate decisions is close to flipping, test_loudness_gpu.py holds
the device to them."""
import functools

import numpy as np

import loudness_model as lm

RATES = (8000, 16000, 11025, 44100)                             # steps 800, 1600 (multiples of 16) and 1103, 4410 (not)
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 1.41, 1.41)                      # BS.1770's 5.1: the LFE row does not count
LOUD, PASSAGE, TAIL = 0.5, 0.5 * 10.0 ** (-30.0 / 20.0), 1e-5   # amplitudes: programme, 30 dB below it, below the absolute gate


def lengths(rate):
    s = lm.step_of(rate)
    return [0, 4 * s - 1, 4 * s, 4 * s + 1, 5 * s - 1, 5 * s, 4095, 4096, 4097, 8191, 8193, long_length(rate)]


def long_length(rate):
    return int(3.4 * rate) + 7


def signal(rng, rows, n, shaped=False, amplitude=LOUD):
    """[rows, n] float32 noise, every row at its own level; shaped: a loud part, a passage 30 dB down -- under the relative
    gate -- and a tail under the absolute gate"""
    x = rng.uniform(-1.0, 1.0, (rows, n))
    env = np.full(n, amplitude)
    if shaped:
        env[int(0.4 * n):int(0.7 * n)] = PASSAGE
        env[int(0.7 * n):] = TAIL
    return (x * env * (1.0 - 0.1 * np.arange(rows))[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def groups(rate):
    """(list of [rows, valid] float32 arrays, list of (a, b): groups a and b hold the same samples)"""
    rng = np.random.default_rng(rate)
    out = []
    for n in lengths(rate):
        shaped = n == long_length(rate)
        out.append(signal(rng, 1, n, shaped))
        out.append(signal(rng, 2, n, shaped))
    out.append(signal(rng, 6, long_length(rate), True))
    out.append(signal(rng, 1, 5 * lm.step_of(rate), amplitude=TAIL))             # blocks, none above the absolute gate
    twins = [(len(out) - 3, len(out)), (2 * lengths(rate).index(5 * lm.step_of(rate)), len(out) + 1)]
    out += [out[a].copy() for a, _ in twins]
    return out, twins


@functools.lru_cache(maxsize=None)
def model(rate):
    """per group of groups(rate): dict of z, Sb, peak, n_blocks, n_abs, rel, gated, energy -- the K-weighting runs once over
    all rows"""
    gs, _ = groups(rate)
    X = np.zeros((sum(g.shape[0] for g in gs), max(g.shape[1] for g in gs)), np.float32)
    at = 0
    for g in gs:
        X[at:at + g.shape[0], :g.shape[1]] = g
        at += g.shape[0]
    S = lm.subblock_sums(X, rate)
    res, at = [], 0
    for g in gs:
        rows, valid = g.shape
        z, Sb = lm.block_energies(S[at:at + rows], valid, rate, WEIGHTS)
        at += rows
        n_abs, rel, gated, energy = lm.gate(z)
        res.append(dict(z=z, Sb=Sb, peak=np.float32(np.abs(g).max()) if g.size else np.float32(0), n_blocks=len(z), n_abs=n_abs, rel=rel,
                        gated=gated, energy=energy))
    return res
