"""tests/loudness_model.py against what is known from outside it: the K-weighting table of ITU-R BS.1770, the standard's
997 Hz conformance figure, EBU Tech 3341's first case, both gates at work on a file with a quiet passage and a tail -- and,
for every group the device tests use (tests/loudness_fixtures.py), that no block lies close enough to a threshold for the
device's gate decisions to be allowed to differ.  No device, no library."""
import math

import numpy as np
import pytest

import filter_model as fm
import loudness_fixtures as lf
import loudness_model as lm


def integrated(x, samplerate, weights=None):
    """the integrated loudness of x [rows, frames] through the chunked K-weighting in float64"""
    x = np.atleast_2d(x)
    step = lm.step_of(samplerate)
    v = lm.kweighted(x, samplerate)
    n = x.shape[1] // step
    S = (v[:, :n * step] ** 2).reshape(x.shape[0], n, step).sum(axis=2)
    z, _ = lm.block_energies(S, x.shape[1], samplerate, weights)
    return lm.lufs(float(lm.gate(z)[3]))


def test_the_design_reproduces_the_standards_table_at_48_khz():
    for got, want in zip(lm.kweight(48000), lm.BS1770_48K):
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)
    for rate in (8000, 11025, 16000, 44100, 48000, 192000):
        assert all(fm.stable(sec) for sec in lm.kweight(rate)), rate


def test_blocks_follow_libebur128s_rounding():
    assert [lm.step_of(r) for r in (8000, 11025, 16000, 22050, 44100, 48000)] == [800, 1103, 1600, 2205, 4410, 4800]
    assert [lm.blocks_of(n, 800) for n in (0, 3199, 3200, 3999, 4000, 4001)] == [0, 0, 1, 1, 2, 2]
    assert abs(lm.GAMMA_ABS / 10.0 ** -6.9309 - 1.0) < 1e-14 and lm.lufs(0.0) == -math.inf and abs(lm.lufs(1.0) + 0.691) < 1e-15


def test_the_chunked_weighting_is_the_sequential_one():
    x = np.random.default_rng(3).uniform(-1.0, 1.0, (2, 5000)).astype(np.float32)
    want = fm.run(lm.kweight(16000), x)[-1]
    assert np.abs(lm.kweighted(x, 16000, chunk=512) - want.astype(np.float64)).max() <= 1e-11
    # in the wide type, what the device is held to: the interval counts K_L = 64 units of the filter bound, the model uses
    # less than a sixteenth of one
    for rate in (8000, 44100):
        want = fm.run(lm.kweight(rate), x)[-1]
        assert float(np.abs(lm.kweighted(x, rate, lm.WIDE) - want).max()) <= lm.filter_bound(rate) * float(np.abs(x).max()) / 16.0


def test_a_full_scale_997_hz_sine_reads_minus_3_01_lkfs():
    n = np.arange(3 * 48000)
    x = np.sin(2.0 * np.pi * 997.0 * n / 48000.0).astype(np.float32)
    got = integrated(x, 48000)
    print(f"997 Hz, 0 dBFS, mono, 48 kHz: {got:.4f} LKFS")
    assert abs(got + 3.01) <= 0.01


def test_ebu_tech_3341_case_1():
    n = np.arange(20 * 48000)
    tone = (10.0 ** (-23.0 / 20.0) * np.sin(2.0 * np.pi * 1000.0 * n / 48000.0)).astype(np.float32)
    got = integrated(np.stack([tone, tone]), 48000)
    print(f"1 kHz, -23 dBFS, stereo, 20 s: {got:.4f} LUFS")
    assert abs(got + 23.0) <= 0.1


def test_a_quiet_passage_and_a_tail_fall_to_the_two_gates():
    gs, _ = lf.groups(8000)
    k = 2 * lf.lengths(8000).index(lf.long_length(8000))        # the mono group with the loud part, the passage and the tail
    m = lf.model(8000)[k]
    assert m["n_blocks"] == lm.blocks_of(gs[k].shape[1], 800) and 0 < m["n_abs"] < m["n_blocks"]
    n_gated = int(m["gated"].sum())
    assert 0 < n_gated < m["n_abs"], "no block fell to the relative gate"
    z = m["z"].astype(np.float64)
    assert (z[~m["gated"]] <= max(lm.GAMMA_ABS, float(m["rel"]))).all() and (z[m["gated"]] > float(m["rel"])).all()
    # gating matters: the ungated mean lies well below the gated one
    assert lm.lufs(float(z.mean())) < lm.lufs(float(m["energy"])) - 1.0
    # ... and the gain to -23 LUFS brings the gated energy there
    g, flags = lm.gain_of(float(m["energy"]), m["peak"])
    assert flags == 0 and abs(lm.lufs(float(m["energy"]) * float(g) ** 2) + 23.0) < 1e-5
    assert lm.gain_of(0.0, 0.5) == (np.float32(1.0), lm.UNGATED)
    assert lm.gain_of(1e-3, 0.5, max_gain=2.0) == (np.float32(2.0), lm.GAIN_CLAMPED)
    assert lm.gain_of(1e-3, 0.5, max_peak=0.25) == (np.float32(0.5), lm.PEAK_CLAMPED)


@pytest.mark.parametrize("rate", lf.RATES)
def test_no_gate_decision_of_the_device_fixtures_is_close(rate):
    """|z_j / Gamma - 1| >= 1e-6 for both gates and every block of every group: the condition under which the device tests
    demand the model's gate sets, no block left out"""
    gs, twins = lf.groups(rate)
    ms = lf.model(rate)
    least, seen = math.inf, set()
    for g, m in zip(gs, ms):
        assert m["n_blocks"] == lm.blocks_of(g.shape[1], lm.step_of(rate))
        least = min(least, lm.gate_margin(m["z"]))
        seen.add((m["n_blocks"] > 0, m["n_abs"] > 0, m["n_abs"] < m["n_blocks"], int(m["gated"].sum()) < m["n_abs"]))
    print(f"{rate} Hz: {len(gs)} groups, least gate margin {least:.3g}")
    assert least >= 1e-6
    # the fixtures hold a group without blocks, one with none above the absolute gate, and one that loses blocks to each gate
    assert (False, False, False, False) in seen and (True, False, True, False) in seen and (True, True, True, True) in seen
    for a, b in twins:
        assert (gs[a].view(np.uint32) == gs[b].view(np.uint32)).all()
