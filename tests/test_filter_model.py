"""tests/filter_model.py against scipy.signal.sosfilt where scipy is installed, and the properties of the coefficient helper's
formulas.  No GPU and no library call."""
import math

import numpy as np
import pytest

import filter_model as fm

FS = 48000.0


def gain(sec, f, fs=FS):
    return abs(fm.response(sec, np.exp(2j * math.pi * f / fs)))


def test_model_matches_scipy_sosfilt():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, (3, 2500)).astype(np.float32)
    for sos in ([fm.design("preemphasis", f0=0.97)],
                [fm.design("highpass", FS, 20.0)],
                [fm.design("highpass", 16000.0, 80.0), fm.design("peaking", 16000.0, 1000.0, 2.0, 6.0), fm.design("lowpass", 16000.0, 7000.0)],
                [fm.design("dc_block", FS, 30.0), fm.design("lowshelf", FS, 200.0, 0.7, -4.0), fm.design("highshelf", FS, 6000.0, 0.7, 3.0)]):
        mine = fm.run(sos, x)[-1].astype(np.float64)
        theirs = signal.sosfilt(np.array([[s[0], s[1], s[2], 1.0, s[3], s[4]] for s in sos]), x.astype(np.float64), axis=-1)
        # float64 against the wide recurrence: within the bound's own measure of a float64 evaluation, five roundings a term
        assert np.abs(mine - theirs).max() <= 5.0 * fm.bound(sos) + 1e-300
        assert all(fm.stable(s) for s in sos)


def test_state_at_reads_the_history():
    sos = [fm.design("highpass", FS, 100.0), fm.design("lowpass", FS, 5000.0)]
    x = np.random.default_rng(4).uniform(-1.0, 1.0, (1, 40)).astype(np.float32)
    sig = fm.run(sos, x)
    st = fm.state_at(sig, 0, 1)
    assert st.shape == (2, 4) and st[0, 0] == x[0, 0] and st[0, 1] == 0 and st[1, 0] == st[0, 2] and st[1, 3] == 0
    st = fm.state_at(sig, 0, 40)
    assert st[0, 0] == x[0, 39] and st[0, 1] == x[0, 38] and st[1, 2] == sig[2][0, 39] and st[1, 3] == sig[2][0, 38]
    assert (fm.state_at(sig, 0, 0) == 0).all()


def test_design_helper_properties():
    for f0 in (20.0, 1000.0, 7000.0, 20000.0):
        hp, lp = fm.design("highpass", FS, f0), fm.design("lowpass", FS, f0)
        assert abs(fm.response(hp, 1.0)) < 1e-9                 # high-pass: nothing at DC
        assert abs(abs(fm.response(lp, 1.0)) - 1.0) < 1e-9      # low-pass: DC unchanged
        assert abs(fm.response(lp, -1.0)) < 1e-9 and abs(abs(fm.response(hp, -1.0)) - 1.0) < 1e-9
        for sec in (hp, lp):                                     # q = 1 / sqrt 2: -3.01 dB at f0
            assert abs(20.0 * math.log10(gain(sec, f0)) + 10.0 * math.log10(2.0)) < 1e-6
        ap = fm.design("allpass", FS, f0, 1.3)
        assert np.abs(np.abs(fm.response(ap, np.exp(1j * np.linspace(0.0, math.pi, 257)))) - 1.0).max() < 1e-9
        for db in (-9.0, 6.0):
            pk = fm.design("peaking", FS, f0, 2.0, db)
            assert abs(20.0 * math.log10(gain(pk, f0)) - db) < 1e-6
            assert abs(abs(fm.response(pk, 1.0)) - 1.0) < 1e-9 and abs(abs(fm.response(pk, -1.0)) - 1.0) < 1e-9
            lo, hi = fm.design("lowshelf", FS, f0, 0.7, db), fm.design("highshelf", FS, f0, 0.7, db)
            assert abs(20.0 * math.log10(abs(fm.response(lo, 1.0))) - db) < 1e-6 and abs(abs(fm.response(lo, -1.0)) - 1.0) < 1e-9
            assert abs(20.0 * math.log10(abs(fm.response(hi, -1.0))) - db) < 1e-6 and abs(abs(fm.response(hi, 1.0)) - 1.0) < 1e-9
        bp, no = fm.design("bandpass", FS, f0, 3.0), fm.design("notch", FS, f0, 3.0)
        assert abs(gain(bp, f0) - 1.0) < 1e-9 and gain(no, f0) < 1e-9
        dc = fm.design("dc_block", FS, f0)
        assert abs(fm.response(dc, 1.0)) == 0.0 and dc[3] == -math.exp(-2.0 * math.pi * f0 / FS) and fm.stable(dc)
        for kind in fm.KINDS[:8]:
            assert fm.stable(fm.design(kind, FS, f0, 0.5, 3.0)), kind
    assert fm.design("preemphasis", f0=0.97) == (1.0, -0.97, 0.0, 0.0, 0.0)


def test_bound_of_simple_cascades():
    # a FIR section: |g|_1 = 1, alpha = 0: E / max|x| = 2^-53 beta
    assert fm.bound([(1.0, -0.97, 0.0, 0.0, 0.0)]) == 1.97 * 2.0 ** -53
    # one pole at r: |g|_1 = 1 / (1 - r), h = g: 2^-53 (1 + r / (1 - r)) / (1 - r)
    r = 0.5
    assert abs(fm.bound([(1.0, 0.0, 0.0, -r, 0.0)]) / (2.0 ** -53 * (1.0 + r / (1.0 - r)) / (1.0 - r)) - 1.0) < 1e-12
    # two FIR sections: beta_1 |h_2|_1 + beta_2 P_1
    assert abs(fm.bound([(2.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 0.0, 0.0)]) / (2.0 ** -53 * (2.0 * 3.0 + 3.0 * 2.0)) - 1.0) < 1e-15
    assert fm.ulp32(1.0) == 2.0 ** -23 and fm.ulp32(0.0) == 2.0 ** -149 and fm.ulp32(1.5) == 2.0 ** -23 and fm.ulp32(2.0 ** -140) == 2.0 ** -149
