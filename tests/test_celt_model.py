"""Pins tests/celt_model.py -- the float64 model of the CELT transform seam, its input set and its error scale -- on the CPU,
and proves that the bound the device tests use (tests/test_celt_frames_gpu.py) can fail.

    R       = max over every sample of the input set of |oracle32 - model64| / scale: the float32 oracle's own rounding
    bound   = |got - model64| <= 4 * R * scale for every sample, R recomputed here from the oracle, never from a device

Every mutant of celt_model.MUTANTS, rounded to float32, has to leave that bound in at least one sample.  Measured values
(printed by the tests, run with -s):

    R = 15.93, by family and level (programme / native):
        spectrum 15.32 / 15.93 (the one-hot frames: one line is the whole signal and the whole scale; worst at 480 x 1)
        scale 2.83 / 3.11      postfilter 0.646 / 0.610      geometry 0.801 / 0.636      cuts 0.612 / 0.695
    (shaped and flat spectra add up out of phase, so the same rounding is a smaller share of the line sum there)
    smallest relative perturbation of bin block/2 (one-hot frames) still outside 4 * R * scale:  2^-17
"""
import numpy as np
import pytest

import celt_model as cm
import oraclelib

R_RECORDED = 15.93
FAMILIES = ("spectrum", "scale", "postfilter", "geometry", "cuts")


@pytest.fixture(scope="module")
def measured():
    """{(level, case name): (case, model result, oracle output, per-sample ratio)} and R."""
    refs = {}
    for level in cm.LEVELS:
        for c in cm.cases(level):
            res = cm.model_of(c)
            o = oraclelib.celt_transform(c.rec_base, c.recs, c.coeffs, c.total)
            refs[level, c.name] = (c, res, o, cm.ratio(o, res))
    return refs, max(float(r.max()) for _, _, _, r in refs.values())


def test_R_and_its_breakdown(measured):
    refs, R = measured
    for level in cm.LEVELS:
        by_family = {f: max(float(r.max()) for (lv, _), (c, _, _, r) in refs.items() if lv == level and c.family == f)
                     for f in FAMILIES}
        print(level, ", ".join(f"{f} {v:.4g}" for f, v in by_family.items()))
    for (level, name), (c, res, o, r) in refs.items():
        print(f"{level:9s} {name:22s} {len(c.recs):3d} records {c.total:6d} samples, {int((res.scale == 0).sum()):4d} at zero scale, "
              f"largest |oracle32 - model64| / scale = {r.max():.4g}")
    print(f"R = {R:.4g}")
    assert np.isfinite(R)
    assert R_RECORDED / 1.1 <= R <= R_RECORDED * 1.1, "the oracle or the model moved: measure again and record it"


def test_oracle_inside_R_scale_on_every_sample(measured):
    """The condition of the device tests: no sample left out, zero scale means +-0 in the oracle and the model."""
    refs, R = measured
    for key, (c, res, o, r) in refs.items():
        assert res.written.all() and not np.isnan(o).any(), key
        assert (r <= R).all(), key
        dead = res.scale == 0
        assert (o[dead] == 0).all() and (res.out[dead] == 0).all(), key
        assert (res.scale[~dead] >= 2.0 ** -149).all(), key


def test_scale_bounds_the_signal_and_follows_the_level(measured):
    """The envelope is a bound (scale >= 2^-24 |model|) and decays behind a loud frame: one 960-sample frame of zeros after
    a live one ends 2^-149-close to nothing, not on the loud frame's scale."""
    refs, _ = measured
    for key, (c, res, o, r) in refs.items():
        assert (res.scale >= 2.0 ** -24 * np.abs(res.out)).all(), key
    c, res, o, r = refs["programme", "spectrum-960x1"]
    C, first, frames = c.streams[0]
    rec = c.recs[int(c.rec_base[first]):int(c.rec_base[first + 1])]
    loud, quiet = int(rec[0]["out_off"]), int(rec[1]["out_off"])
    assert res.scale[quiet + 959] < 1e-30 * res.scale[loud + 500]


def window120():
    n = np.arange(120)
    return np.sin(0.5 * np.pi * np.sin(0.5 * np.pi * (n + 0.5) / 120) ** 2)


def test_window_tables_are_the_formula_to_float32_accuracy():
    w = window120()
    assert np.abs(cm.WINDOW - w).max() < 1.2e-7                          # eight printed digits: within two float32 units
    assert np.abs(cm.WINDOW2 - w ** 2).max() < 6e-7                      # the squared table is printed to six digits


def test_basis_is_the_direct_sum_of_the_oracle_pin():
    """tests/test_oracle_celt.py::test_imdct15_half_matches_direct_sum, evaluated without angle reduction."""
    for bs in (120, 240, 480, 960):
        m = np.arange(bs)[:, None]; k = np.arange(bs)[None, :]
        assert np.abs(cm.basis(bs) - np.cos(np.pi / bs * (m + bs + 0.5) * (k + 0.5))).max() < 1e-11


@pytest.mark.parametrize("blocks", [1, 8])
def test_tdac_reconstruction_long_and_transient(blocks):
    """Forward MDCT (float64, CELT window) -> model -> inverse de-emphasis: the signal comes back (the construction of
    tests/test_oracle_celt.py::test_tdac_reconstruction_long_and_transient, to float64 accuracy: what is left is the float32
    rounding of the window table, 6e-8 relative)."""
    rng = np.random.default_rng(11)
    size, nfr = 960, 4
    bs = size // blocks
    nblk = nfr * blocks
    sig = rng.standard_normal((nblk + 2) * bs) * 1000
    w = window120()
    pad = (bs - 120) // 2
    win = np.concatenate([np.zeros(pad), w, np.ones(bs - 120), w[::-1], np.zeros(pad)])
    n = np.arange(2 * bs)[:, None]; k = np.arange(bs)[None, :]
    fwd = np.cos(np.pi / bs * (n + 0.5 + bs / 2) * (k + 0.5))
    spec = np.stack([(sig[b * bs:b * bs + 2 * bs] * win) @ fwd * (2.0 / bs) for b in range(nblk)])
    frames = [cm._frame_of(size, blocks, spec[f * blocks:(f + 1) * blocks].T.reshape(1, -1)) for f in range(nfr)]
    c = cm.build("tdac", "tdac", [frames])
    # the model is linear: feed it the float64 spectrum's float32 rounding and allow for that rounding
    y = cm.model_of(c).out * 32768.0
    x = y.copy(); x[1:] -= cm.DEEMPH * y[:-1]
    best = min(range(0, 2 * bs), key=lambda d: np.abs(x[size:3 * size] - sig[size + d:3 * size + d]).max())
    err = np.abs(x[size:3 * size] - sig[size + best:3 * size + best]).max()
    assert err < 5e-3, (blocks, best, err)                               # float32 spectrum: 2^-24 * 1000 * sqrt(bs) lines


def test_model_with_carried_state_equals_one_run(measured):
    """Split at every frame boundary, the state carried: the same float64 values, exactly."""
    refs, _ = measured
    for name in ("pf-change", "pf-on-off-on", "geometry-filtered", "cut-960-reach"):
        c, res, _, _ = refs["programme", name]
        longest = int(np.diff(c.rec_base.astype(np.int64)).max())
        for cut in range(1, longest):
            out = np.zeros(c.total)
            scale = np.zeros(c.total)
            states = None
            for lo, hi in ((0, cut), (cut, longest)):
                rb, rc = cm.select(c, lo, hi)
                part = cm.run(rb, rc, c.coeffs, c.total, states)
                out[part.written], scale[part.written] = part.out[part.written], part.scale[part.written]
                states = part.states
            assert np.array_equal(out, res.out) and np.array_equal(scale, res.scale), (name, cut)


def mutant_ratio(refs, R, level, **mutant):
    worst, where = 0.0, None
    for (lv, name), (c, res, _, _) in refs.items():
        if lv != level:
            continue
        got = cm.model_of(c, **mutant).out.astype(np.float32)
        r = cm.ratio(got, res, 4 * R)
        if r.max() > worst:
            worst, where = float(r.max()), (name, int(r.argmax()))
    return worst, where


def test_float32_rounding_of_the_model_is_inside_the_bound(measured):
    """The control of the mutant test: the unmutated model, rounded to float32, passes."""
    refs, R = measured
    assert mutant_ratio(refs, R, "programme")[0] <= 1.0


@pytest.mark.parametrize("name", sorted(cm.MUTANTS))
def test_bound_catches_mutant(measured, name):
    refs, R = measured
    worst, where = mutant_ratio(refs, R, "programme", **{name: cm.MUTANTS[name]})
    print(f"{name}: worst sample {where} at {worst:.4g} of 4 * R * scale")
    assert worst > 1.0, f"mutant {name} survives: worst sample {where} at {worst:.3g} of the bound"


def test_smallest_bin_perturbation_caught(measured):
    """Bin block/2 scaled by 1 + eps: by linearity the mutant is model + eps * (response to that bin alone)."""
    refs, R = measured
    c, res, _, _ = refs["programme", "spectrum-960x1"]
    resp = cm.model_of(c, bin_gain=2.0).out - res.out
    caught = [k for k in range(8, 30) if cm.ratio((res.out + 2.0 ** -k * resp).astype(np.float32), res, 4 * R).max() > 1.0]
    assert caught == list(range(8, max(caught) + 1))
    print(f"smallest relative perturbation of bin block/2 caught: 2^-{max(caught)}")
    assert max(caught) >= 14


def test_input_properties():
    """What the input set promises, asserted: the edges occur, they do not happen by luck of a seed."""
    cs = {c.name: c for c in cm.cases("programme")}
    assert {c.family for c in cs.values()} == set(FAMILIES)
    # layout: stereo streams on even / odd indices, out_off even and + 1; an empty sequence where one is needed
    empties = 0
    for c in cs.values():
        n = np.diff(c.rec_base.astype(np.int64))
        empties += int((n == 0).sum())
        for C, first, frames in c.streams:
            if C == 2:
                a, b = (c.recs[int(c.rec_base[first + i]):int(c.rec_base[first + i + 1])] for i in (0, 1))
                assert first % 2 == 0 and len(a) == len(b) == len(frames)
                assert (a["out_off"] % 2 == 0).all() and (b["out_off"] == a["out_off"] + 1).all() and (a["out_stride"] == 2).all()
    assert empties > 0
    # spectrum: per geometry the five one-hot bins in every block position, a flat frame, zero frames between live ones
    assert [n for n in cs if n.startswith("spectrum")] == [f"spectrum-{F}x{B}" for F, B in cm.GEOMETRIES]
    for F, B in cm.GEOMETRIES:
        c, bs = cs[f"spectrum-{F}x{B}"], F // B
        hot = set()
        for r in c.recs:
            x = c.coeffs[int(r["coef_off"]):int(r["coef_off"]) + F]
            nz = np.flatnonzero(x)
            if nz.size == 1:
                hot.add(int(nz[0]) // B)
        assert hot == {0, 1, bs // 2 - 1, bs // 2, bs - 1}
        for C, first, frames in c.streams:
            assert len(frames) == 3
        assert any(not f[1]["coef"].any() and f[0]["coef"].any() and f[2]["coef"].any() for _, _, f in c.streams)
        assert any(np.signbit(f[1]["coef"]).all() for _, _, f in c.streams)
    # scale: 0.5 on long and transient frames, 0.5 and 1.0 mixed in one sequence
    r = cs["scale"].recs
    assert ((r["imdct_scale"] == 0.5) & (r["blocks"] == 1)).any() and ((r["imdct_scale"] == 0.5) & (r["blocks"] > 1)).any()
    assert any({f["scale"] for f in frames} == {0.5, 1.0} for _, _, frames in cs["scale"].streams)
    # post-filter
    top = [tuple(cm.GAIN_MAX * cm.TAPS[i]) for i in range(3)]
    assert (cs["pf-period15"].recs["pf_period_new"] == 15).all()
    p = cs["pf-period1022-120"].recs
    assert (p["pf_period_new"] == 1022).all() and (p["frame_size"] == 120).all() and min(len(f) for _, _, f in cs["pf-period1022-120"].streams) >= 10
    near = {(int(x["frame_size"]), int(x["pf_period_new"]) - int(x["frame_size"])) for x in cs["pf-period-near-frame"].recs}
    assert {(F, d) for F in (120, 480, 960) for d in (-2, 0, 2)} <= near
    for _, _, frames in cs["pf-change"].streams:
        assert all(a["period"] != b["period"] and a["gains"][0] and b["gains"][0] for a, b in zip(frames, frames[1:]))
    for _, _, frames in cs["pf-on-off-on"].streams:
        live = [bool(f["gains"][0]) for f in frames]
        assert live[:3] == [True, False, True] and len({f["period"] for f in frames}) == 1
    assert {tuple(x["pf_gains_new"]) for x in cs["pf-tapsets"].recs} == set(top)
    # geometry
    seqs = [[(f["size"], f["blocks"]) for f in frames] for _, _, frames in cs["geometry"].streams]
    assert [(960, 1), (120, 1), (960, 1)] in seqs and [(120, 1), (960, 1), (120, 1)] in seqs
    assert any((240, 2) in s and (960, 1) in s for s in seqs) and any(set(s) == {(120, 1)} for s in seqs)
    # cuts: the shortest idle run allows exactly one cut, at the frame that brings the filter back; one record fewer allows none
    for name, (F, idle, T) in cm.CUT_CASES.items():
        c = cs[name]
        for k in range(len(c.rec_base) - 1):
            seq = c.recs[int(c.rec_base[k]):int(c.rec_base[k + 1])]
            if len(seq) == 0:
                continue
            want = {1 + idle: 2 if F == 960 else 10} if name.startswith("cut") else {}
            assert cm.cut_points(seq) == want, name
            assert int(seq[1 + idle]["pf_period_new"]) == T and seq[1 + idle]["pf_gains_new"][0] != 0


def test_levels(measured):
    refs, _ = measured
    for name in ("spectrum-960x1", "scale", "pf-change", "geometry", "cut-960"):
        lo = float(np.sqrt(np.mean(refs["programme", name][2].astype(np.float64) ** 2)))
        hi = float(np.sqrt(np.mean(refs["native", name][2].astype(np.float64) ** 2)))
        print(f"{name}: oracle PCM rms {lo:.3g} (programme), {hi:.3g} (native)")
        assert 0.05 <= lo <= 0.2 and 1.0 <= hi <= 4.0
