"""Pins tests/vorbis_model.py -- the float64 model of the Vorbis transform stage, its input set and its error scale -- on the
CPU, and proves that the bound the device tests use (tests/test_vorbis_fullband_gpu.py) can fail.

    R       = max over every block of the input set of |oracle32 - model64| / scale: the float32 reference's own rounding
    bound   = |got - model64| <= 4 * R * scale for every sample, R recomputed here from the oracle, never from a device

Every mutant of vorbis_model.MUTANTS, rounded to float32, has to leave that bound in at least one block.

Measured (CPU) (printed by the tests, run with -s): R = 6.86 (flat 1.52, onehot 6.86, windows 1.32, silent_channel 1.30,
nz_eighths 1.67, levels 1.05: 0.90 at 2^-20 and 1.05 at 30 times the programme level; by block size 1024 4.97, 2048 6.47,
4096 6.86, short blocks 1.52); flat spectra decode to a PCM rms of 0.051; the smallest relative perturbation the bound still
catches is 2^-18 for one line (64) and 2^-17 for one window tap (n/4 + 5) of the long blocks.

Today's whole-output RMS check (`check` of tests/test_vorbis_walk_gpu.py, imported, on the `flat` case): it stops all
eight mutants at the sizes of MUTANTS, the one-sample neighbour (rms 5.4e-5, ten samples of 434 k) and the 2^-10 line and tap
(rms 3.5e-6 and 1.4e-6) among them, the last two by its clause rms <= 1e-6 * max(signal rms, 1) alone.  What it lets through:
one line scaled by 1 + 2^-12 (rms 9.0e-7) and one tap by 1 + 2^-11 (rms 7.2e-7), which the per-sample bound stops on the same
case, 2.6 and 20 times over, and on the one-hot case down to 2^-18 and 2^-17."""
import numpy as np
import pytest

import oraclelib
import vorbis_model
import vorbis_walk_model
from afgpu import VORBIS_LONG, VORBIS_NEXT, VORBIS_PREV
from test_vorbis_walk_gpu import check

@pytest.fixture(scope="module")
def measured():
    return vorbis_model.measure(vorbis_model.cases(), oraclelib.vorbis_transform)


def ratio(ref, got, R):
    return vorbis_model.ratio_per_packet(got, ref, 4 * R)


def mutant64(case, **mutant):
    return vorbis_model.transform64(*vorbis_model.args(case), case.spec, **mutant)


def where(ref, block):
    stream, packet, channel, flag = (int(col[block]) for col in vorbis_model.block_info(ref.case))
    c = ref.case
    return (f"{c.name}: stream {stream} ({c.channels[stream]} ch, {c.bs0[stream]} / {c.bs1[stream]}), packet {packet}, "
            f"channel {channel}, flags {flag:#04x}")


def test_fft_form_is_the_textbook_sum():
    rng = np.random.default_rng(3)
    for n in (256, 512, 1024, 2048):
        X = rng.standard_normal((3, n // 2))
        want = X @ vorbis_model.imdct_matrix(n).T
        assert np.abs(vorbis_model.imdct64(X) - want).max() <= 1e-12 * n
    # and the window is the oracle's table to float32 rounding and its float32 pi
    for n in (256, 512, 1024, 2048, 4096):
        assert np.abs(vorbis_model.window64(n) - oraclelib.vorbis_tables(n)["window"]).max() <= 2.0 ** -22


def test_model_against_oracle(measured):
    refs, R = measured
    by_size = {}
    for ref in refs:
        c = ref.case
        dead = ref.scale == 0
        assert (ref.oracle32[dead] == 0).all() and (ref.model64[dead] == 0).all(), f"{c.name}: output without input"
        assert np.isfinite(ref.ratio).all(), c.name
        stream, _, _, flag = vorbis_model.block_info(c)
        size = np.where(flag & VORBIS_LONG, c.bs1[stream], 0)
        for n in np.unique(size):
            by_size[int(n)] = max(by_size.get(int(n), 0.0), float(ref.ratio[size == n].max()))
        print(f"{c.name}: {ref.ratio.size} blocks, {ref.oracle32.size} samples, {int(dead.sum())} silent, "
              f"largest |oracle32 - model64| / scale = {ref.ratio.max():.4g}")
    print("per block size (0: short blocks): " + ", ".join(f"{n}: {v:.4g}" for n, v in sorted(by_size.items())))
    print(f"R = {R:.4g}")
    assert np.isfinite(R) and R > 0


def test_float32_rounding_of_the_model_is_inside_the_bound(measured):
    """The control of the mutant test: the unmutated model, rounded to float32, passes."""
    refs, R = measured
    for ref in refs:
        assert ratio(ref, ref.model64.astype(np.float32), R).max() <= 1.0, ref.case.name


@pytest.mark.parametrize("name", sorted(vorbis_model.MUTANTS))
def test_bound_catches_mutant(measured, name):
    refs, R = measured
    worst, at = 0.0, None
    for ref in refs:
        got = mutant64(ref.case, **{name: vorbis_model.MUTANTS[name]}).astype(np.float32)
        r = ratio(ref, got, R)
        if r.max() > worst:
            worst, at = float(r.max()), where(ref, int(r.argmax()))
        print(f"{name}: {ref.case.name}: {int((r > 1).sum())} of {r.size} blocks outside 4 * R * scale, worst {r.max():.4g}")
    print(f"{name}: worst at {at}")
    assert worst > 1.0, f"mutant {name} survives: worst block ({at}) at {worst:.3g} of the bound"


@pytest.mark.parametrize("name", ["bin_gain", "tap_gain"])
def test_smallest_perturbation_caught(measured, name):
    """One line, or one window tap, of the long blocks scaled by 1 + eps: by linearity the mutant is
    model + eps * (response to a gain of 2 less the model)."""
    refs, R = measured
    ref = next(r for r in refs if r.case.name == "onehot")
    resp = mutant64(ref.case, **{name: 2.0}) - ref.model64
    caught = [k for k in range(8, 26) if ratio(ref, (ref.model64 + 2.0 ** -k * resp).astype(np.float32), R).max() > 1.0]
    assert caught == list(range(8, max(caught) + 1))
    print(f"smallest relative perturbation caught, {name}: 2^-{max(caught)}")
    assert max(caught) >= 14, "well below the 2^-10 of MUTANTS"


def test_onehot_reaches_every_lane_group_and_register(measured):
    """Over the one-hot case every lane of the walk's FFT (group_of: lanes 32..63 walk their groups downwards) and every
    register index r < R = n / 256 receives a hot line, for every block size."""
    refs, _ = measured
    c = next(r.case for r in refs if r.case.name == "onehot")
    pkts, _, _, _ = vorbis_model.walk(*vorbis_model.args(c))
    hit = {n: set() for n in (1024, 2048, 4096)}
    listed = {n: set() for n in hit}
    for k in pkts:
        assert k.flag == vorbis_model.FULL
        x = c.spec[k.spec_off:k.spec_off + k.channels * k.n // 2].reshape(k.channels, -1)
        assert ((x != 0).sum(1) == 1).all() and (x.sum(1) == 1).all(), "one line of amplitude 1 per channel"
        lines = np.argmax(x, 1)
        assert len(set(lines)) == k.channels, "a different line in each channel"
        for line in lines:
            hit[k.n].add(vorbis_model.fft_point(k.n, int(line)))
            listed[k.n].add(int(line))
    for n, points in hit.items():
        R = n // 256
        groups = {int(vorbis_walk_model.group_of(np.int64(lane))) for lane in range(64)}
        assert groups == set(range(64))
        assert {j for j, _ in points} == groups, f"{n}: lane groups {sorted(groups - {j for j, _ in points})} never hot"
        assert {r for _, r in points} == set(range(R)), f"{n}: some register index never hot"
        assert {0, 1, 63, 64, 65, n // 4 - 1, n // 4, n // 2 - 2, n // 2 - 1} <= listed[n]
        # fft_point against the lane model: the hot line lands where spectrum_to_lanes / pretwiddle put it
        X = np.zeros(n // 2)
        for line in (1, 64, n // 2 - 2):
            X[:] = 0
            X[line] = 1
            ev, od = vorbis_walk_model.spectrum_to_lanes(X, R)
            t = vorbis_walk_model.pretwiddle(ev, od, R)
            lane, r = (int(v[0]) for v in np.nonzero(t))
            assert (int(vorbis_walk_model.group_of(np.int64(lane))), r) == vorbis_model.fft_point(n, line)


def test_input_properties(measured):
    refs, _ = measured
    by_name = {r.case.name: r for r in refs}
    assert list(by_name) == ["flat", "onehot", "windows", "silent_channel", "nz_eighths", "levels"]
    for ref in refs:
        c = ref.case
        assert set(vorbis_model.TRIPLES) == set(zip(c.channels.tolist(), c.bs0.tolist(), c.bs1.tolist())), c.name
        print(f"{c.name}: {len(c.packets)} streams, {ref.oracle32.size} output samples")
        assert ref.oracle32.size <= 500000
    # flat: 8 to 24 packets and the 130-packet stream; long and short blocks
    c = by_name["flat"].case
    assert sorted(c.packets)[-1] == 130 and all(8 <= p <= 24 for p in sorted(c.packets)[:-1])
    for name in ("flat", "silent_channel", "levels"):
        for k, pf in zip(by_name[name].case.packets, np.split(by_name[name].case.pflags, np.cumsum(by_name[name].case.packets)[:-1])):
            longs = int(((pf & VORBIS_LONG) != 0).sum())
            assert k // 2 <= longs and (longs < k or k == 130), f"{name}: a stream without long or without short blocks"
    # windows: every PREV / NEXT combination on long blocks, and short blocks at both ends of a stream
    c = by_name["windows"].case
    assert {int(f) for f in c.pflags} == {0, VORBIS_LONG, VORBIS_LONG | VORBIS_PREV, VORBIS_LONG | VORBIS_NEXT, vorbis_model.FULL}
    # silent_channel: for even counts the silent channel is the second of a pair in one stream and the first in another
    ref = by_name["silent_channel"]
    c = ref.case
    stream, packet, channel, _ = vorbis_model.block_info(c)
    blocks = vorbis_model.block_scale(c.spec, *vorbis_model.args(c))
    dead = {(int(s), int(ch)) for s, ch, v in zip(stream, channel, blocks) if v == 0}
    for nc in (2, 4, 6):
        parity = {ch % 2 for s, ch in dead if c.channels[s] == nc}
        assert parity == {0, 1}, nc
    assert len(dead) == len(c.packets) and (ref.scale == 0).any()
    # nz_eighths: the declared counts, zeros above them, data right below them
    c = by_name["nz_eighths"].case
    eighths = (c.declared >> 4).astype(int) - 1
    assert set(eighths) == {0, 1, 3, 6, 8} and not (c.pflags >> 4).any()
    for k in vorbis_model.walk(*vorbis_model.args(c))[0]:
        x = c.spec[k.spec_off:k.spec_off + k.channels * k.n // 2].reshape(k.channels, -1)
        edge = k.n // 16 * eighths[k.index]
        assert not x[:, edge:].any() and not np.signbit(x[:, edge:]).any()
        assert edge == 0 or x[:, edge - 1].all()
    # levels: relative to the input, both levels sit where flat sits
    ref, flat = by_name["levels"], by_name["flat"]
    stream, _, _, _ = vorbis_model.block_info(ref.case)
    per_level = [float(ref.ratio[stream % 2 == j].max()) for j in range(2)]
    print(f"levels: largest ratio at 2^-20: {per_level[0]:.4g}, at 30: {per_level[1]:.4g}; flat: {flat.ratio.max():.4g}")
    for v in per_level:
        assert 0.5 * flat.ratio.max() <= v <= 2.0 * flat.ratio.max()
    rms = float(np.sqrt(np.mean(flat.oracle32.astype(np.float64) ** 2)))
    print(f"flat: PCM rms {rms:.4g}")
    assert 0.03 <= rms <= 0.1


def test_block_scale_definition():
    packets, channels, bs0, bs1 = [3, 2], [2, 1], [256, 256], [1024, 1024]
    pflags = np.array([0, VORBIS_LONG | VORBIS_NEXT, vorbis_model.FULL, 0, 0], np.uint8)
    sizes = [128, 512, 512, 128, 128]
    spec = np.concatenate([np.arange(2 * 128 + 4 * 512, dtype=np.float32) % 7 - 3, np.arange(256, dtype=np.float32) % 5 - 2])
    a = (packets, channels, bs0, bs1, pflags)
    L, o = [], 0
    for n2, nc in zip(sizes, (2, 2, 2, 1, 1)):
        for _ in range(nc):
            L.append(np.abs(spec[o:o + n2].astype(np.float64)).sum())
            o += n2
    want = np.array([L[0], L[1], L[0] + L[2], L[1] + L[3], L[2] + L[4], L[3] + L[5], L[6], L[6] + L[7]]) * 2.0 ** -24
    assert (vorbis_model.block_scale(spec, *a) == want).all()
    # short -> long (no PREV) emits frames (bs1 - bs0) / 4 .. bs1 / 2, 320 of them, long -> long 512, short -> short 128
    s = vorbis_model.per_sample(want, *a)
    assert s.size == 2 * (320 + 512) + 128
    assert (s[:640].reshape(320, 2) == want[2:4]).all() and (s[640:1664].reshape(512, 2) == want[4:6]).all()
    assert (s[1664:] == want[7]).all()


def rms_check(got, want):
    """(passed, text) of today's whole-output check."""
    try:
        rms, _ = check(got, want)
        return True, f"passes check() with an rms error of {rms:.3g}"
    except AssertionError as e:
        return False, f"stopped by check(): {str(e).splitlines()[0]}"


@pytest.mark.parametrize("name", sorted(vorbis_model.MUTANTS))
def test_dilution_of_the_mutants(measured, name):
    """What today's whole-output RMS check makes of MUTANTS on the flat case: it stops every one of them at the size listed
    there, the one-sample neighbour and the 2^-10 line and tap by its second clause, rms <= 1e-6 * max(signal rms, 1)."""
    refs, _ = measured
    ref = next(r for r in refs if r.case.name == "flat")
    passed, text = rms_check(mutant64(ref.case, **{name: vorbis_model.MUTANTS[name]}).astype(np.float32), ref.oracle32)
    print(f"{name}: {text}")
    assert not passed, "MUTANTS at this size used to be stopped by the RMS check; the module docstring says so"


@pytest.mark.parametrize("name,k", [("bin_gain", 12), ("tap_gain", 11)])
def test_dilution_gap(measured, name, k):
    """The gap the per-sample bound closes: the largest power-of-two perturbation of one line, and of one window tap, that
    the whole-output RMS check lets through on the flat case is outside the per-sample bound on that same case."""
    refs, R = measured
    ref = next(r for r in refs if r.case.name == "flat")
    got = mutant64(ref.case, **{name: 1 + 2.0 ** -k}).astype(np.float32)
    passed, text = rms_check(got, ref.oracle32)
    r = ratio(ref, got, R)
    print(f"{name} 1 + 2^-{k}: {text}; {int((r > 1).sum())} of {r.size} blocks outside 4 * R * scale, worst {r.max():.4g}")
    assert passed, "expected to slip through the RMS check"
    assert not rms_check(mutant64(ref.case, **{name: 1 + 2.0 ** -(k - 1)}).astype(np.float32), ref.oracle32)[0]
    assert r.max() > 1.0, where(ref, int(r.argmax()))
