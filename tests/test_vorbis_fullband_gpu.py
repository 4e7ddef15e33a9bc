"""Vorbis transform kernels (csrc/vorbis_transform.hip, and csrc/vorbis_walk.hip in the default numeric mode) per sample.

The input set of tests/vorbis_model.py runs every case over nine (channels, blocksize_0, blocksize_1) triples, all of them
shapes the walk takes: flat spectra with long and short blocks, one-hot lines that reach every lane group and register of
the walk's FFT, every window sequence at both ends of a stream, a silent channel beside live ones, declared zero tails that
change from packet to packet, and two far-apart levels.  The exact kernels are compared bit for bit with the oracle; the
default-mode walk is held, sample by sample, to

    |got - model64| <= 4 * R * scale(packet, channel)       scale = 2^-24 * (L[p][c] + L[p-1][c]),  L = sum |line|

where model64 is the float64 model and R the float32 oracle's own distance from it in units of the scale, recomputed from
the oracle on the same inputs at every run and never taken from the device.  tests/test_vorbis_model.py shows on the CPU
that this bound fails for a carried half read one sample late, window halves swapped beside a short block, a lost overlap
at a segment start, crossed channels, one repeated sample, a flipped half, or one line or one window tap off by 2^-10.
The factor 4 is the margin of tests/test_mp3_fullband_gpu.py: four times the float32 reference's distance from the truth.

Measured (CPU): R = 6.86 (flat 1.52, onehot 6.86, windows 1.32, silent_channel 1.30, nz_eighths 1.67, levels 1.05); flat
spectra decode to a PCM rms of 0.051; the smallest relative perturbation the bound still catches is 2^-18 for one line and
2^-17 for one window tap of the long blocks.
Measured (MI355X): largest |got - model64| / (R * scale): exact kernels 1.000 (they are the oracle, bit for bit: flat 0.222,
onehot 1.000, windows 0.193, silent_channel 0.189, nz_eighths 0.244, levels 0.162), default-mode walk 0.392 (flat 0.187,
onehot 0.392 at line 682 of a 4096-sample block, windows 0.175, silent_channel 0.140, nz_eighths 0.136, levels 0.137),
against the 4 the bound allows; outside the one-hot case the largest ratios sit in short blocks (flags 0), in both modes.
80 % to 91 % of the walk's live long-block samples differ from the oracle's bits on every shape.

Every run decodes into the inner view of a PCM plane with 64 sentinel floats on either side (the start stays 16-byte
aligned, so the default mode takes the walk)."""
import numpy as np
import pytest

import oraclelib
import vorbis_model
from afgpu import VORBIS_LONG, VorbisPlan

pytestmark = pytest.mark.gpu

SEGS = (1, 5, 16, 1000)
EXACT_SEGS = (1, 5, 1000)
CASES = ("flat", "onehot", "windows", "silent_channel", "nz_eighths", "levels")
GUARD = 64
SENTINEL = 0x7fa5c3e1          # a NaN no arithmetic produces


@pytest.fixture(scope="module")
def measured():
    refs, R = vorbis_model.measure(vorbis_model.cases(), oraclelib.vorbis_transform)
    return {r.case.name: r for r in refs}, R


def run_guarded(gpu, case, seg, declared=False):
    import torch
    plan = VorbisPlan(*vorbis_model.args(case, declared), seg)
    so, oo, spec_floats, out_floats = oraclelib.vorbis_layout(*vorbis_model.args(case))
    pso, poo = plan.offsets()
    assert plan.out_floats == out_floats and plan.spec_floats == spec_floats and (pso == so).all() and (poo == oo).all()
    plane = torch.full((out_floats + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    inner = plane.view(torch.float32)[GUARD:GUARD + out_floats]
    assert inner.data_ptr() % 16 == 0
    plan.transform(torch.from_numpy(case.spec).to(gpu), inner)
    torch.cuda.synchronize()
    host = plane.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all(), "the kernel wrote in front of the PCM plane"
    assert (host[GUARD + out_floats:] == SENTINEL).all(), "the kernel wrote behind the PCM plane"
    pcm = host[GUARD:GUARD + out_floats]
    assert (pcm != SENTINEL).all(), "unwritten PCM"
    return pcm.view(np.float32).copy()


def bits(a):
    return a.view(np.uint32)


def shape_of(case, stream):
    return int(case.channels[stream]), int(case.bs0[stream]), int(case.bs1[stream])


def check_bound(ref, got, R, what):
    """Every sample inside 4 * R * scale, silent blocks exactly zero.  Prints the largest |got - model64| / (R * scale) per
    shape with the place it occurs and returns the largest of all."""
    c = ref.case
    r = vorbis_model.ratio_per_packet(got, ref, R)
    stream, packet, channel, flag = vorbis_model.block_info(c)
    shapes = np.array([vorbis_model.TRIPLES.index(shape_of(c, s)) for s in stream])
    for i, (nc, bs0, bs1) in enumerate(vorbis_model.TRIPLES):
        idx = np.flatnonzero(shapes == i)
        b = idx[int(r[idx].argmax())]
        print(f"{what}: {c.name}: {nc} ch {bs0} / {bs1}: largest |got - model64| / (R * scale) = {r[b]:.4g} at stream {stream[b]}, "
              f"packet {packet[b]} (flags {int(flag[b]):#04x}), channel {channel[b]}")
    worst = int(r.argmax())
    report = (f"{what}: {c.name}: largest |got - model64| / (R * scale) = {r[worst]:.4g} at stream {stream[worst]} "
              f"({'%d ch %d / %d' % shape_of(c, stream[worst])}), packet {packet[worst]} (flags {int(flag[worst]):#04x}), "
              f"channel {channel[worst]}")
    if c.name == "onehot":
        pk = next(k for k in vorbis_model.walk(*vorbis_model.args(c))[0] if k.stream == stream[worst] and k.p == packet[worst])
        x = c.spec[pk.spec_off:pk.spec_off + pk.channels * pk.n // 2].reshape(pk.channels, -1)
        report += f", hot line {int(np.argmax(x[channel[worst]]))}"
    print(report)
    assert (got[ref.scale == 0] == 0).all(), f"{what}: {c.name}: a channel without input is not silent"
    assert r[worst] <= 4.0, report + f"; {int((r > 4).sum())} of {r.size} blocks outside the bound"
    return float(r[worst])


# ------------------------------------------------------------------------------------------------------- exact mode ---
@pytest.mark.parametrize("seg", EXACT_SEGS)
@pytest.mark.parametrize("name", CASES)
def test_exact_mode_is_the_oracle_bit_for_bit(gpu, measured, name, seg):
    refs, R = measured
    ref = refs[name]
    c = ref.case
    for declared in (False,) if c.declared is None else (True, False):
        got = run_guarded(gpu, c, seg, declared)
        nbad = int((bits(got) != bits(ref.oracle32)).sum())
        assert nbad == 0, f"{name}, segments of {seg}: {nbad} samples differ bitwise"
    assert check_bound(ref, got, R, "exact kernel") <= 1.0


# ----------------------------------------------------------------------------------------------------- default mode ---
@pytest.mark.numeric_tolerance
@pytest.mark.parametrize("name", CASES)
def test_default_mode_inside_the_bound(gpu, measured, name):
    refs, R = measured
    ref = refs[name]
    c = ref.case
    got = run_guarded(gpu, c, SEGS[0])
    check_bound(ref, got, R, "default-mode kernel")
    # the walk is the path taken: on every shape the live samples of long blocks are not the oracle's bits
    stream, _, _, flag = vorbis_model.block_info(c)
    long_live = ((flag & VORBIS_LONG) != 0)[ref.block] & (ref.scale > 0)
    shapes = np.array([vorbis_model.TRIPLES.index(shape_of(c, s)) for s in stream])[ref.block]
    for i, (nc, bs0, bs1) in enumerate(vorbis_model.TRIPLES):
        sel = long_live & (shapes == i)
        if not sel.any():
            assert name == "silent_channel" and nc == 1, f"{name}: no live long block at {nc} ch {bs0} / {bs1}"
            continue
        differ = float((bits(got) != bits(ref.oracle32))[sel].mean())
        print(f"{name}: {nc} ch {bs0} / {bs1}: {differ:.1%} of the live samples of long blocks differ from the oracle's bits")
        assert differ > 0.1, f"{nc} ch {bs0} / {bs1}: the exact kernel ran in the default mode"
    for seg in SEGS[1:]:
        again = run_guarded(gpu, c, seg)
        assert (bits(again) == bits(got)).all(), f"{name}: segments of {seg} changed the samples"
    if c.declared is not None:
        for seg in SEGS[:2]:
            declared = run_guarded(gpu, c, seg, True)
            assert (bits(declared) == bits(got)).all(), f"{name}: declaring the empty eighths changed the samples (segments of {seg})"
