"""A float64 model of the Vorbis transform stage (afg_vorbis_transform_hip), its input set and a per-sample error scale.

`transform64` restates in numpy what the stage computes for one batch, in the plane layout of oraclelib.vorbis_transform
(the offsets come from oraclelib.vorbis_layout, so the model, the oracle and the device write one layout):

    inverse MDCT   y[m] = sum_k X[k] cos(pi/(2n) (2m + 1 + n/2)(2k + 1)), the textbook sum, evaluated in complex128 as one
                   zero-padded 2n-point numpy.fft.ifft with a post-twiddle: with a = 2m + 1 + n/2 the angle is
                   2 pi a (2k + 1) / (4n), so y[m] = Re(e^(i pi a / 2n) * F[a mod 2n]), F the unnormalised inverse DFT.
                   Neither stb_vorbis' passes nor the walk's factorisation (tests/vorbis_walk_model.py) enter; `imdct_matrix`
                   is the same sum as a cosine matrix, which tests/test_vorbis_model.py holds the FFT form against.
    window         sin(pi/2 sin^2(pi (i + 1/2) / n)) from the formula in float64 -- not the float32 table of
                   oraclelib.vorbis_tables widened: the model states what the stage is meant to compute, and a table entry
                   differs from the formula by at most 1/2 ulp of float32 (plus the table's float32 pi, a few 2^-24 in the
                   angle).  That difference is part of the oracle's own rounding, so it is inside R by construction: a tap
                   rounds by 2^-25 relative, a sample is a sum of products of lines and taps, so the share is at most
                   2^-25 * sum |line| = scale / 4 per contributing packet.
    overlap-add    the window bounds by packet flags (left start / end, right start / end; long blocks next to short ones
                   through VORBIS_PREV / VORBIS_NEXT), the carried right half, channel interleave; the first packet of a
                   stream emits nothing.

`block_scale` is the error scale of an output block (packet p, channel c): 2^-24 * (L[p][c] + L[p-1][c]), L the sum of
|line| over the packet's spectrum for that channel -- the samples a packet emits depend on its own spectrum and the one
before and on nothing else.  A channel whose two spectra are all zero has scale 0 and must come out as exact zeros.

Measured on the CPU (tests/test_vorbis_model.py prints them):
    R, the largest |oracle32 - model64| / scale over the input set:          6.86
    (per case: flat 1.52, onehot 6.86, windows 1.32, silent_channel 1.30, nz_eighths 1.67, levels 1.05; by block size:
    1024 4.97, 2048 6.47, 4096 6.86, short blocks 1.52.  A one-hot packet's error is the rounding of the oracle's float32
    twiddles and passes as a share of one line; over a flat packet the same errors add up as a random walk while the scale
    adds the lines up in magnitude.)
    smallest relative perturbation that leaves the bound 4 * R * scale (one-hot case): line 64 of the long blocks 2^-18,
    window tap n/4 + 5 of the long blocks 2^-17
The device tests bound every sample by 4 * R * scale with R recomputed from the oracle at run time.

The keyword switches of `transform64` (MUTANTS) each make the model wrong in one place; the bound has to catch every one.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import oraclelib
from afgpu import VORBIS_LONG, VORBIS_NEXT, VORBIS_NZ_EIGHTHS, VORBIS_PREV, synthetic

F32 = np.float32
FULL = VORBIS_LONG | VORBIS_PREV | VORBIS_NEXT

# (channels, blocksize_0, blocksize_1): the head of SHAPES in tests/test_vorbis_walk_gpu.py and one group of more than two
# channels per packing (3: a wavefront per channel; 4 and 6: a wavefront per pair of channels)
TRIPLES = ((1, 256, 1024), (2, 256, 1024), (1, 256, 2048), (2, 256, 2048), (1, 512, 4096), (2, 512, 4096),
           (3, 256, 1024), (4, 256, 2048), (6, 256, 2048))

MUTANT_BIN = 64                 # the line `bin_gain` scales in every long block
CROSS_PACKET = 3                # the packet of every stream in which `cross_channels` swaps channels 0 and 1
NEIGHBOUR_PACKET = 2            # the packet of every stream in which `neighbour_sample` repeats a sample
NEIGHBOUR_SAMPLE = 17

# keyword -> value that switches the mutant on
MUTANTS = {
    "prev_late": True,                  # the carried right half (previous window) read one sample late
    "swap_halves_by_short": True,       # rising and falling window halves swapped where a long block meets a short one
    "drop_overlap_every": 5,            # the overlap lost in packet k, 2k, ... (a segment's first, "redo the packet before")
    "cross_channels": True,             # channels 0 and 1 crossed in packet CROSS_PACKET
    "neighbour_sample": True,           # sample NEIGHBOUR_SAMPLE of channel 0 of packet NEIGHBOUR_PACKET replaced by the next
    "bin_gain": 1 + 2.0 ** -10,         # one twiddle: line MUTANT_BIN's contribution to every long block scaled
    "tap_gain": 1 + 2.0 ** -10,         # one window tap (n/4 + 5 of the long window) scaled
    "flip_second_half": True,           # the sign convention of the second half of the block flipped
}


# ------------------------------------------------------------------------------------------------------- the stage ---
def window64(n):
    """The n/2 rising taps of the Vorbis window of an n-sample block."""
    i = np.arange(n // 2)
    return np.sin(0.5 * np.pi * np.sin(np.pi * (i + 0.5) / n) ** 2)


@lru_cache(maxsize=None)
def _post_twiddle(n):
    a = 2 * np.arange(n) + 1 + n // 2
    return a % (2 * n), np.exp(1j * np.pi * a / (2 * n))


def imdct64(X):
    """X[..., n/2] -> y[..., n], y[m] = sum_k X[k] cos(pi/(2n) (2m + 1 + n/2)(2k + 1))."""
    n = 2 * X.shape[-1]
    F = np.fft.ifft(X.astype(np.complex128), 2 * n, axis=-1) * (2 * n)
    index, phase = _post_twiddle(n)
    return (F[..., index] * phase).real


@lru_cache(maxsize=None)
def imdct_matrix(n):
    """The same sum as a matrix [n, n/2] (for checking imdct64; 4096 takes 64 MB)."""
    m = np.arange(n)[:, None]
    k = np.arange(n // 2)[None, :]
    return np.cos(np.pi / (2 * n) * (2 * m + 1 + n // 2) * (2 * k + 1))


def window_bounds(bs0, bs1, flag):
    """(n, left start, left end, right start, right end) of a packet."""
    is_long = bool(flag & VORBIS_LONG)
    n = bs1 if is_long else bs0
    if is_long and not flag & VORBIS_PREV:
        ls, le = (n - bs0) >> 2, (n + bs0) >> 2
    else:
        ls, le = 0, n >> 1
    if is_long and not flag & VORBIS_NEXT:
        rs, re = (3 * n - bs0) >> 2, (3 * n + bs0) >> 2
    else:
        rs, re = n >> 1, n
    return n, ls, le, rs, re


Packet = namedtuple("Packet", "index stream p channels bs0 bs1 flag n ls le rs re spec_off out_off block")
Packet.__doc__ = """One packet of a batch: `index` in the batch, `p` in its stream, `block` its first (packet, channel) block."""


def walk(packets, channels, bs0, bs1, pflags):
    """The packets of a batch in order, and the totals (spec floats, out floats, blocks)."""
    so, oo, spec_total, out_total = oraclelib.vorbis_layout(packets, channels, bs0, bs1, pflags)
    out, idx, blk = [], 0, 0
    for s, npk in enumerate(map(int, packets)):
        for p in range(npk):
            f = int(pflags[idx])
            out.append(Packet(idx, s, p, int(channels[s]), int(bs0[s]), int(bs1[s]), f,
                              *window_bounds(int(bs0[s]), int(bs1[s]), f), int(so[idx]), int(oo[idx]), blk))
            idx += 1
            blk += int(channels[s])
    return out, int(spec_total), int(out_total), blk


def transform64(packets, channels, bs0, bs1, pflags, spec, **mutant):
    """What afg_vorbis_transform_hip computes, in float64: float64 [out floats] in the layout of oraclelib.vorbis_transform
    (per emitting packet: frame, channel).  Keywords: see MUTANTS."""
    unknown = set(mutant) - set(MUTANTS)
    assert not unknown, unknown
    pkts, spec_total, out_total, _ = walk(packets, channels, bs0, bs1, pflags)
    spec = np.asarray(spec, F32)
    assert spec.size == spec_total
    out = np.zeros(out_total)
    prevw, before = None, None
    for k in pkts:
        if k.p == 0:
            prevw, before = None, None
        C, n, is_long = k.channels, k.n, bool(k.flag & VORBIS_LONG)
        X = spec[k.spec_off:k.spec_off + C * (n // 2)].reshape(C, n // 2).astype(np.float64)
        if "bin_gain" in mutant and is_long:
            X[:, MUTANT_BIN] *= mutant["bin_gain"]
        y = imdct64(X)
        if mutant.get("flip_second_half"):
            y[:, n // 2:] *= -1.0
        if mutant.get("cross_channels") and k.p == CROSS_PACKET and C >= 2:
            y[[0, 1]] = y[[1, 0]]
        if prevw is not None:
            pn = prevw.shape[1]
            w = window64(2 * pn)
            if "tap_gain" in mutant and 2 * pn == k.bs1:
                w[pn // 2 + 5] *= mutant["tap_gain"]
            rising, falling, pw = w, w[::-1], prevw
            if mutant.get("prev_late"):
                pw = np.concatenate([pw[:, 1:], pw[:, -1:]], axis=1)
            if "drop_overlap_every" in mutant and k.p % mutant["drop_overlap_every"] == 0:
                pw = np.zeros_like(pw)
            meets_short = (is_long and not k.flag & VORBIS_PREV) or (before & VORBIS_LONG and not before & VORBIS_NEXT)
            if mutant.get("swap_halves_by_short") and meets_short:
                rising, falling = falling, rising
            y[:, k.ls:k.ls + pn] = y[:, k.ls:k.ls + pn] * rising + pw * falling
            frames = y[:, k.ls:k.rs]
            if mutant.get("neighbour_sample") and k.p == NEIGHBOUR_PACKET:
                frames = frames.copy()
                frames[0, NEIGHBOUR_SAMPLE] = frames[0, NEIGHBOUR_SAMPLE + 1]
            out[k.out_off:k.out_off + frames.size] = frames.T.reshape(-1)
        prevw, before = y[:, k.rs:k.re].copy(), k.flag
    return out


# --------------------------------------------------------------------------------------------------- the error scale ---
def block_scale(spec, packets, channels, bs0, bs1, pflags):
    """float64 [blocks]: 2^-24 * (L[p][c] + L[p-1][c]) of block (packet p, channel c), L = sum |line| of a packet's channel."""
    pkts, _, _, nblocks = walk(packets, channels, bs0, bs1, pflags)
    spec = np.asarray(spec, F32)
    out = np.zeros(nblocks)
    last = None
    for k in pkts:
        C, n2 = k.channels, k.n // 2
        L = np.abs(spec[k.spec_off:k.spec_off + C * n2].reshape(C, n2).astype(np.float64)).sum(1)
        out[k.block:k.block + C] = L if k.p == 0 else L + last
        last = L
    return out * 2.0 ** -24


def sample_blocks(packets, channels, bs0, bs1, pflags):
    """int64 [out floats]: the block (packet, channel) that emits every float of the PCM plane."""
    pkts, _, out_total, _ = walk(packets, channels, bs0, bs1, pflags)
    out = np.full(out_total, -1, np.int64)
    for k in pkts:
        if k.p:
            frames = k.rs - k.ls
            out[k.out_off:k.out_off + frames * k.channels] = np.tile(k.block + np.arange(k.channels), frames)
    assert (out >= 0).all(), "the layout leaves holes"
    return out


def per_sample(block_values, packets, channels, bs0, bs1, pflags):
    """Spread one value per block (packet, channel) over that block's samples in the PCM layout: [out floats]."""
    return np.asarray(block_values)[sample_blocks(packets, channels, bs0, bs1, pflags)]


def block_info(case):
    """Per block of a case: (stream, packet in the stream, channel, flag byte) as four arrays."""
    pkts, _, _, _ = walk(case.packets, case.channels, case.bs0, case.bs1, case.pflags)
    rows = [(k.stream, k.p, c, k.flag) for k in pkts for c in range(k.channels)]
    return tuple(np.array(col) for col in zip(*rows))


# ------------------------------------------------------------------------------------------------------ the input set ---
Case = namedtuple("Case", "name packets channels bs0 bs1 pflags spec declared")
Case.__doc__ = """One batch: `pflags` without AFG_VORBIS_NZ_EIGHTHS; `declared` the same bytes with it (None: nothing to declare)."""


def legal_flags(longs):
    """Flag bytes of a long / short sequence: a long block's PREV / NEXT say whether its neighbours are long."""
    n = len(longs)
    pf = np.zeros(n, np.uint8)
    for p in range(n):
        if longs[p]:
            prev_long = longs[p - 1] if p > 0 else True
            next_long = longs[p + 1] if p + 1 < n else True
            pf[p] = VORBIS_LONG | (VORBIS_PREV if prev_long else 0) | (VORBIS_NEXT if next_long else 0)
    return pf


def _flat(rng, pf, nc, bs0, bs1, amplitude=1.0):
    """Gaussian lines under synthetic.vorbis_floor_curve, one [nc, n/2] array per packet."""
    out = []
    for f in pf:
        n2 = (bs1 if f & VORBIS_LONG else bs0) // 2
        x = rng.standard_normal((nc, n2)).astype(F32) * synthetic.vorbis_floor_curve(n2)
        out.append(x * F32(amplitude))
    return out


def _batch(name, streams, declare=False):
    """streams: list of (channels, bs0, bs1, flag bytes, [spectrum [channels, n/2] per packet]) -> Case."""
    flags = np.concatenate([np.asarray(s[3], np.uint8) for s in streams])
    spec = np.concatenate([x.reshape(-1) for s in streams for x in s[4]]).astype(F32)
    return Case(name, np.array([len(s[3]) for s in streams], np.uint32), np.array([s[0] for s in streams], np.uint8),
                np.array([s[1] for s in streams], np.uint16), np.array([s[2] for s in streams], np.uint16),
                flags & np.uint8(0x0f), spec, flags if declare else None)


def _mixed_flags(rng, npk):
    """synthetic.vorbis_packet_flags at p_short_run 0.2, drawn again until at least half the packets are long blocks and
    one is short: every stream then meets the walk's long-block path and its window changes."""
    while True:
        pf = synthetic.vorbis_packet_flags(rng, npk, p_short_run=0.2)
        longs = int(((pf & VORBIS_LONG) != 0).sum())
        if npk // 2 <= longs < npk:
            return pf


def _packets_for(nc, bs1, budget=25000):
    """8 to 24 packets, about `budget` output floats per stream."""
    return max(8, min(24, budget // (nc * bs1 // 2)))


def _flat_case(seed):
    streams = []
    for i, (nc, bs0, bs1) in enumerate(TRIPLES):
        rng = np.random.default_rng([seed, 1, i])
        pf = _mixed_flags(rng, _packets_for(nc, bs1))
        streams.append((nc, bs0, bs1, pf, _flat(rng, pf, nc, bs0, bs1)))
    # 130 long packets: two refills of the walk's 64-packet flag register
    rng = np.random.default_rng([seed, 1, 99])
    pf = np.full(130, FULL, np.uint8)
    streams.append((2, 256, 2048, pf, _flat(rng, pf, 2, 256, 2048)))
    return _batch("flat", streams)


def fft_point(n, line):
    """(lane group j, register index r) of the walk's FFT input point that line `line` of an n-sample block feeds: the
    point q holds X[2q] + i X[n/2 - 1 - 2q] (vorbis_walk_model.pretwiddle) and sits in register r = q // 64 of the lanes
    whose group_of is q % 64."""
    q = line // 2 if line % 2 == 0 else (n // 2 - 1 - line) // 2
    return q % 64, q // 64


def onehot_lines(n, count, rng):
    """`count` distinct lines of an n-sample block: the edges of the walk's index map, then one even line per lane group
    chosen so that every register index occurs too, then a seeded draw of the rest."""
    R = n // 256
    first = [0, 1, 63, 64, 65, n // 4 - 1, n // 4, n // 2 - 2, n // 2 - 1] + [2 * (j + 64 * (j % R)) for j in range(64)]
    lines = list(dict.fromkeys(first))
    assert count >= len(lines), (n, count, len(lines))
    rest = np.setdiff1d(np.arange(n // 2), lines)
    return lines + [int(v) for v in rng.permutation(rest)[:count - len(lines)]]


ONEHOT_PACKETS = {1024: 16, 2048: 8, 4096: 24}


def _onehot_case(seed):
    streams = []
    for bs1, npk in ONEHOT_PACKETS.items():
        shapes = [t for t in TRIPLES if t[2] == bs1]
        rng = np.random.default_rng([seed, 2, bs1])
        lines = iter(onehot_lines(bs1, npk * sum(t[0] for t in shapes), rng))
        for nc, bs0, _ in shapes:
            xs = []
            for _ in range(npk):
                x = np.zeros((nc, bs1 // 2), F32)
                for c in range(nc):
                    x[c, next(lines)] = 1.0
                xs.append(x)
            streams.append((nc, bs0, bs1, np.full(npk, FULL, np.uint8), xs))
    return _batch("onehot", streams)


L_, S_ = True, False
WINDOW_SEQUENCES = ([L_, L_, L_, L_], [S_, L_, L_, S_], [L_, S_, L_, S_, L_], [S_, S_, L_, S_, S_],
                    [L_, L_, S_, S_, S_, L_, L_], [S_] * 6, [L_], [S_])


def _windows_case(seed):
    streams = []
    for i, (nc, bs0, bs1) in enumerate(TRIPLES):
        rng = np.random.default_rng([seed, 3, i])
        for seq in WINDOW_SEQUENCES:
            pf = legal_flags(seq)
            streams.append((nc, bs0, bs1, pf, _flat(rng, pf, nc, bs0, bs1)))
    return _batch("windows", streams)


def silent_channels(nc):
    """The silent channel of each stream of a shape: for even counts the second of a packed pair in one stream and the
    first of a pair in another."""
    if nc % 2:
        return [nc // 2]
    return [nc - 1, nc - 2] if nc == 2 else [1, nc - 2]


def _silent_case(seed):
    streams = []
    for i, (nc, bs0, bs1) in enumerate(TRIPLES):
        for j, dead in enumerate(silent_channels(nc)):
            rng = np.random.default_rng([seed, 4, i, j])
            pf = _mixed_flags(rng, 8)
            xs = _flat(rng, pf, nc, bs0, bs1)
            for x in xs:
                x[dead] = 0.0
            streams.append((nc, bs0, bs1, pf, xs))
    return _batch("silent_channel", streams)


NZ_EIGHTHS = (8, 6, 3, 1, 0, 3, 0, 1, 6, 8)


def _nz_case(seed):
    streams = []
    for i, (nc, bs0, bs1) in enumerate(TRIPLES):
        rng = np.random.default_rng([seed, 5, i])
        pf = np.full(len(NZ_EIGHTHS), FULL, np.uint8)
        xs = _flat(rng, pf, nc, bs0, bs1)
        # flat, not under the floor curve's cut at 16 kHz: the last declared eighth carries lines up to its end
        xs = [rng.standard_normal(x.shape).astype(F32) * F32(synthetic.VORBIS_LEVEL * 0.1) + x for x in xs]
        order = np.roll(NZ_EIGHTHS, i)
        for x, e in zip(xs, order):
            x[:, bs1 // 16 * int(e):] = 0.0
        declared = np.array([FULL | VORBIS_NZ_EIGHTHS(int(e)) for e in order], np.uint8)
        streams.append((nc, bs0, bs1, declared, xs))
    return _batch("nz_eighths", streams, declare=True)


LEVELS = (2.0 ** -20, 30.0)


def _levels_case(seed):
    streams = []
    for i, (nc, bs0, bs1) in enumerate(TRIPLES):
        for j, amp in enumerate(LEVELS):
            rng = np.random.default_rng([seed, 6, i, j])
            pf = _mixed_flags(rng, 8)
            streams.append((nc, bs0, bs1, pf, _flat(rng, pf, nc, bs0, bs1, amp)))
    return _batch("levels", streams)


def cases(seed=2024):
    """The input set: six batches, deterministic in `seed`, each with one or more streams of every triple of TRIPLES.

    flat            Gaussian lines under synthetic.vorbis_floor_curve, long and short blocks in every stream (p_short_run 0.2), 8 to 24 packets
                    a stream, and one stereo stream of 130 long packets (two refills of the walk's flag register)
    onehot          long packets with full overlap, one line of amplitude 1 per channel, another line in every channel:
                    onehot_lines
    windows         flat spectra over WINDOW_SEQUENCES: every PREV / NEXT combination at both ends of a stream
    silent_channel  flat, one channel of every stream all zeros: silent_channels
    nz_eighths      long packets zeroed above 0, 1, 3, 6 or 8 eighths, varying from packet to packet; `declared` carries
                    AFG_VORBIS_NZ_EIGHTHS
    levels          flat at 2^-20 and at 30 times the programme level, one stream each per triple
    """
    return [_flat_case(seed), _onehot_case(seed), _windows_case(seed), _silent_case(seed), _nz_case(seed), _levels_case(seed)]


# ------------------------------------------------------------------------------------------------------ the reference ---
Reference = namedtuple("Reference", "case oracle32 model64 scale block ratio")
Reference.__doc__ = """Per case: the oracle's float32 PCM, the model's float64 PCM, the per-sample scale, the block of every
sample and, per block, the largest |oracle32 - model64| / scale (0 where the scale is 0)."""


def args(case, declared=False):
    """The arguments of oraclelib.vorbis_transform / transform64 up to the flags."""
    return case.packets, case.channels, case.bs0, case.bs1, case.declared if declared else case.pflags


def ratio_per_packet(got, ref, units=1.0):
    """Per block (packet, channel) of ref.case: max over its samples of |got - model64| / (units * scale); blocks of zero
    scale give 0 if they are exactly zero and inf if not; blocks that emit nothing (a stream's first packet) give 0."""
    err = np.abs(np.asarray(got, np.float64) - ref.model64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.scale > 0, err / (units * ref.scale), np.where(err == 0, 0.0, np.inf))
    out = np.zeros(ref.ratio.size if ref.ratio is not None else int(ref.block.max()) + 1)
    np.maximum.at(out, ref.block, r)
    return out


def measure(cases, oracle):
    """(references, R): `oracle` is oraclelib.vorbis_transform.  R is the float32 reference's own rounding in units of the
    scale, the largest ratio over every block of every case."""
    refs = []
    for c in cases:
        a = args(c)
        so, oo, _, out_total = oraclelib.vorbis_layout(*a)
        o = oracle(*a, so, oo, c.spec, out_total)
        m = transform64(*a, c.spec)
        blocks = block_scale(c.spec, *a)
        ref = Reference(c, o, m, per_sample(blocks, *a), sample_blocks(*a), np.zeros(blocks.size))
        refs.append(ref._replace(ratio=ratio_per_packet(o, ref)))
    return refs, max(float(r.ratio.max()) for r in refs)
