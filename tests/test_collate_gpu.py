"""afg_collate_hip against tests/collate_model.py, bit for bit (uint32 views).  d_out is prefilled with a NaN word and
compared as a whole, so a store outside what a span names shows."""
import numpy as np
import pytest
import torch

import afgpu
import collate_model as cm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

TILE = afgpu.WAV_TILE_SAMPLES
COUNTS = (4095, 4096, 4097, 2 * 4096 + 1)      # tile borders


def launch(spans, d_in, out_floats, in_floats=None):
    """runs the spans (dicts of collate_model.span) over d_in (uint32) on the device; returns (got, want) as uint32"""
    rec = np.zeros(len(spans), afgpu.COLLATE_SPAN_DTYPE)
    for k, sp in enumerate(spans):
        for name, v in sp.items():
            rec[k][name] = v
    tiles = afgpu.collate_layout(rec)
    before = np.full(out_floats, cm.PREFILL, np.uint32)
    d_spans = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
    d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
    try:
        afgpu.collate(len(rec), d_spans, tiles, d_src, len(d_in) if in_floats is None else in_floats, d_out, out_floats)
    finally:
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
    return got, cm.apply_spans(spans, d_in, before)


def words(rng, n):
    """random finite-looking and not so finite words: every bit pattern is fair game, the kernel does no arithmetic"""
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


class Planes:
    """lays runs into one input plane and slabs into one output plane, with gaps of foreign words between them"""

    def __init__(self, rng):
        self.rng, self.in_at, self.out_at, self.spans = rng, 0, 0, []

    def run(self, count, odd_in):
        self.in_at += 3
        if (self.in_at & 1) != odd_in:
            self.in_at += 1
        at = self.in_at
        self.in_at += count
        return at

    def slab(self, floats, phase):
        self.out_at += 5
        while (self.out_at & 3) != phase:
            self.out_at += 1
        at = self.out_at
        self.out_at += floats
        return at

    def check(self):
        d_in = words(self.rng, self.in_at + 8)
        got, want = launch(self.spans, d_in, self.out_at + 8)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:8], [hex(v) for v in got[bad[:8]]], [hex(v) for v in want[bad[:8]]])
        assert (want != cm.PREFILL).any()


@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8, 64, 65, 300])
def test_runs_of_every_shape(gpu, ch):
    """T in 1, 5, 16, 4099 x rows at every 16-byte phase, with the run lengths, the in_off parity, sample0 (mid-frame for more
    than one channel), first_frame (0, inside the run, past its end) and out_channels (below, at, above the file's) cycling.
    64, 65 and 300 channels: the two sides of the kernel's threshold between lanes over frames and lanes over rows, and more
    rows than a workgroup has lanes; a tile holds few frames of such a file, so the long row is 131 there."""
    rng = np.random.default_rng(100 + ch)
    pl = Planes(rng)
    n = 0
    for T in (1, 5, 16, 4099 if ch <= 8 else 131):
        for phase in range(4):
            for rep in range(3):
                count = COUNTS[n % 4] if rep < 2 else int(rng.integers(1, 60)) * ch + (1 if ch > 1 else 0)
                sample0 = int(rng.integers(0, 5000)) * ch + (int(rng.integers(1, ch)) if ch > 1 else 0)
                if ch > 1:
                    assert sample0 % ch != 0
                    if count % ch == 0:
                        count += 1 if count not in COUNTS else 0
                frames0, frames1 = sample0 // ch, (sample0 + count) // ch
                ff = (0, (frames0 + frames1) // 2, frames1 + 3, frames0, max(frames0 - 2, 0))[n % 5]
                C = (max(ch - 1, 1), ch, ch + 1)[n % 3]
                pl.spans.append(cm.span(in_off=pl.run(count, n & 1), count=count, sample0=sample0, out_off=pl.slab(C * T, phase),
                                        first_frame=ff, frames=T, channels=ch, out_channels=C))
                n += 1
    if ch > 1:
        assert any(sp["count"] % ch for sp in pl.spans)
    assert {sp["count"] for sp in pl.spans} >= set(COUNTS)
    pl.check()


def test_a_row_longer_than_the_run_keeps_its_prefill(gpu):
    rng = np.random.default_rng(7)
    for ch in (1, 2, 3):
        pl = Planes(rng)
        T = 4099
        pl.spans.append(cm.span(in_off=pl.run(300 * ch, 1), count=300 * ch, sample0=0, out_off=pl.slab(ch * T, 1), first_frame=0, frames=T,
                                channels=ch, out_channels=ch))
        d_in = words(rng, pl.in_at + 4)
        got, want = launch(pl.spans, d_in, pl.out_at + 4)
        assert (got == want).all()
        rows = got[pl.spans[0]["out_off"]:][:ch * T].reshape(ch, T)
        assert (rows[:, 300:] == cm.PREFILL).all() and (rows[:, :300] == d_in[pl.spans[0]["in_off"]:][:300 * ch].reshape(300, ch).T).all()


@pytest.mark.parametrize("ch", [1, 2, 3, 6])
def test_consecutive_spans_and_adjacent_slabs(gpu, ch):
    """one file's run cut in two at a sample that is mid-frame (the halves land adjacent in the same rows), a second file whose
    slab follows the first's directly, and the padding of both as zero runs next to the copied floats"""
    rng = np.random.default_rng(40 + ch)
    T, C = 5000, ch + 1
    frames = (4601, 3000)
    spans, in_at = [], 1
    for i, fr in enumerate(frames):
        n = fr * ch
        cut = ((n // 2) // ch) * ch + (1 if ch > 1 else 0)               # not a multiple of the channel count
        for a, b in ((0, cut), (cut, n)):
            spans.append(cm.span(in_off=in_at + a, count=b - a, sample0=a, out_off=3 + i * C * T, first_frame=0, frames=T, channels=ch, out_channels=C))
        in_at += n + 1
        for k in range(ch):                                              # the tails, then the row the file has no channel for
            spans.append(cm.zero_run(3 + i * C * T + k * T + fr, T - fr))
        spans.append(cm.zero_run(3 + i * C * T + ch * T, T))
    d_in = words(rng, in_at + 2)
    got, want = launch(spans, d_in, 3 + 2 * C * T + 2)
    assert (got == want).all()
    assert (want[:3] == cm.PREFILL).all() and (want[-2:] == cm.PREFILL).all() and (want[3:-2] != cm.PREFILL).all()
    first = want[3:3 + C * T].reshape(C, T)
    assert (first[:ch, :frames[0]] == d_in[1:1 + frames[0] * ch].reshape(-1, ch).T).all() and (first[:, frames[0]:] == 0).all() and (first[ch] == 0).all()


def test_zero_runs(gpu):
    rng = np.random.default_rng(9)
    spans, at = [], 1
    for n in (1, 3, 16, 4097, 2 * 4096 + 5):
        for odd in (1, 1, 0):
            at += 2
            if (at & 1) != odd:
                at += 1
            spans.append(cm.zero_run(at, n))
            at += n
    # behind a copy span's last float, and in front of its first
    src = words(rng, 40)
    spans.append(cm.span(in_off=3, count=33, sample0=0, out_off=at + 10, first_frame=0, frames=33, channels=1, out_channels=1))
    spans.append(cm.zero_run(at + 10 + 33, 7))
    spans.append(cm.zero_run(at + 10 - 5, 5))
    got, want = launch(spans, src, at + 64)
    assert (got == want).all() and (want == 0).sum() >= 3 * (1 + 3 + 16 + 4097) and (want == cm.PREFILL).any()


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_words_come_through_as_they_are(gpu, ch):
    special = np.array([0x7fc00000, 0x7fc0dead, 0xffc12345, 0x7f800001, 0x7fbfffff, 0xff800000, 0x7f800000, 0x80000000, 0x00000001,
                        0x807fffff, 0x007fffff, 0x3f800000], np.uint32)
    d_in = np.resize(special, 4096 * ch + 60 * ch)
    spans = [cm.span(in_off=1, count=len(d_in) - 1 - (len(d_in) - 1) % ch, sample0=0, out_off=1, first_frame=0, frames=4200, channels=ch, out_channels=ch)]
    got, want = launch(spans, d_in, 1 + ch * 4200 + 1)
    assert (got == want).all()
    assert set(np.unique(got)) >= set(special.tolist())


def test_a_span_that_leaves_a_plane_is_refused_and_nothing_is_written(gpu):
    rng = np.random.default_rng(3)
    d_in = words(rng, 5000)
    good = cm.span(in_off=0, count=4000, sample0=0, out_off=0, first_frame=0, frames=2000, channels=2, out_channels=2)
    for bad in (dict(good, in_off=1001),                                   # past in_floats
                dict(good, out_off=4193),                                  # the slab past out_floats
                dict(good, frames=4097),                                   # likewise, by its rows
                cm.zero_run(8000, 193)):                                   # a zero run past out_floats
        for spans in ([good, bad], [bad, good]):
            with pytest.raises(afgpu.AfgError, match="invalid argument"):
                launch(spans, d_in, 8192)
            rec = np.zeros(2, afgpu.COLLATE_SPAN_DTYPE)
            for k, sp in enumerate(spans):
                for name, v in sp.items():
                    rec[k][name] = v
            tiles = afgpu.collate_layout(rec)
            d_out = torch.full((8192,), -1, dtype=torch.int32, device="cuda")
            with pytest.raises(afgpu.AfgError):
                afgpu.collate(2, torch.from_numpy(rec.view(np.uint8).copy()).cuda(), tiles, torch.from_numpy(d_in.view(np.int32).copy()).cuda(), 5000, d_out, 8192)
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == -1).all()
    got, want = launch([good], d_in, 8192)                                # (the good span alone does run)
    assert (got == want).all() and (got != cm.PREFILL).sum() == 4000
    # first_frame: refused from 2^61 on; the largest one accepted stores nothing (no sample index reaches such a frame)
    for ch in (1, 2, 3, 65):
        far = dict(good, channels=ch, out_channels=1, count=3999)
        with pytest.raises(afgpu.AfgError, match="invalid argument"):
            launch([dict(far, first_frame=1 << 61)], d_in, 8192)
        with pytest.raises(afgpu.AfgError, match="invalid argument"):
            launch([dict(far, first_frame=-(1 << 61))], d_in, 8192)
        got, want = launch([dict(far, first_frame=(1 << 61) - 1)], d_in, 8192)
        assert (got == want).all() and (got == cm.PREFILL).all()


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_spans_without_tiles(gpu, case):
    """1, 2 and 5 spans, with spans of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    pl = Planes(np.random.default_rng(17))
    for k, count in enumerate(record_lengths(TILE)[case]):
        T = max(count, 1)
        pl.spans.append(cm.span(in_off=pl.run(count, k & 1), count=count, sample0=0, out_off=pl.slab(T, k & 3), first_frame=0, frames=T,
                                channels=1, out_channels=1))
    pl.check()
