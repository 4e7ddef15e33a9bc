"""afg_melspec_fft_hip against the interval tests/melspec_fft_model.py computes from the float64 definition: every output
element inside it, none left out.  Every input row lies between NaN guard floats and every output slab between sentinel
words: a read outside the row turns outputs into NaN, a store outside a slab kills a sentinel.  Locality is tested by its
two consequences: the same row gives the same bits wherever it stands, and a NaN sample reaches exactly the frames over it."""
import functools

import numpy as np
import pytest
import torch

import afgpu
import melspec_fft_model as fm
import melspec_model as mm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
TILE = 16                                                        # frames per tile (include/afg.h: afg_mel_fft_layout)
# n_fft, win_length, hop, n_mels, center: radix 4, 2, 5, 5 behind the split pass; a zero-padded window, radix 4 alone; the
# minimal shape; radix 2, 3, 5 with an odd window in an even frame; an odd half length (125 = 5^3); the largest allowed
SHAPES = [(400, 400, 160, 80, True), (512, 400, 128, 23, True), (16, 16, 1, 1, True), (60, 45, 7, 5, True), (250, 250, 100, 17, True),
          (2048, 2048, 2048, 256, False)]
SAMPLERATE = 16000
KINDS = [(afgpu.MEL_POWER, 0.0), (afgpu.MEL_POWER, 1e-3), (afgpu.MEL_LOG10, 0.0), (afgpu.MEL_LOG10, 1e-3)]
KIND_IDS = ["power-0", "power-1e-3", "log10-0", "log10-1e-3"]


@functools.lru_cache(maxsize=None)
def tables(n_fft, win, n_mels):
    return afgpu.mel_fft_tables(n_fft, win), afgpu.mel_filters(SAMPLERATE, n_fft, n_mels)


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, shape, pad_mode, out_kind=afgpu.MEL_POWER, log_floor=0.0):
        self.n_fft, self.win, self.hop, self.n_mels, self.center = shape
        self.pad_mode, self.out_kind, self.log_floor = pad_mode, out_kind, log_floor
        self.prm = afgpu.mel_params(self.n_fft, self.hop, self.n_mels, self.win, self.center, pad_mode, out_kind, log_floor)
        self.table, self.bank = tables(self.n_fft, self.win, self.n_mels)
        self.recs, self.rows, self.in_at, self.out_at = [], [], 0, 0

    def most(self, in_frames):
        m = afgpu.mel_frames(self.prm, in_frames)
        assert m == mm.max_frames(in_frames, self.n_fft, self.hop, self.center)
        return m

    def add(self, x, out_frames=None):
        x = np.ascontiguousarray(x, np.float32)
        out_frames = self.most(len(x)) if out_frames is None else out_frames
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, len(x), out_frames))
        self.rows.append(x)
        self.in_at += len(x)
        self.out_at += self.n_mels * out_frames

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.MEL_ROW_DTYPE)
        for k, ((i, o, n, f), x) in enumerate(zip(self.recs, self.rows)):
            d_in.view(np.uint32)[i:i + n] = x.view(np.uint32)
            rec[k]["in_off"], rec[k]["out_off"], rec[k]["in_frames"], rec[k]["out_frames"] = i, o, n, f
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def device(self, rec, d_in, before, tiles=None, prm=None, **sizes):
        tiles = afgpu.mel_fft_layout(rec, self.prm) if tiles is None else tiles
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_tab = torch.from_numpy(self.table.copy()).cuda()
        d_fil = torch.from_numpy(np.ascontiguousarray(self.bank, np.float32).reshape(-1).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            afgpu.melspec_fft(len(rec), d_rec, tiles, self.prm if prm is None else prm, d_src, sizes.get("in_floats", len(d_in)), d_tab,
                              sizes.get("table_floats", self.table.size), d_fil, sizes.get("filters_floats", self.bank.size), d_out,
                              sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
        return got

    def interval(self, k):
        """(lo, hi, mid) of record k for this launch's out_kind, [n_mels, out_frames]; mid is the float64 power"""
        i, o, n, f = self.recs[k]
        lo, hi, mid = fm.power_interval(self.rows[k], self.bank, self.n_fft, self.win, self.hop, self.center, self.pad_mode, f)
        if self.out_kind == afgpu.MEL_LOG10:
            lo, hi = fm.log_interval(lo, hi, self.log_floor)
        return lo, hi, mid

    def slab(self, got, k):
        i, o, n, f = self.recs[k]
        return got[o:o + self.n_mels * f].view(np.float32).reshape(self.n_mels, f)

    def run(self):
        """every element of every slab inside its interval, everything else untouched; returns (got, used fraction)"""
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        written = np.zeros(len(before), bool)
        used = 0.0
        for k, (i, o, n, f) in enumerate(self.recs):
            written[o:o + self.n_mels * f] = True
            if f == 0:
                continue
            lo, hi, mid = self.interval(k)
            y = self.slab(got, k)
            bad = fm.outside(y, lo, hi)
            assert bad.size == 0, (k, len(bad), bad[:4].tolist(), [(float(y[tuple(b)]), float(lo[tuple(b)]), float(hi[tuple(b)])) for b in bad[:4]])
            if self.out_kind == afgpu.MEL_POWER:
                used = max(used, fm.used_fraction(y, lo, hi, mid))
        assert (got[~written] == SENTINEL).all()
        return got, used


@pytest.mark.parametrize("pad_mode", [afgpu.MEL_PAD_REFLECT, afgpu.MEL_PAD_ZERO], ids=["reflect", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}-{s[3]}")
def test_rows_of_every_shape(gpu, shape, pad_mode):
    n_fft, win, hop, n_mels, center = shape
    rng = np.random.default_rng(n_fft + hop + pad_mode)
    la = Launch(shape, pad_mode)
    pad = n_fft // 2 if center else 0
    noise = lambda n: rng.standard_normal(n) * 0.5
    la.add(noise(1600 if n_fft == 400 else 3 * n_fft + 5))                      # a few frames
    la.add(noise(max(pad + 1, 0 if center else n_fft)))                          # reflect's minimum (without centre: one frame)
    la.add(noise(TILE * hop + n_fft - 2 * pad))                                  # exactly one tile of frames plus one
    assert la.recs[-1][3] == TILE + 1
    la.add(np.zeros(0), 0 if (pad_mode == afgpu.MEL_PAD_REFLECT or not center) else None)     # no samples: zero padding alone makes a frame
    long_ = noise(5 * hop + n_fft)
    la.add(long_, la.most(len(long_)) - 2)                                       # out_frames < max_frames
    got, used = la.run()
    print(f"n_fft {n_fft} pad_mode {pad_mode}: largest deviation {used:.4f} of the interval's half-width")
    assert (la.slab(got, 0) > 0).any()
    if pad_mode == afgpu.MEL_PAD_ZERO and center:
        i, o, n, f = la.recs[3]
        assert (n, f) == (0, 1) and (got[o:o + n_mels] == 0).all()                # the frame of an empty row: +0.0f


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_a_sine_on_a_bin_centre(gpu, kind):
    """most bins hold rounding noise alone: their power interval starts at 0 and ends at the bound's square"""
    la = Launch(SHAPES[0], afgpu.MEL_PAD_REFLECT, *kind)
    n = np.arange(2400, dtype=np.float64)
    la.add(0.5 * np.sin(2.0 * np.pi * 40.0 * n / 400.0))
    la.add(np.zeros(1000))                                                       # and a silent row: +0.0f, or the floor
    got, _ = la.run()
    silent = la.slab(got, 1)
    assert (silent.view(np.uint32) == silent.view(np.uint32)[0, 0]).all()
    if kind[0] == afgpu.MEL_POWER:
        assert silent.view(np.uint32)[0, 0] == 0


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_the_same_row_gives_the_same_bits_wherever_it_stands(gpu, kind):
    rng = np.random.default_rng(21)
    x = rng.standard_normal(3000) * 0.5                                          # 19 frames: two tiles
    la = Launch(SHAPES[0], afgpu.MEL_PAD_REFLECT, *kind)
    la.add(x)
    la.add(rng.standard_normal(777) * 0.5)
    la.add(x)
    la.add(rng.standard_normal(2000) * 3.0)
    got, _ = la.run()
    alone = Launch(SHAPES[0], afgpu.MEL_PAD_REFLECT, *kind)
    alone.add(x)
    got1, _ = alone.run()
    a, b, c = la.slab(got, 0), la.slab(got, 2), alone.slab(got1, 0)
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and (a.view(np.uint32) == c.view(np.uint32)).all()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_a_nan_sample_reaches_exactly_the_frames_over_it(gpu, kind):
    shape = SHAPES[0]
    n_fft, win, hop, n_mels, center = shape
    rng = np.random.default_rng(22)
    x = (rng.standard_normal(4000) * 0.5).astype(np.float32)
    x[1700] = np.nan
    la = Launch(shape, afgpu.MEL_PAD_REFLECT, *kind)
    la.add(x)
    la.add(rng.standard_normal(900) * 0.5)
    rec, d_in, before = la.planes()
    got = la.device(rec, d_in, before)
    f = la.recs[0][3]
    hit = np.isnan(mm.frames_of(x, n_fft, win, hop, center, la.pad_mode, f)).any(axis=1)
    assert list(np.flatnonzero(hit)) == [10, 11]
    y = la.slab(got, 0)
    if kind[0] == afgpu.MEL_POWER:
        assert np.isnan(y[:, hit]).all()
    else:                                                                        # fmaxf: a NaN mel gives the floor
        floor = np.float64(np.float32(kind[1] if kind[1] else 1e-10))
        v = y[:, hit]
        assert (v.view(np.uint32) == v.view(np.uint32)[0, 0]).all()
        assert abs(float(v[0, 0]) - np.log10(floor)) <= 3 * np.spacing(np.abs(np.float32(np.log10(floor))))
    lo, hi, _ = la.interval(0)
    assert np.isnan(lo[:, hit]).all() and np.isfinite(hi[:, ~hit]).all()
    assert fm.outside(y[:, ~hit], lo[:, ~hit], hi[:, ~hit]).size == 0
    lo, hi, _ = la.interval(1)
    assert fm.outside(la.slab(got, 1), lo, hi).size == 0
    written = np.zeros(len(before), bool)
    for (i, o, n, fr) in la.recs:
        written[o:o + n_mels * fr] = True
    assert (got[~written] == SENTINEL).all()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu, kind):
    rng = np.random.default_rng(12)
    la = Launch(SHAPES[0], afgpu.MEL_PAD_REFLECT, *kind)
    la.add(rng.standard_normal(2000) * 0.5)
    la.add(rng.standard_normal(700) * 0.5)
    rec, d_in, before = la.planes()
    tiles = afgpu.mel_fft_layout(rec, la.prm)
    assert (la.device(rec, d_in, before) != before).any()                          # as it stands it runs
    seen = set()

    def both(change=None, word="invalid argument", **kw):
        bad = rec.copy()
        if change:
            change(bad)
        d_rec = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_tab = torch.from_numpy(la.table.copy()).cuda()
        d_fil = torch.from_numpy(la.bank.reshape(-1).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            with pytest.raises(afgpu.AfgError) as e:
                afgpu.melspec_fft(len(bad), d_rec, kw.get("tiles", tiles), kw.get("prm", la.prm), d_src, kw.get("in_floats", len(d_in)), d_tab,
                                  kw.get("table_floats", la.table.size), d_fil, kw.get("filters_floats", la.bank.size), d_out,
                                  kw.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
        assert word in str(e.value)
        seen.add(str(e.value))
        assert (d_out.cpu().numpy().view(np.uint32) == before).all()

    both(out_floats=len(before) - GUARD - 1)                                       # the last slab's last float
    both(in_floats=int(rec[1]["in_off"]) + 699)
    both(table_floats=la.table.size - 1)
    both(filters_floats=la.bank.size - 1)
    both(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    both(lambda b: b["out_off"].__setitem__(1, (1 << 64) - 8))
    both(lambda b: b["first_tile"].__setitem__(1, 0))
    both(tiles=tiles + 1)
    both(lambda b: b["out_frames"].__setitem__(1, la.most(700) + 1))
    both(lambda b: b["in_frames"].__setitem__(1, 200))                             # reflect with in_frames <= pad (and too many frames)
    both(prm=afgpu.mel_params(400, 160, 257))
    both(word="unsupported", prm=afgpu.mel_params(401, 160, 80, 400))              # a size the direct path alone takes
    assert len(seen) >= 10


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case):
    """1, 2 and 5 rows, with rows of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    shape = (60, 45, 7, 5, True)
    n_fft, hop = shape[0], shape[2]
    rng = np.random.default_rng(23)
    la = Launch(shape, afgpu.MEL_PAD_ZERO)
    for f in record_lengths(TILE)[case]:
        la.add(rng.standard_normal(max(f, 1) * hop + n_fft) * 0.5, f)          # (room for more frames than are asked for)
    la.run()
