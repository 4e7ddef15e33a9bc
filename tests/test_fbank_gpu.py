"""afg_fbank_hip against the intervals tests/fbank_model.py computes from the float64 definition: every delivered element
inside its interval, none left out.  Every input row lies between NaN guard floats and every output slab between sentinel
words: a read outside the row turns outputs into NaN, a store outside a slab kills a sentinel.  Locality is tested by its
two consequences: the same row gives the same bits wherever it stands, and a NaN sample reaches exactly the frames over it.
Each test prints the largest share of an interval's half-width that the device used."""
import functools

import numpy as np
import pytest
import torch

import afgpu
import fbank_model as fm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
TILE = 16                                                        # frames per tile (include/afg.h: afg_fbank_layout)
SAMPLERATE = 16000
# win_length, hop, n_fft, n_mels: Kaldi at 16 kHz with 80 and 23 mels; 8 kHz; a transform that is no power of two; a hop
# beyond the window; the longest transform
FRAMINGS = [(400, 160, 512, 80), (400, 160, 512, 23), (200, 80, 256, 15), (400, 160, 400, 40), (64, 100, 64, 17), (1200, 480, 2048, 128)]
# the options, so that every value of every one of them runs with every framing, edge mode and layout
VARIANTS = [dict(use_power=1, use_log=1, use_energy=1, raw_energy=1, htk_compat=0, preemph=0.97),
            dict(use_power=0, use_log=0, use_energy=1, raw_energy=0, htk_compat=1, preemph=0.0),
            dict(use_power=1, use_log=0, use_energy=0, preemph=0.97, remove_dc=0),
            dict(use_power=0, use_log=1, use_energy=1, raw_energy=0, htk_compat=0, preemph=0.97, energy_floor=0.5, scale=32768.0)]
VARIANT_IDS = ["power-log-raw-front", "magnitude-windowed-htk-nopre", "power-noenergy-nodc", "magnitude-log-windowed-floor-scale"]


@functools.lru_cache(maxsize=None)
def tables(ws, n_fft, n_mels, window_type=afgpu.FBANK_WINDOW_POVEY):
    return afgpu.fbank_tables(window_type, ws, n_fft), afgpu.fbank_filters(SAMPLERATE, n_fft, n_mels, 20.0, 0.0)


class Shares(dict):
    """the largest share of an interval's half-width used, per kind of interval"""

    def __str__(self):
        return ", ".join(f"{k} {v:.4f}" for k, v in self.items())


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, framing, snip_edges=1, layout=afgpu.FBANK_FRAMES_MAJOR, **kw):
        self.ws, self.hop, self.n_fft, self.n_mels = framing
        self.prm = afgpu.fbank_params(self.ws, self.hop, self.n_fft, self.n_mels, snip_edges=snip_edges, layout=layout,
                                      **{"energy_floor": 0.0, **kw})
        self.cols = self.n_mels + self.prm.use_energy
        self.table, self.bank = tables(self.ws, self.n_fft, self.n_mels)
        self.recs, self.rows, self.in_at, self.out_at = [], [], 0, 0

    def most(self, in_frames):
        m = afgpu.fbank_frames(self.prm, in_frames)
        assert m == fm.n_frames(in_frames, self.ws, self.hop, self.prm.snip_edges)
        return m

    def add(self, x, out_frames=None):
        x = np.ascontiguousarray(x, np.float32)
        out_frames = self.most(len(x)) if out_frames is None else out_frames
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, len(x), out_frames))
        self.rows.append(x)
        self.in_at += len(x)
        self.out_at += self.cols * out_frames

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.MEL_ROW_DTYPE)
        for k, ((i, o, n, f), x) in enumerate(zip(self.recs, self.rows)):
            d_in.view(np.uint32)[i:i + n] = x.view(np.uint32)
            rec[k]["in_off"], rec[k]["out_off"], rec[k]["in_frames"], rec[k]["out_frames"] = i, o, n, f
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def device(self, rec, d_in, before, tiles=None, prm=None, **sizes):
        tiles = afgpu.fbank_layout(rec, self.prm) if tiles is None else tiles
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_tab = torch.from_numpy(self.table.copy()).cuda()
        d_fil = torch.from_numpy(np.ascontiguousarray(self.bank, np.float32).reshape(-1).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            afgpu.fbank(len(rec), d_rec, tiles, self.prm if prm is None else prm, d_src, sizes.get("in_floats", len(d_in)), d_tab,
                        sizes.get("table_floats", self.table.size), d_fil, sizes.get("filters_floats", self.bank.size), d_out,
                        sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
        return got

    def interval(self, k):
        """(lo, hi, mid) of record k, [out_frames, cols]"""
        i, o, n, f = self.recs[k]
        return fm.intervals(self.rows[k], self.prm, self.table[:self.ws], self.bank, f)

    def slab(self, got, k):
        """record k's slab as [out_frames, cols], whatever the layout"""
        i, o, n, f = self.recs[k]
        y = got[o:o + self.cols * f].view(np.float32)
        return y.reshape(f, self.cols) if self.prm.layout == afgpu.FBANK_FRAMES_MAJOR else y.reshape(self.cols, f).T

    def untouched(self, got, before):
        written = np.zeros(len(before), bool)
        for (i, o, n, f) in self.recs:
            written[o:o + self.cols * f] = True
        return (got[~written] == SENTINEL).all() and not (got[written] == SENTINEL).any()

    def run(self):
        """every element of every slab inside its interval, everything else untouched; returns (got, the largest share used of
        each kind of interval the launch has: the mel columns' -- power, magnitude or log -- and the energy column's)"""
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        kind = ("log " if self.prm.use_log else "") + ("power" if self.prm.use_power else "magnitude")
        used = Shares({kind: 0.0})
        e_col = np.zeros(self.cols, bool)
        if self.prm.use_energy:
            e_col[self.n_mels if self.prm.htk_compat else 0] = True
            used["raw energy" if self.prm.raw_energy else "windowed energy"] = 0.0
        e_kind = list(used)[-1]
        for k, (i, o, n, f) in enumerate(self.recs):
            if f == 0:
                continue
            lo, hi, mid = self.interval(k)
            y = self.slab(got, k)
            bad = fm.outside(y, lo, hi)
            assert bad.size == 0, (k, n, f, len(bad), bad[:4].tolist(), [(float(y[tuple(b)]), float(lo[tuple(b)]), float(hi[tuple(b)])) for b in bad[:4]])
            used[kind] = max(used[kind], fm.used_share(y[:, ~e_col], lo[:, ~e_col], hi[:, ~e_col], mid[:, ~e_col]))
            if self.prm.use_energy:
                used[e_kind] = max(used[e_kind], fm.used_share(y[:, e_col], lo[:, e_col], hi[:, e_col], mid[:, e_col]))
        assert self.untouched(got, before)
        return got, used


def lengths_of(ws, hop, snip_edges):
    """the row lengths of the issue: 0, 1, pad - 1 (the mirror folds more than once), ws - 1, ws, ws + hop - 1, ws + hop, and
    exactly 16, 17 and 33 frames"""
    frames = (lambda f: ws + (f - 1) * hop) if snip_edges else (lambda f: f * hop)
    ns = [0, 1, ws - 1, ws, ws + hop - 1, ws + hop, frames(16), frames(17), frames(33)]
    pad = fm.pad_of(ws, hop, snip_edges)
    if pad - 1 >= 1:
        ns.insert(2, pad - 1)
    return ns


@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
@pytest.mark.parametrize("snip_edges", [1, 0], ids=["snip", "mirror"])
@pytest.mark.parametrize("framing", FRAMINGS, ids=lambda s: "-".join(map(str, s)))
def test_rows_of_every_framing(gpu, framing, snip_edges, layout, variant):
    ws, hop, n_fft, n_mels = framing
    rng = np.random.default_rng(ws + hop + 2 * snip_edges + layout)
    la = Launch(framing, snip_edges, layout, **VARIANTS[variant])
    amp = 0.5 if la.prm.scale else 2000.0                        # (Kaldi's level either way)
    ns = lengths_of(ws, hop, snip_edges)
    for n in ns:
        la.add(rng.standard_normal(n) * amp + 0.1 * amp)
    n17 = ns[-2]
    impulse = np.zeros(n17)
    impulse[n17 // 2] = amp
    la.add(impulse)
    la.add(np.full(n17, amp))
    long_ = rng.standard_normal(ws + 5 * hop) * amp
    la.add(long_, la.most(len(long_)) - 2)                       # out_frames below the row's frames
    assert [la.recs[ns.index(n)][3] for n in ns[-3:]] == [16, 17, 33] and la.recs[0][3] == 0
    got, used = la.run()
    print(f"fbank {framing} snip {snip_edges} layout {layout} {VARIANT_IDS[variant]}: largest share of an interval's half-width: {used}")
    assert np.isfinite(la.slab(got, len(ns) - 1)).all()


CROSS = [dict(use_power=p, use_log=lg, use_energy=1, raw_energy=raw, htk_compat=htk, preemph=pre)
         for p, lg in ((1, 0), (0, 0), (1, 1)) for raw in (1, 0) for htk in (0, 1) for pre in (0.0, 0.97)]


@pytest.mark.parametrize("edges_layout", [(1, afgpu.FBANK_FRAMES_MAJOR), (0, afgpu.FBANK_MEL_MAJOR)], ids=["snip-frames-major", "mirror-mel-major"])
@pytest.mark.parametrize("opts", CROSS, ids=lambda o: "-".join(f"{k[4:] if k.startswith('use_') else k}{v}" for k, v in o.items() if k != "use_energy"))
def test_every_combination_of_the_options(gpu, opts, edges_layout):
    """power / magnitude / log x raw / windowed energy x front / htk_compat x preemph 0 / 0.97, all 24, on Kaldi's framing"""
    snip_edges, layout = edges_layout
    rng = np.random.default_rng(31)
    la = Launch(FRAMINGS[1], snip_edges, layout, **opts)
    la.add(rng.standard_normal(3000) * 2000.0 + 300.0)           # two tiles
    la.add(rng.standard_normal(401) * 2000.0)
    got, used = la.run()
    print(f"fbank options {opts} snip {snip_edges} layout {layout}: largest share of an interval's half-width: {used}")


# win_length, hop, n_fft, n_mels with an odd n_fft: the transform at full length with a zero imaginary part and no split pass;
# 2025 leaves LDS for two transforming wavefronts only
ODD_FRAMINGS = [(400, 160, 405, 20), (2000, 800, 2025, 30), (1875, 625, 1875, 256)]


@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
@pytest.mark.parametrize("snip_edges", [1, 0], ids=["snip", "mirror"])
@pytest.mark.parametrize("framing", ODD_FRAMINGS, ids=lambda s: "-".join(map(str, s)))
def test_odd_transform_lengths(gpu, framing, snip_edges, layout):
    ws, hop, n_fft, n_mels = framing
    rng = np.random.default_rng(n_fft)
    la = Launch(framing, snip_edges, layout, use_energy=1, raw_energy=0)
    la.add(rng.standard_normal(ws + 17 * hop) * 2000.0 + 100.0)  # two tiles
    la.add(rng.standard_normal(ws - 1) * 2000.0)
    la.add(rng.standard_normal(ws + hop) * 2000.0)
    got, used = la.run()
    print(f"fbank {framing} snip {snip_edges} layout {layout}: largest share of an interval's half-width: {used}")


def test_a_dc_offset_at_kaldis_scale_needs_the_float64_mean(gpu):
    """a unit tone on an offset of 10000 at scale 32768: a float32 accumulator steps by 0.25 near the frame's sum of 4e6, the
    tone is 1 (440 Hz: no whole number of periods in a frame, so the roundings do not cancel)"""
    la = Launch(FRAMINGS[0], 1, afgpu.FBANK_FRAMES_MAJOR, scale=32768.0, use_log=1)
    t = np.arange(3000, dtype=np.float64)
    la.add((10000.0 + np.sin(2.0 * np.pi * 440.0 * t / SAMPLERATE)) / 32768.0)
    got, used = la.run()
    print(f"fbank dc offset: largest share of an interval's half-width: {used}")
    # the same frames with the mean formed by a float32 accumulator, everything else in float64: outside the interval
    lo, hi, _ = la.interval(0)
    F = la.recs[0][3]
    s = (la.rows[0] * np.float32(32768.0))[fm.frame_index(3000, 400, 160, 1, F)]
    mu32 = (np.add.accumulate(s, axis=1, dtype=np.float32)[:, -1] / np.float32(400)).astype(np.float64)
    d = s.astype(np.float64) - mu32[:, None]
    z = np.zeros((F, 512))
    z[:, :400] = (d - la.prm.preemph * np.concatenate([d[:, :1], d[:, :-1]], axis=1)) * la.table[:400].astype(np.float64)
    y32 = np.log(np.maximum((np.abs(np.fft.rfft(z, axis=1)) ** 2) @ la.bank.astype(np.float64).T, fm.EPS))
    assert fm.outside(y32, lo, hi).size > 0


@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
@pytest.mark.parametrize("snip_edges", [1, 0], ids=["snip", "mirror"])
def test_the_same_row_gives_the_same_bits_wherever_it_stands(gpu, snip_edges, layout):
    rng = np.random.default_rng(21)
    x = rng.standard_normal(3000) * 0.5                          # 17 or 19 frames: two tiles
    kw = dict(use_energy=1, scale=32768.0)
    la = Launch(FRAMINGS[0], snip_edges, layout, **kw)
    la.add(x)
    la.add(rng.standard_normal(777) * 0.5)
    la.add(x)
    la.add(rng.standard_normal(2000) * 3.0)
    got, _ = la.run()
    alone = Launch(FRAMINGS[0], snip_edges, layout, **kw)
    alone.add(x)
    got1, _ = alone.run()
    a, b, c = la.slab(got, 0), la.slab(got, 2), alone.slab(got1, 0)
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and (a.view(np.uint32) == c.view(np.uint32)).all()


@pytest.mark.parametrize("use_log", [1, 0], ids=["log", "linear"])
@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
@pytest.mark.parametrize("remove_dc", [1, 0], ids=["dc", "nodc"])
@pytest.mark.parametrize("where", [0, 1700, 3999, -1700], ids=["first", "middle", "last", "middle-snip"])
def test_a_nan_sample_reaches_exactly_the_frames_over_it(gpu, where, remove_dc, layout, use_log):
    """without snip_edges: the first and the last sample stand under the edge frames twice, through the mirror; and one case
    with snip_edges, where the mirror is never taken"""
    snip, where = (1, -where) if where < 0 else (0, where)
    framing = FRAMINGS[1]
    ws, hop, n_fft, n_mels = framing
    rng = np.random.default_rng(22)
    x = (rng.standard_normal(4000) * 0.5).astype(np.float32)
    x[where] = np.nan
    la = Launch(framing, snip, layout, use_energy=1, use_log=use_log, remove_dc=remove_dc)
    la.add(x)
    la.add(rng.standard_normal(900) * 0.5)
    rec, d_in, before = la.planes()
    got = la.device(rec, d_in, before)
    F = la.recs[0][3]
    count = (fm.frame_index(4000, ws, hop, snip, F) == where).sum(axis=1)
    hit = count > 0
    assert list(np.flatnonzero(hit)) == ([9, 10] if snip else {0: [0], 1700: [9, 10, 11], 3999: [24]}[where]) and count.max() == (1 if where == 1700 else 2)
    y = la.slab(got, 0)
    floor = np.log(fm.EPS)
    logs = np.ones(la.cols, bool) if use_log else np.arange(la.cols) == 0          # the energy column is a log always
    v = y[hit]
    assert np.isnan(v[:, ~logs]).all()
    assert (np.abs(v[:, logs] - floor) <= 3 * np.spacing(np.float32(abs(floor)))).all()
    lo, hi, _ = la.interval(0)
    assert np.isnan(lo[hit]).all() and np.isfinite(hi[~hit]).all()
    assert fm.outside(y[~hit], lo[~hit], hi[~hit]).size == 0
    lo, hi, _ = la.interval(1)
    assert fm.outside(la.slab(got, 1), lo, hi).size == 0
    assert la.untouched(got, before)


@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu, layout):
    rng = np.random.default_rng(12)
    la = Launch(FRAMINGS[0], 1, layout, use_energy=1)
    la.add(rng.standard_normal(2000) * 0.5)
    la.add(rng.standard_normal(700) * 0.5)
    rec, d_in, before = la.planes()
    tiles = afgpu.fbank_layout(rec, la.prm)
    assert (la.device(rec, d_in, before) != before).any()       # as it stands it runs
    seen = set()

    def both(change=None, word="invalid argument", **kw):
        bad = rec.copy()
        if change:
            change(bad)
        with pytest.raises(afgpu.AfgError) as e:
            got = la.device(bad, d_in, before, tiles=kw.pop("tiles", tiles), **kw)
        assert word in str(e.value)
        seen.add(str(e.value))

    def unchanged(**kw):
        # (device() raises before it returns: run the refused call again by hand and read the plane)
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_tab = torch.from_numpy(la.table.copy()).cuda()
        d_fil = torch.from_numpy(la.bank.reshape(-1).copy()).cuda()
        with pytest.raises(afgpu.AfgError):
            afgpu.fbank(len(rec), d_rec, kw.get("tiles", tiles), kw.get("prm", la.prm), d_src, len(d_in), d_tab, la.table.size, d_fil, la.bank.size,
                        d_out, kw.get("out_floats", len(before)))
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint32) == before).all()

    both(out_floats=len(before) - GUARD - 1)                     # the last slab's last float
    both(in_floats=int(rec[1]["in_off"]) + 699)
    both(table_floats=la.table.size - 1)
    both(filters_floats=la.bank.size - 1)
    both(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    both(lambda b: b["out_off"].__setitem__(1, (1 << 64) - 8))
    both(lambda b: b["first_tile"].__setitem__(1, 0))
    both(tiles=tiles + 1)
    both(lambda b: b["out_frames"].__setitem__(1, la.most(700) + 1))
    both(prm=afgpu.fbank_params(400, 160, 512, 257))
    both(word="unsupported", prm=afgpu.fbank_params(1102, 441, 1102, 40))
    assert len(seen) >= 10
    unchanged(out_floats=len(before) - GUARD - 1)
    unchanged(tiles=tiles + 1)
    unchanged(prm=afgpu.fbank_params(400, 160, 512, 80, preemph=1.5))


@pytest.mark.parametrize("layout", [afgpu.FBANK_FRAMES_MAJOR, afgpu.FBANK_MEL_MAJOR], ids=["frames-major", "mel-major"])
@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case, layout):
    """1, 2 and 5 rows, with rows of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    framing = (25, 10, 32, 5)
    rng = np.random.default_rng(23)
    la = Launch(framing, 1, layout, use_energy=1)
    for f in record_lengths(TILE)[case]:
        la.add(rng.standard_normal(max(f, 1) * 10 + 25) * 0.5, f)               # (room for more frames than are asked for)
    la.run()


def test_fbank_tensor_is_the_kernel_call(gpu):
    """the tensor call: torchaudio's argument names, valid lengths, both layouts"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 2, 4000)) * 0.3).astype(np.float32)
    wave = torch.from_numpy(x).cuda()
    y = afgpu.fbank_tensor(wave, num_mel_bins=23, use_energy=True, energy_floor=0.0, scale=32768.0)
    assert tuple(y.shape) == (2, 2, 23, 24)
    prm = afgpu.fbank_params(400, 160, 512, 23, use_energy=True, energy_floor=0.0, scale=32768.0)
    table, bank = tables(400, 512, 23)
    for i in range(2):
        for c in range(2):
            lo, hi, _ = fm.intervals(x[i, c], prm, table[:400], bank, 23)
            assert fm.outside(y[i, c].cpu().numpy(), lo, hi).size == 0
    t, counts = afgpu.fbank_tensor(wave, num_mel_bins=23, use_energy=True, energy_floor=0.0, scale=32768.0, snip_edges=False,
                                   layout=afgpu.FBANK_MEL_MAJOR, valid=[4000, 1000, 0, 399])
    assert tuple(t.shape) == (2, 2, 24, 25) and list(counts) == [25, 6, 0, 2]
    full = afgpu.fbank_tensor(wave[:1, 1:2, :1000].contiguous(), num_mel_bins=23, use_energy=True, energy_floor=0.0, scale=32768.0, snip_edges=False)
    assert (t[0, 1].reshape(-1)[:24 * 6].reshape(24, 6).T.cpu().numpy().view(np.uint32) == full[0, 0].cpu().numpy().view(np.uint32)).all()
    assert (t[1, 0] == 0).all()
