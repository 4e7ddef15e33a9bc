"""afg_istft_hip against the interval tests/istft_model.py computes from the float64 definition: every delivered sample inside
its interval, none left out.  The harness is tests/test_stft_gpu.py's turned round: every slab lies between NaN guard floats
(and what a row's in_pitch holds beyond its n_frames is NaN too) and every output row between sentinel words -- a read outside
the record turns samples into NaN, a store outside a row kills a sentinel.  Locality and order are tested by their
consequences: the same slab gives the same bits wherever it stands and whichever tile a sample falls in, and a NaN reaches
exactly the window span of its frame."""
import functools

import numpy as np
import pytest
import torch

import afgpu
import istft_model as im
from record_cases import RECORD_CASES, record_lengths
import melspec_fft_model as fm

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
PAD_REFLECT = 0
# n_fft, win_length, hop, center: the minimal shape; m = 16 frames over every sample; Whisper's (radix 4, 2, 5, 5 behind the
# split pass); a window shorter than the frame; an odd n_fft, the full-length path; the two long power-of-two shapes, whose
# staging is 16 and 4 frames wide; the two odd n_fft whose full-length buffers leave room for two transforming wavefronts;
# and two lines without centring, which start behind the window's zero
SHAPES = [(16, 16, 4, True), (16, 16, 1, True), (400, 400, 160, True), (400, 300, 100, True), (75, 60, 20, True), (1024, 1024, 256, True),
          (2048, 2048, 512, True), (1875, 1875, 625, True), (2025, 2025, 405, True), (400, 400, 160, False), (400, 300, 100, False)]
IDS = ["-".join(map(str, s[:3])) + ("" if s[3] else "-uncentred") for s in SHAPES]


@functools.lru_cache(maxsize=None)
def table_of(n_fft, win):
    return afgpu.mel_fft_tables(n_fft, win)


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, shape):
        self.n_fft, self.win, self.hop, self.center = shape
        self.prm = afgpu.istft_params(self.n_fft, self.hop, self.win, self.center)
        self.tile = afgpu.istft_tile_samples(self.prm)
        self.table = table_of(self.n_fft, self.win)
        self.n_bins, self.n_lo, self.pad = self.n_fft // 2 + 1, (self.n_fft - self.win) // 2, (self.n_fft // 2 if self.center else 0)
        self.first0 = 0 if self.center else self.n_lo + 1         # the first sample a line can deliver
        self.recs, self.slabs, self.in_at, self.out_at = [], [], 0, 0

    def frames_for(self, first, count):
        """the fewest frames whose line holds samples first .. first + count with the envelope well above its floor"""
        return -(-(first + count) // self.hop) + 1

    def add(self, spec, count, first=None, pitch=None):
        """spec: float32 [n_bins, n_frames, 2]"""
        spec = np.ascontiguousarray(spec, np.float32)
        f = spec.shape[1]
        pitch = f if pitch is None else pitch
        first = self.first0 if first is None else first
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, f, pitch, first, count))
        self.slabs.append(spec)
        self.in_at += 2 * self.n_bins * pitch
        self.out_at += count
        return len(self.recs) - 1

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.ISTFT_ROW_DTYPE)
        for k, ((i, o, f, pitch, first, count), s) in enumerate(zip(self.recs, self.slabs)):
            d_in[i:i + 2 * self.n_bins * pitch].reshape(self.n_bins, pitch, 2)[:, :f] = s
            rec[k] = (i, o, 0, f, pitch, first, count)
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def device(self, rec, d_in, before, **kw):
        tiles = kw["tiles"] if "tiles" in kw else afgpu.istft_layout(rec, self.prm)      # (a caller with tiles has laid the records out)
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_tab = torch.from_numpy(self.table.copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            afgpu.istft(len(rec), d_rec, tiles, kw.get("prm", self.prm), d_src, kw.get("in_floats", len(d_in)), d_tab,
                        kw.get("table_floats", self.table.size), d_out, kw.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = self.last = d_out.cpu().numpy().view(np.uint32)
        return got

    def interval(self, k):
        i, o, f, pitch, first, count = self.recs[k]
        s = self.slabs[k].astype(np.float64)
        return im.interval(s[:, :, 0], s[:, :, 1], self.n_fft, self.win, self.hop, self.center, first, count)

    def row(self, got, k):
        i, o, f, pitch, first, count = self.recs[k]
        return got[o:o + count].view(np.float32)

    def written(self, before):
        w = np.zeros(len(before), bool)
        for (i, o, f, pitch, first, count) in self.recs:
            w[o:o + count] = True
        return w

    def run(self, skip=()):
        """every sample of every row inside its interval, everything else untouched; returns (got, used fraction)"""
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        used = 0.0
        for k, r in enumerate(self.recs):
            if r[5] == 0 or k in skip:
                continue
            lo, hi, mid = self.interval(k)
            y = self.row(got, k)
            bad = im.outside(y, lo, hi)
            assert bad.size == 0, (k, len(bad), bad[:4].ravel().tolist(), [(float(y[b[0]]), float(lo[b[0]]), float(hi[b[0]])) for b in bad[:4]])
            used = max(used, im.used_fraction(y, lo, hi, mid))
        assert (got[~self.written(before)] == SENTINEL).all()
        return got, used


def noise_spec(rng, n_bins, f):
    return rng.standard_normal((n_bins, f, 2)).astype(np.float32)


def stft_of(x, la, f):
    """the float64 STFT of a float32 row, rounded to float32: [n_bins, f, 2]"""
    re, imag, _ = fm.spectrum64(x, la.n_fft, la.win, la.hop, True, PAD_REFLECT, f)
    return np.stack([re, imag], axis=-1).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_of_every_geometry(gpu, shape):
    n_fft, win, hop, center = shape
    rng = np.random.default_rng(n_fft + hop + center)
    la = Launch(shape)
    T = la.tile
    for count in (T - 1, T, T + 1):                                               # rows that end 1 before, on and 1 after a tile edge
        la.add(noise_spec(rng, la.n_bins, la.frames_for(la.first0, count)), count)
    if center:                                                                    # three tiles of a signal's own spectrum, to the natural length
        f = -(-(2 * T + 5) // hop) + 1
        x = rng.standard_normal(hop * f).astype(np.float32)                       # (a hop more than delivered: an odd n_fft pads one sample less)
        trip = la.add(stft_of(x, la, f), hop * (f - 1))
    else:
        trip = la.add(noise_spec(rng, la.n_bins, la.frames_for(la.first0, 2 * T + 5)), 2 * T + 5)
    first = la.first0 + 3 * hop + 7                                               # out_first > 0 inside a slab wider than its frames
    f = la.frames_for(first, 333)
    la.add(noise_spec(rng, la.n_bins, f), 333, first=first, pitch=f + 5)
    one = np.zeros((la.n_bins, 4, 2), np.float32)                                 # a single bin, in a single frame
    one[min(3, la.n_bins - 2), 1] = (0.75, -0.5)
    la.add(one, min(2 * hop, 300))
    zero = la.add(np.zeros((la.n_bins, 5, 2), np.float32), min(3 * hop, 500))
    la.add(noise_spec(rng, la.n_bins, 2), 0)                                      # nothing to deliver
    got, used = la.run()
    print(f"istft {IDS[SHAPES.index(shape)]}: tile {T}, largest deviation {used:.4f} of the interval's half-width")
    assert (la.row(got, zero).view(np.uint32) == 0).all()                         # +0.0f
    assert (la.row(got, 0) != 0).any()
    if center:
        y = la.row(got, trip).astype(np.float64)
        s = torch.view_as_complex(torch.from_numpy(la.slabs[trip]).cuda())
        ref = torch.istft(s, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, device="cuda"), center=True, length=len(y))
        print(f"   round trip |ours - input| {np.abs(y - x[:len(y)]).max():.3g}, |ours - torch.istft| {np.abs(y - ref.cpu().numpy()).max():.3g} (informational)")


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[1], SHAPES[4]], ids=[IDS[2], IDS[1], IDS[4]])
def test_the_same_slab_gives_the_same_bits_wherever_it_stands_and_whichever_tile_a_sample_falls_in(gpu, shape):
    n_fft, win, hop, center = shape
    rng = np.random.default_rng(31)
    la = Launch(shape)
    T = la.tile
    count, shift = 2 * T + 77, T // 2 + 13                                        # the second range starts elsewhere in its tiles
    spec = noise_spec(rng, la.n_bins, la.frames_for(shift, count))
    a = la.add(spec, count)
    la.add(noise_spec(rng, la.n_bins, 9), min(5 * hop, 700))
    b = la.add(spec, count)                                                       # the twin, elsewhere in the batch
    c = la.add(spec, count, first=shift)                                          # and the same line from another first sample
    la.add(noise_spec(rng, la.n_bins, 4) * 3.0, min(2 * hop, 300))
    got, _ = la.run()
    alone = Launch(shape)
    alone.add(spec, count)
    got1, _ = alone.run()
    ya, yb, yc, y1 = (r.view(np.uint32) for r in (la.row(got, a), la.row(got, b), la.row(got, c), alone.row(got1, 0)))
    assert (ya == yb).all() and (ya == y1).all()
    assert (ya[shift:] == yc[:count - shift]).all()                               # the overlap of the two ranges


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[0]], ids=[IDS[2], IDS[3], IDS[4], IDS[0]])
def test_a_nan_reaches_exactly_the_window_span_of_its_frame_and_the_ignored_parts_reach_nothing(gpu, shape):
    n_fft, win, hop, center = shape
    rng = np.random.default_rng(32)
    la = Launch(shape)
    f = 12
    count = hop * (f - 1)
    clean = noise_spec(rng, la.n_bins, f)
    hit = clean.copy()
    hit[5, 7, 0] = np.nan                                                         # a real part in frame 7 ...
    hit[la.n_bins - 2, 3, 1] = np.nan                                             # ... and an imaginary part in frame 3
    blind = clean.copy()
    blind[im.real_only(n_fft), :, 1] = np.nan                                     # parts that take no part
    blind[0, 4, 1] = np.inf
    a, b, c = la.add(clean, count), la.add(hit, count), la.add(blind, count)
    d = la.add(noise_spec(rng, la.n_bins, 6), 3 * hop)
    rec, d_in, before = la.planes()
    got = la.device(rec, d_in, before)
    t = np.arange(count) + la.pad
    under = np.zeros(count, bool)
    for fr in (7, 3):
        under |= (t >= fr * hop + la.n_lo) & (t < fr * hop + la.n_lo + win)
    assert under.any() and not under.all()
    ya, yb, yc = la.row(got, a), la.row(got, b), la.row(got, c)
    assert np.isnan(yb[under]).all()                                              # (the sample under w = 0 included)
    assert (yb[~under].view(np.uint32) == ya[~under].view(np.uint32)).all()
    assert (yc.view(np.uint32) == ya.view(np.uint32)).all()
    lo, hi, _ = la.interval(b)
    assert np.isnan(lo[under]).all() and np.isfinite(lo[~under]).all()
    for k in (a, d):
        lo, hi, _ = la.interval(k)
        assert im.outside(la.row(got, k), lo, hi).size == 0
    assert (got[~la.written(before)] == SENTINEL).all()


def test_istft_tensor_on_the_librarys_own_spectrum_and_valid_frames(gpu):
    n_fft, hop, frames = 400, 160, 140                                            # three tiles
    rng = np.random.default_rng(33)
    x = (rng.standard_normal((2, 3, hop * (frames - 1))) * 0.5).astype(np.float32)
    prm = afgpu.stft_params(n_fft, hop, None, True, afgpu.MEL_PAD_REFLECT, afgpu.STFT_COMPLEX)
    n_bins, n = n_fft // 2 + 1, 6
    rows = np.zeros(n, afgpu.MEL_ROW_DTYPE)
    rows["in_off"] = np.arange(n) * x.shape[-1]
    rows["out_off"] = np.arange(n) * (2 * n_bins * frames)
    rows["in_frames"], rows["out_frames"] = x.shape[-1], frames
    tiles = afgpu.stft_layout(rows, prm)
    table = torch.from_numpy(table_of(n_fft, n_fft)).cuda()
    d_x = torch.from_numpy(x).cuda()
    spec = torch.zeros((2, 3, n_bins, frames, 2), dtype=torch.float32, device="cuda")
    afgpu.stft(n, torch.from_numpy(rows.view(np.uint8).copy()).cuda(), tiles, prm, d_x, d_x.numel(), table, table.numel(), spec, spec.numel())
    y = afgpu.istft_tensor(torch.view_as_complex(spec), n_fft, hop)
    assert y.shape == x.shape and y.dtype == torch.float32
    s = spec.cpu().numpy().astype(np.float64)
    got = y.cpu().numpy()
    used = 0.0
    for i in range(2):
        for k in range(3):
            lo, hi, mid = im.interval(s[i, k, :, :, 0], s[i, k, :, :, 1], n_fft, n_fft, hop, True, 0, x.shape[-1])
            assert im.outside(got[i, k], lo, hi).size == 0
            used = max(used, im.used_fraction(got[i, k], lo, hi, mid))
    ref = torch.istft(torch.view_as_complex(spec).reshape(6, n_bins, frames), n_fft, hop_length=hop, window=torch.hann_window(n_fft, device="cuda"),
                      length=x.shape[-1]).reshape(x.shape)
    print(f"istft_tensor: used {used:.4f}; round trip |ours - input| {np.abs(got - x).max():.3g}, |ours - torch.istft| {float((y - ref).abs().max()):.3g} (informational)")
    # the float32 view, a range of its own and an out tensor
    part = torch.full((2, 3, 1000), 7.0, device="cuda")
    assert afgpu.istft_tensor(spec, n_fft, hop, length=1000, first=321, out=part) is part
    assert (part.cpu().numpy().view(np.uint32) == got[..., 321:1321].view(np.uint32)).all()
    # valid_frames: every slab's own frames, and what lies behind them is left alone
    valid = np.array([frames, 1, 0, 17, frames - 1, 64])
    kept = torch.full(x.shape, 7.0, device="cuda")
    afgpu.istft_tensor(spec, n_fft, hop, valid_frames=valid, out=kept)
    kept = kept.cpu().numpy().reshape(6, -1)
    for r, v in enumerate(valid):
        reach = hop * (v - 1) if v else 0
        i, k = divmod(r, 3)
        assert (kept[r, reach:] == 7.0).all()
        if reach:
            lo, hi, _ = im.interval(s[i, k, :, :v, 0], s[i, k, :, :v, 1], n_fft, n_fft, hop, True, 0, reach)
            assert im.outside(kept[r, :reach], lo, hi).size == 0
    fresh = afgpu.istft_tensor(spec, n_fft, hop, valid_frames=torch.from_numpy(valid)).cpu().numpy().reshape(6, -1)
    assert (fresh[1] == 0).all() and (fresh[3, hop * 16:] == 0).all() and (fresh[3, :hop * 16].view(np.uint32) == kept[3, :hop * 16].view(np.uint32)).all()
    with pytest.raises(afgpu.AfgError, match="envelope"):
        afgpu.istft_tensor(spec, n_fft, hop, center=False, length=1000)
    with pytest.raises(ValueError):
        afgpu.istft_tensor(spec[:, :, :-1], n_fft, hop)


def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu):
    rng = np.random.default_rng(34)
    la = Launch(SHAPES[2])
    la.add(noise_spec(rng, la.n_bins, 11), 1600)
    la.add(noise_spec(rng, la.n_bins, 6), 700, pitch=8)
    rec, d_in, before = la.planes()
    tiles = afgpu.istft_layout(rec, la.prm)
    assert (la.device(rec, d_in, before) != before).any()                          # as it stands it runs
    seen = set()

    def refused(change=None, word="invalid argument", **kw):
        bad = rec.copy()
        if change:
            change(bad)
        kw.setdefault("tiles", tiles)
        with pytest.raises(afgpu.AfgError) as e:
            la.device(bad, d_in, before, **kw)
        assert word in str(e.value)
        seen.add(str(e.value))
        assert (la.last == before).all()                                           # nothing was written

    refused(out_floats=len(before) - GUARD - 1)
    refused(in_floats=int(rec[1]["in_off"]) + 2 * ((la.n_bins - 1) * 8 + 6) - 1)      # the last slab's last pair
    refused(table_floats=la.table.size - 1)
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["first_tile"].__setitem__(1, 0))
    refused(lambda b: b["n_frames"].__setitem__(1, 9))
    refused(lambda b: b["out_frames"].__setitem__(0, 1801))
    refused(prm=afgpu.IstftParams(400, 400, 160, 0))                              # the line starts on the window's zero
    refused(prm=afgpu.IstftParams(400, 400, 160, 1, (1, 0, 0, 0)))
    refused(word="unsupported", prm=afgpu.IstftParams(14 * 3 * 5, 16, 16, 1))
    assert len(seen) == 10


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case):
    """1, 2 and 5 rows, with rows of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(29)
    la = Launch((16, 16, 4, True))
    for count in record_lengths(la.tile)[case]:
        la.add(noise_spec(rng, la.n_bins, la.frames_for(la.first0, count)), count)
    la.run()
