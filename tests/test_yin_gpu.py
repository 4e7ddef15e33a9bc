"""afg_yin_hip against tests/yin_model.py's float32 restatement of include/afg.h: both planes of every record compared as
uint32 bit patterns, decisions included.  Every input row lies between NaN guard floats and every output slab between
sentinel words: a read outside the row turns outputs into NaN, a store outside a slab kills a sentinel.  Every launch runs
behind afg_lds_fill_probe_hip(0x7fc00000): a word of LDS the kernel reads without having written it is a NaN.  Locality is
tested by its consequences: the same row gives the same bits wherever it stands, and a NaN sample reaches exactly the
frames whose samples 0 .. W - 1 + tau_max cover it."""
import numpy as np
import pytest
import torch

import afgpu
import yin_model as ym
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
TILE = afgpu.YIN_TILE
RATE = 16000.0
# frame_length, win_length, hop, tau_min, tau_max: the limit N - W - 1; one lag and a hop beyond the frame; a lag count that
# crosses and one that meets the chunk edge; librosa's defaults at 16 kHz; all 128 chunks
SHAPES = [(64, 32, 16, 2, 31), (64, 32, 100, 7, 7), (100, 37, 33, 5, 17), (100, 37, 33, 3, 16), (2048, 1024, 512, 32, 320),
          (4096, 2048, 1024, 1, 2047)]
SHAPE_IDS = ["-".join(map(str, s)) for s in SHAPES]
OPTIONS = [(1, afgpu.MEL_PAD_ZERO), (1, afgpu.MEL_PAD_REFLECT), (0, afgpu.MEL_PAD_ZERO), (0, afgpu.MEL_PAD_REFLECT)]
OPTION_IDS = ["center-zero", "center-reflect", "nocenter-zero", "nocenter-reflect"]


def length_for(shape, center, frames):
    """the shortest row with exactly `frames` frames (0: none)"""
    N, W, hop = shape[:3]
    return max(N - (2 * (N // 2) if center else 0) + (frames - 1) * hop, 1 if frames == 1 else 0)


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, shape, center=1, pad_mode=afgpu.MEL_PAD_ZERO, threshold=0.1):
        self.shape = shape
        N, W, hop, tau_min, tau_max = shape
        self.prm = afgpu.yin_params(RATE, N, W, hop, tau_min, tau_max, threshold, center, pad_mode)
        self.model = ym.params(RATE, N, W, hop, tau_min, tau_max, threshold, center, pad_mode)
        self.recs, self.rows, self.in_at, self.out_at = [], [], 0, 0

    def most(self, in_frames):
        m = afgpu.yin_frames(self.prm, in_frames)
        assert m == ym.n_frames(in_frames, self.model)
        return m

    def add(self, x, out_frames=None):
        x = np.ascontiguousarray(x, np.float32)
        out_frames = self.most(len(x)) if out_frames is None else out_frames
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, len(x), out_frames))
        self.rows.append(x)
        self.in_at += len(x)
        self.out_at += 2 * out_frames

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.MEL_ROW_DTYPE)
        for k, ((i, o, n, f), x) in enumerate(zip(self.recs, self.rows)):
            d_in.view(np.uint32)[i:i + n] = x.view(np.uint32)
            rec[k]["in_off"], rec[k]["out_off"], rec[k]["in_frames"], rec[k]["out_frames"] = i, o, n, f
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def device(self, rec, d_in, before, tiles=None, prm=None, d_out=None, **sizes):
        tiles = afgpu.yin_layout(rec, self.prm) if tiles is None else tiles
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda() if d_out is None else d_out
        afgpu.lds_fill()
        try:
            afgpu.yin(len(rec), d_rec, tiles, self.prm if prm is None else prm, d_src, sizes.get("in_floats", len(d_in)), d_out,
                      sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
        return got

    def want(self, k):
        """[2, out_frames] uint32, and tau* per frame"""
        i, o, n, f = self.recs[k]
        planes, taus, _ = ym.yin32(self.rows[k], self.model, f)
        return planes.view(np.uint32), taus

    def slab(self, got, k):
        i, o, n, f = self.recs[k]
        return got[o:o + 2 * f].reshape(2, f)

    def untouched(self, got, before):
        written = np.zeros(len(before), bool)
        for (i, o, n, f) in self.recs:
            written[o:o + 2 * f] = True
        return (got[~written] == SENTINEL).all() and not (got[written] == SENTINEL).any()

    def run(self):
        """every slab bit for bit the model's, everything else untouched; returns (got, tau* per record)"""
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        taus = []
        for k in range(len(self.recs)):
            want, t = self.want(k)
            y = self.slab(got, k)
            bad = np.argwhere(y != want)
            assert bad.size == 0, (k, self.recs[k], len(bad), bad[:4].tolist(), [(hex(y[tuple(b)]), hex(want[tuple(b)])) for b in bad[:4]])
            taus.append(t)
        assert self.untouched(got, before)
        return got, taus


def tone(f_true, n, rng, noise):
    t = np.arange(n, dtype=np.float64) / RATE
    x = sum(a * np.sin(2.0 * np.pi * k * f_true * t + 0.3 * k) for k, a in ((1, 1.0), (2, 0.5), (3, 0.33)))
    return 0.25 * (x + noise * rng.standard_normal(n))


@pytest.mark.parametrize("option", OPTIONS, ids=OPTION_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rows_of_every_shape(gpu, shape, option):
    """row lengths that give TILE - 1, TILE, TILE + 1 frames and 1 frame, a zero-pad row shorter than the padding, a record that
    asks for fewer frames than its row has; noise (the global-minimum path), tone + noise (the threshold path), an integer
    periodic row with d'(P) = d'(2 P) = 0 (the tie goes to the first), all-zero and constant rows.  The longest shape, whose
    model costs W * tau_max * frames fmaf in numpy, runs fewer and shorter rows: TILE + 1 frames and 1 frame of noise, two
    frames of every other signal"""
    N, W, hop, tau_min, tau_max = shape
    center, pad_mode = option
    rng = np.random.default_rng(N + hop + tau_max + 2 * center + pad_mode)
    la = Launch(shape, center, pad_mode)
    reflect_pad = N // 2 if center and pad_mode == afgpu.MEL_PAD_REFLECT else 0
    heavy = N >= 4096
    counts, asked = [], (TILE + 1, 1) if heavy else (TILE - 1, TILE, TILE + 1, 1)
    for frames in asked:
        n = length_for(shape, center, frames)
        if n <= reflect_pad:                                     # (reflect needs more than pad samples: the next longer row)
            n = reflect_pad + 1
        la.add(rng.standard_normal(n) * 0.3)
        counts.append(la.recs[-1][3])
    if not reflect_pad:
        assert counts == list(asked)
    n5 = max(length_for(shape, center, 2 if heavy else TILE + 1), reflect_pad + 1)
    period = max(2, min(tau_max // 2, (tau_min + tau_max) // 3))
    la.add(tone(RATE / (period + 0.37), n5, rng, 0.01))
    la.add(np.resize(rng.integers(-8, 9, period), n5))
    la.add(np.zeros(n5))
    la.add(np.full(n5, -0.625))
    la.add(rng.standard_normal(n5) * 0.3, la.most(n5) - 1)       # out_frames below the row's frames
    if center and pad_mode == afgpu.MEL_PAD_ZERO and not heavy:
        la.add(rng.standard_normal(max(N // 2 - 3, 1)) * 0.3)    # shorter than the padding
        assert la.recs[-1][3] >= 1
    got, taus = la.run()
    k0 = len(asked)
    if not center:                                               # whole frames: the paths the signals were made for
        assert (la.slab(got, k0)[1].view(np.float32) < 0.1).all() or tau_min == tau_max or period < tau_min
        if tau_min < period and 2 * period < tau_max:
            assert (taus[k0 + 1] == period).all() and (la.slab(got, k0 + 1)[1] == 0).all()
        for k in (k0 + 2, k0 + 3):
            y = la.slab(got, k).view(np.float32)
            assert (y[0] == np.float32(RATE / tau_min)).all() and (y[1] == 1.0).all()
        if tau_max > tau_min:
            assert (la.slab(got, 0)[1].view(np.float32) >= 0.1).all()     # noise: nothing under the threshold


def test_reflect_row_not_longer_than_the_padding_is_refused(gpu):
    la = Launch(SHAPES[0], 1, afgpu.MEL_PAD_REFLECT)
    rng = np.random.default_rng(3)
    la.add(rng.standard_normal(200))
    la.add(rng.standard_normal(32), 1)                           # pad = 32: needs 33 samples
    rec, d_in, before = la.planes()
    with pytest.raises(afgpu.AfgError, match="reflect padding"):
        la.device(rec, d_in, before)
    zero = Launch(SHAPES[0], 1, afgpu.MEL_PAD_ZERO)
    zero.add(rng.standard_normal(200))
    zero.add(rng.standard_normal(32), 1)
    zero.run()


@pytest.mark.parametrize("option", [OPTIONS[0], OPTIONS[1]], ids=OPTION_IDS[:2])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[4]])
def test_a_nan_sample_reaches_exactly_the_frames_over_it(gpu, shape, option):
    N, W, hop, tau_min, tau_max = shape
    center, pad_mode = option
    rng = np.random.default_rng(22)
    n = N + 9 * hop
    for where in (0, n // 2, n - 1):
        x = (rng.standard_normal(n) * 0.3).astype(np.float32)
        x[where] = np.nan
        la = Launch(shape, center, pad_mode)
        la.add(x)
        la.add(rng.standard_normal(N + hop) * 0.3)
        got, _ = la.run()
        F = la.recs[0][3]
        idx = ym.frame_index(la.model, F)
        if pad_mode == afgpu.MEL_PAD_REFLECT:
            idx = np.where(idx < 0, -idx, idx)
            idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
        hit = (idx == where).any(axis=1)                         # the span [start, start + W + tau_max) covers it
        assert hit.any() and not hit.all()
        y = la.slab(got, 0)
        assert (y[:, hit] == ym.NAN_WORD).all() and np.isfinite(y[:, ~hit].view(np.float32)).all()
        assert np.isfinite(la.slab(got, 1).view(np.float32)).all()


def test_twin_rows_and_mixed_launches_give_the_same_bits(gpu):
    rng = np.random.default_rng(21)
    shape = (1024, 512, 160, 32, 320)
    x = tone(123.4, 3000, rng, 0.05)
    la = Launch(shape)
    la.add(x)
    la.add(rng.standard_normal(777) * 0.5)
    la.add(x)
    la.add(rng.standard_normal(2000) * 3.0)
    got, _ = la.run()
    assert (la.slab(got, 0) == la.slab(got, 2)).all()
    # two launches on one output plane: the even records, then the odd ones, each leaving the other's slabs alone
    rec, d_in, before = la.planes()
    d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
    for part in (rec[0::2].copy(), rec[1::2].copy()):
        mixed = la.device(part, d_in, before, d_out=d_out)
    assert (mixed == got).all()


def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu):
    rng = np.random.default_rng(12)
    la = Launch((1024, 512, 160, 32, 320))
    la.add(rng.standard_normal(2000) * 0.5)
    la.add(rng.standard_normal(700) * 0.5)
    rec, d_in, before = la.planes()
    tiles = afgpu.yin_layout(rec, la.prm)
    assert (la.device(rec, d_in, before) != before).any()       # as it stands it runs
    seen = set()

    def refused(change=None, **kw):
        bad = rec.copy()
        if change:
            change(bad)
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        with pytest.raises(afgpu.AfgError) as e:
            la.device(bad, d_in, before, tiles=kw.pop("tiles", tiles), d_out=d_out, **kw)
        assert "invalid argument" in str(e.value) and "afg_yin_hip" in str(e.value)
        seen.add(str(e.value))
        assert (d_out.cpu().numpy().view(np.uint32) == before).all()

    def prm(**kw):
        p = afgpu.yin_params(RATE, 1024, 512, 160, 32, 320)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    refused(out_floats=len(before) - GUARD - 1)                  # the last slab's last float
    refused(in_floats=int(rec[1]["in_off"]) + 699)
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(1, (1 << 64) - 8))
    refused(lambda b: b["first_tile"].__setitem__(1, 0))
    refused(tiles=tiles + 1)
    refused(lambda b: b["out_frames"].__setitem__(1, la.most(700) + 1))
    refused(prm=prm(tau_max=512))
    refused(prm=prm(threshold=float("nan")))
    refused(prm=prm(samplerate=0.0))
    assert len(seen) >= 9


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case):
    """1, 2 and 5 rows, with rows of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(23)
    la = Launch((64, 32, 16, 2, 31), 0)
    for f in record_lengths(TILE)[case]:
        la.add(rng.standard_normal(max(f, 1) * 16 + 64) * 0.5, f)              # (room for more frames than are asked for)
    la.run()


def test_yin_tensor_is_the_kernel_call(gpu):
    """the tensor call: librosa's argument names, the lag helper, valid lengths"""
    rng = np.random.default_rng(5)
    x = np.stack([tone(f, 6000, rng, 0.02) for f in (110.0, 220.5, 83.1, 401.7)]).reshape(2, 2, 6000).astype(np.float32)
    wave = torch.from_numpy(x).cuda()
    y = afgpu.yin_tensor(wave, 16000, 50, 500, frame_length=1024)
    assert tuple(y.shape) == (2, 2, 2, 24)
    p = ym.params(RATE, 1024, 512, 256, 32, 320)
    for i in range(2):
        for c in range(2):
            want, _, _ = ym.yin32(x[i, c], p, 24)
            assert (y[i, c].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    f0 = y[:, :, 0, 4:-4].cpu().numpy()
    assert np.abs(f0 - np.array([[110.0, 220.5], [83.1, 401.7]])[:, :, None]).max() < 1.0
    t, counts = afgpu.yin_tensor(wave, 16000, 50, 500, frame_length=1024, valid=[6000, 1000, 0, 300])
    assert tuple(t.shape) == (2, 2, 2, 24) and list(counts) == [24, 4, 0, 2]
    short = afgpu.yin_tensor(wave[:1, 1:2, :1000].contiguous(), 16000, 50, 500, frame_length=1024)
    assert (t[0, 1, :, :4].cpu().numpy().view(np.uint32) == short[0, 0].cpu().numpy().view(np.uint32)).all()
    assert (t[0, 1, :, 4:] == 0).all() and (t[1, 0] == 0).all() and (t[0, 0] == y[0, 0]).all()
