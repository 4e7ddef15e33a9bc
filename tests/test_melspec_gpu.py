"""afg_melspec_hip against tests/melspec_model.py's float32 restatement, bit for bit as uint32, with the library's own tables
(so libm plays no part).  Where the model's value is NaN only NaN-ness is compared.  Every input row lies between NaN guard
floats and every output slab between sentinel words: a read outside the row turns outputs into NaN, a store outside a slab
kills a sentinel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import afgpu
import melspec_model as mm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
# n_fft, win_length, hop, n_mels, center: K = 400, 402 columns and 80 mels, none a multiple of the MFMA tile in N; a
# zero-padded window; the minimal shape; the largest allowed
SHAPES = [(400, 400, 160, 80, True), (512, 400, 128, 23, True), (16, 16, 1, 1, True), (2048, 2048, 2048, 256, False)]
SAMPLERATE = 16000


def tile_frames(n_fft, win, n_mels):
    """include/afg.h: afg_mel_layout (csrc/melspec.hip: geo_of)"""
    k4 = (win + 3) // 4 * 4
    pitch = k4 if k4 % 8 == 4 else k4 + 4
    mel16 = (n_mels + 15) // 16 * 16
    f = 64
    while f > 16 and (max(f * pitch, mel16 * (f + 4)) + 64 * (f + 16)) * 4 > 152 * 1024:
        f //= 2
    return f


@functools.lru_cache(maxsize=None)
def tables(n_fft, win, n_mels):
    basis = afgpu.mel_basis(n_fft, win)
    bank = afgpu.mel_filters(SAMPLERATE, n_fft, n_mels)
    Cf, Sf = mm.split_basis(basis, n_fft)
    return basis, bank, Cf, Sf


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, shape, pad_mode, out_kind=afgpu.MEL_POWER, log_floor=0.0, bank=None):
        self.n_fft, self.win, self.hop, self.n_mels, self.center = shape
        self.pad_mode, self.out_kind, self.log_floor = pad_mode, out_kind, log_floor
        self.prm = afgpu.mel_params(self.n_fft, self.hop, self.n_mels, self.win, self.center, pad_mode, out_kind, log_floor)
        self.basis, lib_bank, self.Cf, self.Sf = tables(self.n_fft, self.win, self.n_mels)
        self.bank = lib_bank if bank is None else bank
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

    def model(self, before):
        """the output plane as the model has it, AFG_MEL_POWER"""
        want = before.copy()
        for (i, o, n, f), x in zip(self.recs, self.rows):
            if f:
                _, mel = mm.melspec32(x, self.Cf, self.Sf, self.bank, self.n_fft, self.win, self.hop, self.center, self.pad_mode, f)
                want[o:o + self.n_mels * f] = mel.reshape(-1).view(np.uint32)
        return want

    def device(self, rec, d_in, before, tiles=None, **sizes):
        tiles = afgpu.mel_layout(rec, self.prm) if tiles is None else tiles
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_bas = torch.from_numpy(self.basis.reshape(-1).copy()).cuda()
        d_fil = torch.from_numpy(np.ascontiguousarray(self.bank, np.float32).reshape(-1).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            afgpu.melspec(len(rec), d_rec, tiles, self.prm, d_src, sizes.get("in_floats", len(d_in)), d_bas, sizes.get("basis_floats", self.basis.size),
                          d_fil, sizes.get("filters_floats", self.bank.size), d_out, sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint32)
        return got

    def run(self):
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        want = self.model(before)
        bad = mm.same_bits(got.view(np.float32), want.view(np.float32)).reshape(-1)
        assert bad.size == 0, (len(bad), bad[:8], [hex(v) for v in got[bad[:8]]], [hex(v) for v in want[bad[:8]]])
        assert (got[want == SENTINEL] == SENTINEL).all()                       # (NaN words: compared by value here)
        return got, want


@pytest.mark.parametrize("pad_mode", [afgpu.MEL_PAD_REFLECT, afgpu.MEL_PAD_ZERO], ids=["reflect", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}-{s[3]}")
def test_rows_of_every_shape(gpu, shape, pad_mode):
    n_fft, win, hop, n_mels, center = shape
    rng = np.random.default_rng(n_fft + hop + pad_mode)
    la = Launch(shape, pad_mode)
    pad = n_fft // 2 if center else 0
    F = tile_frames(n_fft, win, n_mels)
    assert F == (16 if n_fft == 2048 else 64)
    noise = lambda n: rng.standard_normal(n) * 0.5
    la.add(noise(1600 if n_fft == 400 else 3 * n_fft + 5))
    la.add(noise(max(pad + 1, 0 if center else n_fft)))                          # reflect's minimum (without centre: one frame)
    one_more = F * hop + n_fft - 2 * pad                                         # exactly one tile of frames plus one
    la.add(noise(one_more))
    assert la.recs[-1][3] == F + 1
    la.add(np.zeros(0), 0 if (pad_mode == afgpu.MEL_PAD_REFLECT or not center) else None)     # no samples: zero padding alone makes a frame
    long_ = noise(5 * hop + n_fft)
    la.add(long_, la.most(len(long_)) - 2)                                       # out_frames < max_frames
    got, want = la.run()
    assert (want != SENTINEL).any() and (want.view(np.float32)[want != SENTINEL] > 0).any()
    if pad_mode == afgpu.MEL_PAD_ZERO and center:
        i, o, n, f = la.recs[3]
        assert (n, f) == (0, 1) and (got[o:o + n_mels] == 0).all()                # the frame of an empty row: +0.0f


def test_infinity_and_nan_travel_as_the_model_says(gpu):
    shape = SHAPES[0]
    la = Launch(shape, afgpu.MEL_PAD_REFLECT)
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(4000) * 0.5).astype(np.float32)
    x[1700] = np.inf
    x[3100] = np.nan
    la.add(x)
    la.add(rng.standard_normal(900) * 0.5)
    got, want = la.run()
    w = want.view(np.float32)[want != SENTINEL]
    assert np.isnan(w).any() and np.isfinite(w).any()


def test_a_callers_own_bank_with_negative_weights(gpu):
    shape = SHAPES[1]
    rng = np.random.default_rng(8)
    bank = rng.standard_normal((shape[3], shape[0] // 2 + 1)).astype(np.float32)
    la = Launch(shape, afgpu.MEL_PAD_ZERO, bank=bank)
    la.add(rng.standard_normal(2000) * 0.5)
    la.run()


def ulps(got, ref64):
    """|got - ref| in float32 ulps of the result"""
    ref32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / ulp


@pytest.mark.parametrize("log_floor", [0.0, 1e-3])
def test_log10_within_three_ulp_and_the_floor_exactly(gpu, log_floor):
    """AFG_MEL_LOG10 against float64 log10 of the model's float32 mel: 3 float32 ulp, OpenCL's bound for log10, which the ROCm
    device library states it meets.  A silent row is the floor exactly."""
    shape = SHAPES[0]
    rng = np.random.default_rng(11)
    la = Launch(shape, afgpu.MEL_PAD_REFLECT, afgpu.MEL_LOG10, log_floor)
    la.add(rng.standard_normal(6000) * 0.5)
    la.add(rng.standard_normal(3000) * 1e-4)
    la.add(np.zeros(1000))
    rec, d_in, before = la.planes()
    got = la.device(rec, d_in, before)
    power = la.model(before)
    assert (got[power == SENTINEL] == SENTINEL).all()
    worst = 0.0
    for (i, o, n, f) in la.recs:
        mel = power[o:o + la.n_mels * f].view(np.float32)
        ref = mm.log10_64(mel, log_floor)
        y = got[o:o + la.n_mels * f].view(np.float32)
        assert np.isfinite(y).all()
        worst = max(worst, float(ulps(y, ref).max()))
    print(f"log10f: worst error {worst:.3f} ulp")
    assert worst <= 3.0
    i, o, n, f = la.recs[2]
    floor32 = np.float32(log_floor if log_floor else 1e-10)
    silent = got[o:o + la.n_mels * f].view(np.float32)
    assert (silent.view(np.uint32) == silent.view(np.uint32)[0]).all()
    assert ulps(silent[:1], np.log10(np.array([floor32], np.float64)))[0] <= 3.0
    if log_floor:
        assert (got[la.recs[1][1]:la.recs[1][1] + 8].view(np.float32) >= silent[0]).all()


def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu):
    shape = SHAPES[0]
    rng = np.random.default_rng(12)
    la = Launch(shape, afgpu.MEL_PAD_REFLECT)
    la.add(rng.standard_normal(2000) * 0.5)
    la.add(rng.standard_normal(700) * 0.5)
    rec, d_in, before = la.planes()
    tiles = afgpu.mel_layout(rec, la.prm)
    assert (la.device(rec, d_in, before) != before).any()                          # as it stands it runs
    seen = set()

    def refused(change=None, tiles_=None, prm=None, **sizes):
        bad = rec.copy()
        if change:
            change(bad)
        keep = la.prm
        try:
            if prm is not None:
                la.prm = prm
            d_rec = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
            d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
            d_bas = torch.from_numpy(la.basis.reshape(-1).copy()).cuda()
            d_fil = torch.from_numpy(la.bank.reshape(-1).copy()).cuda()
            d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
            try:
                with pytest.raises(afgpu.AfgError) as e:
                    afgpu.melspec(len(bad), d_rec, tiles if tiles_ is None else tiles_, la.prm, d_src, sizes.get("in_floats", len(d_in)), d_bas,
                                  sizes.get("basis_floats", la.basis.size), d_fil, sizes.get("filters_floats", la.bank.size), d_out,
                                  sizes.get("out_floats", len(before)))
            finally:
                torch.cuda.synchronize()
            assert "invalid argument" in str(e.value)
            seen.add(str(e.value))
            assert (d_out.cpu().numpy().view(np.uint32) == before).all()
        finally:
            la.prm = keep

    refused(out_floats=len(before) - GUARD - 1)                                    # the last slab's last float
    refused(in_floats=int(rec[1]["in_off"]) + 699)
    refused(basis_floats=la.basis.size - 1)
    refused(filters_floats=la.bank.size - 1)
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(1, (1 << 64) - 8))
    refused(lambda b: b["first_tile"].__setitem__(1, 0))
    refused(tiles_=tiles + 1)
    refused(lambda b: b["out_frames"].__setitem__(1, la.most(700) + 1))
    refused(lambda b: b["in_frames"].__setitem__(1, 200))                          # reflect with in_frames <= pad (and too many frames)
    refused(prm=afgpu.mel_params(400, 160, 257))
    assert len(seen) >= 9


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case):
    """1, 2 and 5 rows, with rows of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    shape = (16, 16, 1, 1, True)
    n_fft, hop = shape[0], shape[2]
    rng = np.random.default_rng(23)
    la = Launch(shape, afgpu.MEL_PAD_ZERO)
    for f in record_lengths(tile_frames(16, 16, 1))[case]:
        la.add(rng.standard_normal(max(f, 1) * hop + n_fft) * 0.5, f)          # (room for more frames than are asked for)
    la.run()
