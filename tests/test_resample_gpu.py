"""afg_resample_hip against tests/resample_model.py's float32 restatement, bit for bit, with the library's own tables.  Where
the model's value is NaN only NaN-ness is compared.  Every input row lies between NaN guard floats and every output row
between sentinel words: a read outside [0, in_frames) turns outputs into NaN, a store outside a row kills a sentinel."""
import itertools

import numpy as np
import pytest
import torch

import afgpu
import resample_model as rm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
# per-lane phases; L == 1; going up; no filter; a table read through L2 (544 000 floats); the widest window of the audio
# rates (tiles of 256); a ratio whose window does not fit the tile at all (computed from global memory)
PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (16000, 16000), (44101, 16000), (96000, 8000), (44100, 700)]


def tile_frames(M, L, W):
    """include/afg.h: afg_resample_layout"""
    n = 1024
    while W and n > 64 and n * M // L + 2 * W + 1 > 4096:
        n //= 2
    return n


class Launch:
    """records of several rate pairs over one input plane, one table plane and one output plane"""

    def __init__(self, rng):
        self.rng, self.recs, self.inputs, self.tables, self.table_at = rng, [], [], [], {}
        self.in_at, self.out_at, self.taps_at = 0, 0, 0

    def table(self, pair):
        if pair not in self.table_at:
            taps, M, L, W = afgpu.resample_taps(*pair)
            self.table_at[pair] = (self.taps_at + 5, taps, M, L, W)
            self.tables.append((self.taps_at + 5, taps.reshape(-1)))
            self.taps_at += 5 + taps.size
        return self.table_at[pair]

    def add(self, pair, in_rows, in_frames, out_frames, in_frame0, specials=False):
        taps_off, taps, M, L, W = self.table(pair)
        stride = in_frames + GUARD + int(self.rng.integers(0, 3))
        self.in_at += GUARD
        rows = (self.rng.standard_normal((in_rows, in_frames)) * 0.5).astype(np.float32)
        if specials and in_frames:
            w = rows.view(np.uint32)
            w[:, ::7] = self.rng.integers(0, 1 << 32, w[:, ::7].shape, dtype=np.uint64).astype(np.uint32)
            w[0, :4] = [0x7fc12345, 0x7f800000, 0xff800000, 0x80000000][:min(4, in_frames)]
        self.inputs.append((self.in_at, stride, rows))
        self.out_at += GUARD
        self.recs.append(dict(in_off=self.in_at, in_stride=stride, in_frame0=in_frame0, out_off=self.out_at, taps_off=taps_off,
                              in_rows=in_rows, in_frames=in_frames, out_frames=out_frames, M=M, L=L, W=W, rows=rows, taps=taps))
        self.in_at += in_rows * stride
        self.out_at += out_frames

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        for at, stride, rows in self.inputs:
            for r in range(rows.shape[0]):
                d_in.view(np.uint32)[at + r * stride:at + r * stride + rows.shape[1]] = rows[r].view(np.uint32)
        d_taps = np.full(self.taps_at + 5, np.nan, np.float32)
        for at, t in self.tables:
            d_taps[at:at + t.size] = t
        rec = np.zeros(len(self.recs), afgpu.RESAMPLE_ROW_DTYPE)
        for k, r in enumerate(self.recs):
            for name in rec.dtype.names:
                if name != "first_tile":
                    rec[k][name] = r[name]
        return rec, d_in, d_taps, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def run(self):
        rec, d_in, d_taps, before = self.planes()
        tiles = afgpu.resample_layout(rec)
        got = device(rec, tiles, d_in, d_taps, before)
        want = before.copy()
        for r in self.recs:
            x = rm.mix(r["rows"]) if r["in_frames"] else np.zeros(0, np.float32)
            y = rm.resample32(x, r["taps"], r["M"], r["L"], r["W"], r["out_frames"], r["in_frame0"])
            want[r["out_off"]:r["out_off"] + r["out_frames"]] = y.view(np.uint32)
        bad = rm.same_bits(got.view(np.float32), want.view(np.float32)).reshape(-1)
        assert bad.size == 0, (len(bad), bad[:8], [hex(v) for v in got[bad[:8]]], [hex(v) for v in want[bad[:8]]])
        assert (got[want == SENTINEL] == SENTINEL).all()                       # (NaN words: compared by value here)
        return got, want


def device(rec, tiles, d_in, d_taps, before, **sizes):
    d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
    d_tab = torch.from_numpy(d_taps.view(np.int32).copy()).cuda()
    d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
    try:
        afgpu.resample(len(rec), d_rec, tiles, d_src, sizes.get("in_floats", len(d_in)), d_tab, sizes.get("taps_floats", len(d_taps)),
                       d_out, sizes.get("out_floats", len(before)))
    finally:
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
    return got


def cases(pair):
    """in_rows 1, 2, 3, 6 x out_frames 1, 255, one tile plus 1, 5000, with in_frame0 cycling through 0, inside the row, W - 1
    before its end, its end and past it; then a row without input"""
    M, L, W, _ = rm.shape(*pair)
    tile = tile_frames(M, L, W)
    for n, (rows, out_frames) in enumerate(itertools.product((1, 2, 3, 6), (1, 255, tile + 1, 5000))):
        in_frames = out_frames * M // L + 40
        f0 = (0, 17, in_frames - max(W - 1, 0), in_frames, in_frames + 3 * W + 9)[n % 5]
        yield rows, in_frames, out_frames, f0
    yield 2, 0, 300, 0
    yield 1, 0, 1, 5


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_rows_of_every_shape(gpu, pair):
    la = Launch(np.random.default_rng(pair[0] + pair[1]))
    for rows, in_frames, out_frames, f0 in cases(pair):
        la.add(pair, rows, in_frames, out_frames, f0, specials=pair[0] == pair[1])
    # ... and a negative in_frame0: the row begins inside the output
    la.add(pair, 2, 900, 700, -33, specials=pair[0] == pair[1])
    got, want = la.run()
    assert (want != SENTINEL).any() and np.isfinite(want.view(np.float32)[want != SENTINEL]).any()
    if pair[0] == pair[1]:
        assert np.isnan(want[want != SENTINEL].view(np.float32)).any()           # the NaN words did travel


def test_records_of_different_rates_in_one_launch(gpu):
    la = Launch(np.random.default_rng(9))
    for n, pair in enumerate(PAIRS[:4] + [(22050, 16000), (44100, 48000)] + PAIRS[:4]):
        la.add(pair, 1 + n % 3, 3000 + 7 * n, 1500 + 333 * n, (0, 11, 2900)[n % 3], specials=pair[0] == pair[1])
        if n % 4 == 1:
            la.add(pair, 2, 0, 77, 0)
    la.run()


def test_a_record_that_leaves_a_plane_is_refused_and_nothing_is_written(gpu):
    la = Launch(np.random.default_rng(10))
    la.add((44100, 16000), 2, 3000, 1000, 0)
    la.add((16000, 16000), 1, 500, 400, 0)
    rec, d_in, d_taps, before = la.planes()
    tiles = afgpu.resample_layout(rec)
    assert (device(rec, tiles, d_in, d_taps, before) != before).any()             # as it stands it runs
    seen = set()

    def refused(change=None, tiles_=None, **sizes):
        bad = rec.copy()
        if change:
            change(bad)
        with pytest.raises(afgpu.AfgError) as e:
            device(bad, tiles if tiles_ is None else tiles_, d_in, d_taps, before, **sizes)
        assert "invalid argument" in str(e.value)
        seen.add(str(e.value))
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            with pytest.raises(afgpu.AfgError):
                afgpu.resample(len(bad), torch.from_numpy(bad.view(np.uint8).copy()).cuda(), tiles if tiles_ is None else tiles_,
                               torch.from_numpy(d_in.view(np.int32).copy()).cuda(), sizes.get("in_floats", len(d_in)),
                               torch.from_numpy(d_taps.view(np.int32).copy()).cuda(), sizes.get("taps_floats", len(d_taps)), d_out,
                               sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint32) == before).all()

    refused(out_floats=len(before) - GUARD - 1)                                    # the last row's last float
    refused(in_floats=int(rec[1]["in_off"]) + 499)
    refused(taps_floats=int(rec[0]["taps_off"]) + 160 * 34 - 1)
    refused(lambda b: b["in_stride"].__setitem__(0, len(d_in)))
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(1, (1 << 64) - 8))
    refused(lambda b: b["first_tile"].__setitem__(1, 0))
    refused(tiles_=tiles + 1)
    refused(lambda b: b["W"].__setitem__(0, 0))                                    # no filter, but M and L are not 1
    refused(lambda b: b["L"].__setitem__(0, 0))
    refused(lambda b: b["in_rows"].__setitem__(0, 0))
    refused(lambda b: b["in_frame0"].__setitem__(0, 1 << 61))
    assert len(seen) >= 8


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_rows_without_tiles(gpu, case):
    """1, 2 and 5 rows, with rows of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    pair = (44100, 16000)
    M, L, W, _ = rm.shape(*pair)
    la = Launch(np.random.default_rng(19))
    for k, out_frames in enumerate(record_lengths(tile_frames(M, L, W))[case]):
        la.add(pair, 1 + k % 2, out_frames * M // L + 40, out_frames, (0, 17)[k % 2])
    la.run()
