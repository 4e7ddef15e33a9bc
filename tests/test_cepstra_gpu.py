"""afg_cepstra_hip against tests/cepstra_model.py's float32 restatement, bit for bit as uint32, with the library's own table
(so libm plays no part).  Where the model's value is NaN only NaN-ness is compared.  Every input slab lies between NaN guard
floats and every output between 64 sentinel words, at odd float offsets: a read outside the slab turns outputs into NaN, a
store outside an output kills a sentinel.  Shapes: the smallest at which halo, clamp and tile edges can go wrong."""
import functools

import numpy as np
import pytest
import torch

import afgpu
import cepstra_model as cm
from record_cases import RECORD_CASES, record_lengths
import melspec_model as mm

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 64
TILE = afgpu.CEP_TILE


def frame_list(N):
    return [1, 2, N, 2 * N, 2 * N + 1, TILE - 1, TILE, TILE + 1, TILE + 2 * N, 2 * TILE + 1]


@functools.lru_cache(maxsize=None)
def table(n_ceps, n_mels):
    return afgpu.cep_dct(n_ceps, n_mels, "ortho", 22.0, 1.0)


def slab(rng, n_mels, F):
    return rng.uniform(-10.0, 3.0, (n_mels, F)).astype(np.float32)


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, n_mels, n_ceps, order, N, D=None):
        self.n_mels, self.n_ceps, self.order, self.N = n_mels, n_ceps, order, N
        self.prm = afgpu.cep_params(n_mels, n_ceps, order, N)
        self.D = table(n_ceps, n_mels) if D is None else D
        self.out_rows = (1 + order) * n_ceps
        self.recs, self.slabs, self.in_at, self.out_at = [], [], 0, 0

    def add(self, x):
        x = np.ascontiguousarray(x, np.float32)
        F = x.shape[1]
        self.in_at += GUARD + 1                                  # (65 floats between the slabs: offsets of both parities)
        self.out_at += GUARD + 1
        self.recs.append((self.in_at, self.out_at, F))
        self.slabs.append(x)
        self.in_at += self.n_mels * F
        self.out_at += self.out_rows * F

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.CEP_ROW_DTYPE)
        for k, ((i, o, F), x) in enumerate(zip(self.recs, self.slabs)):
            d_in.view(np.uint32)[i:i + x.size] = x.reshape(-1).view(np.uint32)
            rec[k]["in_off"], rec[k]["out_off"], rec[k]["frames"] = i, o, F
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def model(self, before):
        want = before.copy()
        for (i, o, F), x in zip(self.recs, self.slabs):
            if F:
                want[o:o + self.out_rows * F] = cm.cepstra32(self.D, x, self.order, self.N).reshape(-1).view(np.uint32)
        return want

    def device(self, rec, d_in, before, tiles=None, prm=None, **sizes):
        tiles = afgpu.cep_layout(rec, self.prm) if tiles is None else tiles
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_dct = torch.from_numpy(np.ascontiguousarray(self.D, np.float32).reshape(-1).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        try:
            afgpu.cepstra(len(rec), d_rec, tiles, self.prm if prm is None else prm, d_src, sizes.get("in_floats", len(d_in)), d_dct,
                          sizes.get("dct_floats", self.D.size), d_out, sizes.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = self.last = d_out.cpu().numpy().view(np.uint32)
            assert (d_src.cpu().numpy().view(np.uint32) == d_in.view(np.uint32)).all()       # the input plane is as it was
        return got

    def run(self):
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        want = self.model(before)
        bad = mm.same_bits(got.view(np.float32), want.view(np.float32)).reshape(-1)
        assert bad.size == 0, (len(bad), bad[:8], [hex(v) for v in got[bad[:8]]], [hex(v) for v in want[bad[:8]]])
        assert (got[want == SENTINEL] == SENTINEL).all()                       # (NaN words: compared by value here)
        return got, want

    def out_of(self, plane, k):
        i, o, F = self.recs[k]
        return plane[o:o + self.out_rows * F].view(np.float32).reshape(self.out_rows, F)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_every_length_in_one_launch(gpu, order):
    """Whisper's slab height with 13 coefficients, N = 2: the whole list of lengths, and records without frames between"""
    rng = np.random.default_rng(10 + order)
    la = Launch(80, 13, order, 2)
    for k, F in enumerate(frame_list(2)):
        la.add(slab(rng, 80, F))
        if k % 4 == 1:
            la.add(np.zeros((80, 0), np.float32))
    got, want = la.run()
    assert (got != SENTINEL).sum() == sum((1 + order) * 13 * F for F in frame_list(2))      # exactly the outputs are written


def combos():
    """a few dozen of n_mels x n_ceps x delta_order x N x F, every value of each list in one of them at the least"""
    out, k = [], 0
    for n_mels in (1, 3, 80, 256):
        for n_ceps in sorted({1, min(13, n_mels), n_mels}):
            for order in (0, 1, 2):
                N = (1, 2, 8)[k % 3]
                Fs = frame_list(N)
                out.append((n_mels, n_ceps, order, N, Fs[k % 10], Fs[(k + 5) % 10]))
                k += 7
    return out


@pytest.mark.parametrize("n_mels,n_ceps,order,N,F1,F2", combos())
def test_sampled_shapes(gpu, n_mels, n_ceps, order, N, F1, F2):
    rng = np.random.default_rng(n_mels * 7 + n_ceps * 3 + order + N + F1)
    la = Launch(n_mels, n_ceps, order, N)
    la.add(slab(rng, n_mels, F1))
    la.add(slab(rng, n_mels, F2))
    la.run()


def test_the_widest_window_at_every_length(gpu):
    """N = 8 with both delta planes: a halo of 16 frames, longer than most of these records"""
    rng = np.random.default_rng(3)
    la = Launch(80, 40, 2, 8)
    for F in frame_list(8):
        la.add(slab(rng, 80, F))
    la.run()


def test_the_same_slab_gives_the_same_bits_wherever_it_stands(gpu):
    rng = np.random.default_rng(4)
    x = slab(rng, 80, 2 * TILE + 1)
    la = Launch(80, 13, 2, 2)
    la.add(x)
    la.add(slab(rng, 80, 7))
    la.add(x)
    got, _ = la.run()
    assert (la.out_of(got, 0).view(np.uint32) == la.out_of(got, 2).view(np.uint32)).all()


def reads(F, N, hit):
    """the frames whose delta reads a frame of `hit`: some min(t + n, F - 1) or max(t - n, 0), n = 1 .. N, is in it"""
    t = np.arange(F)
    out = np.zeros(F, bool)
    for n in range(1, N + 1):
        out |= hit[np.minimum(t + n, F - 1)] | hit[np.maximum(t - n, 0)]
    return out


@pytest.mark.parametrize("N", [1, 2, 8])
def test_a_nan_frame_reaches_exactly_the_frames_that_read_it(gpu, N):
    F = 2 * TILE + 1
    rng = np.random.default_rng(20 + N)
    la = Launch(80, 13, 2, N)
    at = [0, F - 1, TILE - 1, TILE]                              # both ends, and either side of a tile edge
    for t in at:
        x = slab(rng, 80, F)
        x[rng.integers(0, 80), t] = np.nan
        la.add(x)
    got, _ = la.run()
    for k, t in enumerate(at):
        nan = np.isnan(la.out_of(got, k)).reshape(3, 13, F)
        hit0 = np.zeros(F, bool)
        hit0[t] = True
        hit1 = reads(F, N, hit0)
        hit2 = reads(F, N, hit1)
        for plane, hit in enumerate((hit0, hit1, hit2)):
            assert (nan[plane] == hit[None, :]).all(), (t, plane)
        assert hit1[t] == (t in (0, F - 1)) and hit1.sum() == (N + 1 if t in (0, F - 1) else 2 * N)


def test_every_device_side_refusal_writes_nothing(gpu):
    rng = np.random.default_rng(6)
    la = Launch(80, 13, 2, 2)
    for F in (70, 0, 5):
        la.add(slab(rng, 80, F))
    rec, d_in, before = la.planes()
    tiles = afgpu.cep_layout(rec, la.prm)
    seen = set()

    def refused(change=None, **kw):
        bad = rec.copy()
        if change:
            change(bad)
        with pytest.raises(afgpu.AfgError) as e:
            la.device(bad, d_in, before, kw.pop("tiles", tiles), **kw)
        assert str(e.value) not in seen
        seen.add(str(e.value))
        assert (la.last == before).all()                         # the output plane after the refused call: every sentinel

    refused(tiles=tiles + 1)
    refused(in_floats=len(d_in) - GUARD - 1)
    refused(out_floats=len(before) - GUARD - 1)
    refused(dct_floats=13 * 80 - 1)
    refused(lambda b: b["first_tile"].__setitem__(2, 1))
    refused(lambda b: b["reserved"].__setitem__(0, 1))
    refused(lambda b: b["out_off"].__setitem__(0, 2 ** 64 - 8))
    refused(lambda b: b["frames"].__setitem__(2, 6))             # one frame more: the slab and the output leave their planes' ends
    refused(prm=afgpu.cep_params(80, 13, 2, 9))
    got = la.device(rec, d_in, before)                           # the records as they were: the launch runs
    assert (got != SENTINEL).sum() == 39 * 75


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_records_without_tiles(gpu, case):
    """1, 2 and 5 records, with records of no frames first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(31)
    la = Launch(40, 13, 1, 2)
    for F in record_lengths(TILE)[case]:
        la.add(slab(rng, 40, F))
    la.run()
