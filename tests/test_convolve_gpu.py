"""afg_convolve_hip and afg_convolve_bank_hip against tests/convolve_model.py: the direct path bit for bit against the float32
restatement, the FFT path inside the interval of the float64 definition, none left out.  The harness is
tests/test_istft_gpu.py's: rows and bank kernels lie between NaN guard floats, outputs, spectra and work planes between
sentinel words -- a read outside a record turns samples into NaN, a store outside kills a sentinel.  Locality and order are
tested by their consequences.  The largest share of the interval used is printed by test_fft_dense_cases."""
import numpy as np
import pytest
import torch

import afgpu
import convolve_model as cm

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
EDGE = 4                                                         # sentinel words round the spectra and the work plane (they stay 8-byte aligned)
B, TILE, SPEC, TABLE = cm.B, cm.DIRECT_TILE, cm.SPEC_FLOATS, cm.TABLE_FLOATS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Bank:
    """kernels between NaN guards on the device, transformed once; the spectra between sentinels"""

    def __init__(self, kernels):
        self.h = [np.ascontiguousarray(h, np.float32) for h in kernels]
        self.rec = np.zeros(len(self.h), afgpu.CONV_KERNEL_DTYPE)
        at, parts = 0, []
        for i, h in enumerate(self.h):
            at += GUARD
            self.rec[i]["bank_off"], self.rec[i]["taps"] = at, len(h)
            at += len(h)
        plane = np.full(at + GUARD, np.nan, np.float32)
        for r, h in zip(self.rec, self.h):
            plane[int(r["bank_off"]):int(r["bank_off"]) + len(h)] = h
        self.spec_floats = afgpu.convolve_bank_layout(self.rec)
        self.bank_floats = len(plane)
        self.d_rec = torch.from_numpy(self.rec.view(np.uint8).copy()).cuda()
        self.d_bank = torch.from_numpy(plane).cuda()
        self.d_spec_all = torch.from_numpy(np.full(self.spec_floats + 2 * EDGE, SENTINEL, np.uint32).view(np.int32)).cuda()
        self.d_spec = self.d_spec_all[EDGE:EDGE + self.spec_floats].view(torch.float32)
        afgpu.convolve_bank(len(self.h), self.d_rec, self.d_bank, self.bank_floats, self.d_spec, self.spec_floats)
        torch.cuda.synchronize()
        self.spec0 = self.d_spec_all.cpu().numpy().view(np.uint32).copy()
        assert (self.spec0[:EDGE] == SENTINEL).all() and (self.spec0[-EDGE:] == SENTINEL).all()
        body = self.spec0[EDGE:-EDGE].view(np.float32)
        assert (bits(body[:TABLE]) == bits(afgpu.mel_fft_tables(2048, 1)[1:])).all() and not np.isnan(body).any()

    def unchanged(self):
        return (self.d_spec_all.cpu().numpy().view(np.uint32) == self.spec0).all()


class Launch:
    """records over one input plane and one output plane, against one bank"""

    def __init__(self, bank, direct_max=128):
        self.bank, self.prm, self.direct_max = bank, afgpu.convolve_params(direct_max), direct_max
        self.recs, self.xs, self.in_at, self.out_at, self.intervals = [], [], 0, 0, {}

    def add(self, x, kernel, first=None, count=None, mode="full"):
        x = np.ascontiguousarray(x, np.float32)
        taps = len(self.bank.h[kernel])
        if first is None:
            first, count = cm.mode_range(mode, len(x), taps)
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, len(x), kernel, first, count))
        self.xs.append(x)
        self.in_at += len(x)
        self.out_at += count
        return len(self.recs) - 1

    def is_direct(self, k):
        return len(self.bank.h[self.recs[k][3]]) <= self.direct_max

    def run(self, only=None):
        """launches the records (or those of `only`); returns the output words"""
        keep = list(range(len(self.recs))) if only is None else list(only)
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(keep), afgpu.CONV_ROW_DTYPE)
        for q, k in enumerate(keep):
            i, o, frames, kernel, first, count = self.recs[k]
            d_in[i:i + frames] = self.xs[k]
            rec[q] = (i, o, 0, 0, frames, kernel, first, count)
        before = np.full(self.out_at + GUARD, SENTINEL, np.uint32)
        tiles, work = afgpu.convolve_layout(rec, self.bank.rec, self.prm)
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        d_work_all = torch.from_numpy(np.full(work + 2 * EDGE, SENTINEL, np.uint32).view(np.int32)).cuda()
        d_work = d_work_all[EDGE:EDGE + work].view(torch.float32) if work else d_work_all[EDGE:].view(torch.float32)
        try:
            afgpu.convolve(len(rec), d_rec, tiles, self.bank.d_rec, len(self.bank.h), self.prm, d_src, len(d_in), self.bank.d_bank,
                           self.bank.bank_floats, self.bank.d_spec, self.bank.spec_floats, d_work, work, d_out, len(before))
        finally:
            torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        w = d_work_all.cpu().numpy().view(np.uint32)
        assert (w[:EDGE] == SENTINEL).all() and (w[EDGE + work:] == SENTINEL).all()
        written = np.zeros(len(before), bool)
        for k in keep:
            written[self.recs[k][1]:self.recs[k][1] + self.recs[k][5]] = True
        assert (got[~written] == SENTINEL).all()
        assert self.bank.unchanged()
        return got

    def row(self, got, k):
        return got[self.recs[k][1]:self.recs[k][1] + self.recs[k][5]].view(np.float32)

    def want32(self, k):
        i, o, frames, kernel, first, count = self.recs[k]
        return cm.direct32(self.xs[k], self.bank.h[kernel], first, count)

    def interval(self, k):
        if k not in self.intervals:
            i, o, frames, kernel, first, count = self.recs[k]
            self.intervals[k] = cm.interval(self.xs[k], self.bank.h[kernel], first, count)
        return self.intervals[k]

    def check(self, got, skip=()):
        """direct rows bit for bit, FFT rows inside their interval; returns the largest share of an interval used"""
        used = 0.0
        for k in range(len(self.recs)):
            if k in skip or self.recs[k][5] == 0:
                continue
            y = self.row(got, k)
            if self.is_direct(k):
                want = self.want32(k)
                bad = np.flatnonzero(bits(y) != bits(want))
                assert bad.size == 0, (k, self.recs[k], len(bad), bad[:4].tolist(), y[bad[:4]].tolist(), want[bad[:4]].tolist())
            else:
                lo, hi, mid = self.interval(k)
                bad = cm.outside(y, lo, hi)
                assert bad.size == 0, (k, self.recs[k], len(bad), bad[:4].ravel().tolist(), [(float(y[b[0]]), float(lo[b[0]]), float(hi[b[0]])) for b in bad[:4]])
                used = max(used, cm.used_fraction(y, lo, hi, mid))
        return used


def decaying(rng, taps):
    return (rng.standard_normal(taps) * np.exp(-3.0 * np.arange(taps) / taps)).astype(np.float32)


DIRECT_TAPS = [1, 2, 3, 63, 64, 65, 127, 128]


@pytest.mark.parametrize("taps", DIRECT_TAPS)
def test_direct_path_bit_for_bit(gpu, taps):
    rng = np.random.default_rng(taps)
    bank = Bank([rng.standard_normal(taps), np.ones(taps), -rng.random(taps)])
    la = Launch(bank)
    sizes = sorted({1, 2, max(1, taps - 1), taps, TILE - 1, TILE, TILE + 1, 2 * TILE + 5})
    for q, frames in enumerate(sizes):
        la.add(rng.standard_normal(frames), q % 3)                           # noise, "full"
    imp = np.zeros(TILE + 1, np.float32)
    imp[[0, 77, TILE]] = [1, -2, 3]
    la.add(imp, 0)
    la.add(np.ones(2 * TILE + 5), 1)
    x = rng.standard_normal(2 * TILE + 5).astype(np.float32)
    for first in range(8):                                                    # every out_first % 4, and every alignment of the output with it
        la.add(x, 0, first, len(x) + taps - 1 - first - (first & 1))
    la.add(x, 0, mode="same")
    z = np.zeros(300, np.float32)                                            # signed zeros: +0.0 out whatever the signs in
    z[::2] = -0.0
    la.add(z, 2)
    la.add(z, 1)
    z2 = x[:300].copy()
    z2[::3] = -0.0
    la.add(z2, 2)
    la.add(x[:10], 0, 3 if taps > 3 else 0, 0)                                # no output: nothing read, nothing written
    got = la.run()
    la.check(got)
    n = len(la.recs)
    assert not np.signbit(la.row(got, n - 4)).any() and not la.row(got, n - 4).any() and not np.signbit(la.row(got, n - 3)).any()


def sparse_kernel(P, rng):
    h = np.zeros(P * B, np.float32)
    for p in range(P):
        h[p * B], h[p * B + B - 1] = rng.choice([-1.0, 1.0], 2)
    return h


@pytest.mark.parametrize("P", [1, 2, 5, 64])
def test_fft_structural_cases(gpu, P):
    rng = np.random.default_rng(P)
    bank = Bank([sparse_kernel(P, rng)])
    la = Launch(bank)
    for frames in ([1500] if P == 64 else [2048 + 1, 3 * B + 7]):
        edges = [e for e in (0, 1023, 1024, 2047) if e < frames - 1] + [frames - 1]
        x = np.zeros(frames, np.float32)
        x[edges] = rng.choice([-1.0, 1.0], len(edges))
        la.add(x, 0)
        for e in edges:                                                       # a single impulse at each of them
            x = np.zeros(frames, np.float32)
            x[e] = 1.0
            la.add(x, 0)
    for k in range(len(la.recs)):                                             # the interval is far below the unit-sized outputs
        lo, hi, mid = la.interval(k)
        assert (hi - lo).max() / 2 < 0.01 and np.abs(mid).max() >= 1.0
        assert (np.abs(mid - np.rint(mid)) < 1e-9).all()
    got = la.run()
    la.check(got)
    for k in range(len(la.recs)):                                             # so rounding gives the integers back: nothing dropped, doubled or shifted
        assert (np.rint(la.row(got, k)) == np.rint(la.interval(k)[2])).all()


FFT_TAPS = [129, 1023, 1024, 1025, 2048, 2049, 5000]
USED = {}


@pytest.mark.parametrize("taps", FFT_TAPS)
def test_fft_dense_cases(gpu, taps):
    rng = np.random.default_rng(taps)
    bank = Bank([decaying(rng, taps)])
    la = Launch(bank)
    for frames in (1, 1023, 1024, 1025, 2049, 3 * B + 7):
        x = rng.standard_normal(frames).astype(np.float32)
        la.add(x, 0, mode="full")
        la.add(x, 0, mode="same")
        la.add(x, 0, min(taps - 1, 517), frames)                              # "head", out_first in the middle of a block
    x = rng.standard_normal(3 * B + 7).astype(np.float32)
    la.add(x, 0, B + 300, 1500)                                               # a range in the middle of the line
    la.add(x, 0, 2 * B, B)                                                    # one whole block
    la.add(x, 0, 77, 0)
    used = la.check(la.run())
    USED[taps] = used
    print(f"\nconvolve: taps {taps}: largest share of the interval used {used:.3g} (over the suite so far {max(USED.values()):.3g})")
    assert 0.0 < used <= 1.0


def test_direct_max_0_sends_short_kernels_through_the_fft(gpu):
    rng = np.random.default_rng(11)
    taps = list(range(1, 129))
    bank = Bank([rng.standard_normal(t) for t in taps])
    x = rng.standard_normal(B + 300).astype(np.float32)
    fft, direct = Launch(bank, 0), Launch(bank, 128)
    for la in (fft, direct):
        for k in range(len(taps)):
            la.add(x, k)
    got_f, got_d = fft.run(), direct.run()
    assert not any(fft.is_direct(k) for k in range(len(taps))) and all(direct.is_direct(k) for k in range(len(taps)))
    used = fft.check(got_f)
    direct.check(got_d)
    print(f"\nconvolve: direct_max 0, taps 1 .. 128: largest share of the interval used {used:.3g}")
    for k, t in enumerate(taps):                                              # round the same values: the direct sum is within taps u sum |h| |x| of them
        lo, hi, mid = fft.interval(k)
        slack = t * cm.U * np.convolve(np.abs(x.astype(np.float64)), np.abs(bank.h[k].astype(np.float64)))
        d = direct.row(got_d, k).astype(np.float64)
        assert (d >= lo - slack).all() and (d <= hi + slack).all()


def test_locality(gpu):
    rng = np.random.default_rng(3)
    bank = Bank([decaying(rng, 2500), rng.standard_normal(100), decaying(rng, 700)])
    x, x2 = rng.standard_normal(3 * B + 7).astype(np.float32), rng.standard_normal(5000).astype(np.float32)
    la = Launch(bank)
    a = la.add(x, 0)                       # FFT
    b = la.add(x2, 1)                      # direct
    la.add(rng.standard_normal(777), 2)
    c = la.add(x, 0)                       # the twin of a, elsewhere in the batch
    d = la.add(x2, 1)
    e = la.add(x, 0, 1000, 2000)           # ranges of a's line that overlap each other
    f = la.add(x, 0, 2500, 1200)
    g = la.add(x2, 1, 37, 4500)
    got = la.run()
    la.check(got)
    A = bits(la.row(got, a))
    assert (A == bits(la.row(got, c))).all() and (bits(la.row(got, b)) == bits(la.row(got, d))).all()
    assert (bits(la.row(got, e)) == A[1000:3000]).all() and (bits(la.row(got, f)) == A[2500:3700]).all()
    assert (bits(la.row(got, g)) == bits(la.row(got, b))[37:4537]).all()
    # other launches: the FFT rows alone, the direct rows alone, one record alone
    for only in ([a, c, e, f, 2], [b, d, g], [c]):
        alone = la.run(only)
        for k in only:
            assert (bits(la.row(alone, k)) == bits(la.row(got, k))).all(), k


def test_nan_containment(gpu):
    rng = np.random.default_rng(4)
    taps_f, taps_d = 2500, 100                                                # P = 3
    bank = Bank([decaying(rng, taps_f), rng.standard_normal(taps_d)])
    frames = 6 * B + 50
    clean = rng.standard_normal(frames).astype(np.float32)
    la = Launch(bank)
    la.add(clean, 0)
    la.add(clean, 1)
    base = la.run()
    for m in (0, 1500, 2047, 2048, frames - 1):
        x = clean.copy()
        x[m] = np.nan
        lb = Launch(bank)
        lb.add(x, 0)                                                          # full lines
        lb.add(x, 1)
        lb.add(clean, 0)
        lb.add(clean, 1)
        lb.add(x, 0, 1700, 3000)                                              # and a range
        got = lb.run()
        y = lb.row(got, 0)
        nan = np.isnan(y)
        P = cm.partitions(taps_f)
        allowed = np.zeros(len(y), bool)
        allowed[(m // B) * B:(m // B + P + 2) * B] = True
        assert nan[m:m + taps_f].all() and not nan[~allowed].any()
        lo, hi, _ = cm.interval(clean, bank.h[0], 0, len(y))
        assert cm.outside(y[~nan], lo[~nan], hi[~nan]).size == 0
        yd = lb.row(got, 1)
        want = np.zeros(len(yd), bool)
        want[m:m + taps_d] = True
        assert (np.isnan(yd) == want).all()
        assert (bits(yd)[~want] == bits(la.row(base, 1))[~want]).all()
        assert (bits(lb.row(got, 2)) == bits(la.row(base, 0))).all() and (bits(lb.row(got, 3)) == bits(la.row(base, 1))).all()
        r = lb.row(got, 4)
        assert (np.isnan(r) == nan[1700:4700]).all() and (bits(r)[~nan[1700:4700]] == bits(y)[1700:4700][~nan[1700:4700]]).all()


def test_refusals_write_nothing(gpu):
    rng = np.random.default_rng(6)
    bank = Bank([rng.standard_normal(64), decaying(rng, 2000)])
    la = Launch(bank)
    la.add(rng.standard_normal(3000), 1, 0, 5000)                             # the line has 4999 samples
    with pytest.raises(afgpu.AfgError, match="make a line of 4999"):
        la.run()
    # an output inside the input plane, one allocation
    x = torch.from_numpy(rng.standard_normal(8000).astype(np.float32)).cuda()
    rec = np.zeros(1, afgpu.CONV_ROW_DTYPE)
    rec[0] = (0, 2000, 0, 0, 3000, 0, 0, 3063)
    tiles, work = afgpu.convolve_layout(rec, bank.rec, la.prm)
    keep = x.clone()
    with pytest.raises(afgpu.AfgError, match="output overlaps a row of record"):
        afgpu.convolve(1, torch.from_numpy(rec.view(np.uint8).copy()).cuda(), tiles, bank.d_rec, 2, la.prm, x, 8000, bank.d_bank, bank.bank_floats,
                       bank.d_spec, bank.spec_floats, torch.empty(2, device="cuda"), work, x, 8000)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32))


def test_convolve_tensor(gpu):
    rng = np.random.default_rng(8)
    hs = [rng.standard_normal(64).astype(np.float32), decaying(rng, 1500), rng.standard_normal(3).astype(np.float32)]
    bank = afgpu.ConvolveBank(hs)
    assert len(bank) == 3
    x = rng.standard_normal((3, 2, 2500)).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    valid = np.array([2500, 0, 1, 1024, 2499, 77])
    kern = np.array([0, 1, 2, 1, 1, 0])
    ref = Bank(hs)

    def want(mode, first=None):
        la = Launch(ref)
        for i in range(6):
            f, c = cm.mode_range(mode, int(valid[i]), len(hs[kern[i]]), 0 if first is None else int(first[i]))
            la.add(x.reshape(6, -1)[i, :valid[i]], int(kern[i]), f, c if valid[i] else 0)
        got = la.run()
        return [la.row(got, i) for i in range(6)]

    firsts = np.array([5, 0, 2, 1499, 700, 63])
    for mode, first in (("full", None), ("same", None), ("head", firsts), ("head", None)):
        y = afgpu.convolve_tensor(t, bank, torch.from_numpy(kern), mode, first, valid=valid)
        widest = 2500 + 1500 - 1 if mode == "full" else 2500
        assert tuple(y.shape) == (3, 2, widest) and y.dtype == torch.float32
        rows = y.cpu().numpy().reshape(6, -1)
        for i, w in enumerate(want(mode, first)):
            assert (bits(rows[i, :len(w)]) == bits(w)).all(), (mode, i)
            assert (bits(rows[i, len(w):]) == 0).all(), (mode, i)
    # one kernel for all, no valid, out given, the FFT path for everything
    out = torch.full((3, 2, 2500), float("nan"), device="cuda")
    y = afgpu.convolve_tensor(t, bank, 1, "same", out=out)
    assert y is out
    la = Launch(ref)
    for i in range(6):
        la.add(x.reshape(6, -1)[i], 1, mode="same")
    got = la.run()
    for i in range(6):
        assert (bits(y.cpu().numpy().reshape(6, -1)[i]) == bits(la.row(got, i))).all()
    y0 = afgpu.convolve_tensor(t, bank, 0, "same", direct_max=0)
    y1 = afgpu.convolve_tensor(t, bank, 0, "same")
    assert torch.allclose(y0, y1, rtol=0, atol=1e-3) and not torch.equal(y0, y1)
    # refusals, and an empty tensor
    for kw in (dict(kernel=3), dict(kernel=[0, 1]), dict(mode="valid"), dict(first=2), dict(mode="head", first=64), dict(valid=[1] * 5),
               dict(valid=[2501] * 6), dict(out=torch.empty(3, 2, 2499, device="cuda")), dict(direct_max=129), dict(bank=None)):
        args = dict(bank=bank, kernel=0, mode="full")
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.convolve_tensor(t, **args)
    with pytest.raises(ValueError):
        afgpu.convolve_tensor(t.cpu(), bank)
    with pytest.raises(ValueError):
        afgpu.convolve_tensor(t.double(), bank)
    assert tuple(afgpu.convolve_tensor(torch.empty(0, 2500, device="cuda"), bank, 1).shape) == (0, 2500 + 1499)
    assert tuple(afgpu.convolve_tensor(torch.empty(4, 0, device="cuda"), bank, 1, "same").shape) == (4, 0)
