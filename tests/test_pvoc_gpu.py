"""afg_pvoc_hip against the interval tests/pvoc_model.py computes from the long-double definition: every delivered component
inside E_t, none left out.  The harness is tests/test_istft_gpu.py's: every slab lies between NaN guard floats, what a row's
in_pitch holds beyond its n_frames is NaN too, and every output slab lies between sentinel words with sentinels in its pitch
padding -- a read outside the record turns results into NaN, a store outside it kills a sentinel.  Every launch runs behind
afgpu.lds_fill().  The kernel's paths depend on the rate (<= 1: one run of frames per tile; > 1: a pair per step) and on
F_out against the lane chunk C = 4 and the tile T = 256 = 64 C, not on n_fft; so the two small shapes take every rate with
every F_out, and 400 / 160 -- 201 bins, not a multiple of a workgroup's four -- takes every rate with fewer lengths."""
import numpy as np
import pytest
import torch

import afgpu
import pvoc_model as pm

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead
GUARD = 3
C_, T_ = afgpu.PVOC_CHUNK, afgpu.PVOC_TILE
RATES = [1.0, 0.5, 2.0, 1.25, 0.8, 1.0 / 3.0, 1.1, 0.9, 64.0, 1.0 / 64.0]
TARGETS = sorted({1, 2, 63, 64, 65, 64 * C_ - 1, 64 * C_, 64 * C_ + 1, T_ - 1, T_, T_ + 1, 2 * T_ + 1})
SHAPES = [(16, 4, None), (30, 7, None), (400, 160, (0, 1, 100, 199, 200))]


def frames_for(rate, target):
    """the n_frames whose out_frames is `target`, or the nearest above it that a rate below 1 can make"""
    n = max(1, int(np.floor((target - 1) * rate)) + 1)
    while pm.out_frames(n, rate) < target:
        n += 1
    return n


def noise_spec(rng, n_bins, f, spread=False):
    mag = 10.0 ** rng.uniform(-30, 30, (n_bins, f)) if spread else rng.uniform(0.5, 2.0, (n_bins, f))
    ang = rng.uniform(-np.pi, np.pi, (n_bins, f))
    return np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1).astype(np.float32)


class Launch:
    """records of one parameter set over one input plane and one output plane"""

    def __init__(self, n_fft, hop, bins=None):
        self.n_fft, self.hop, self.n_bins = n_fft, hop, n_fft // 2 + 1
        self.bins = np.arange(self.n_bins) if bins is None else np.asarray(bins)
        self.prm = afgpu.pvoc_params(n_fft, hop)
        self.recs, self.slabs, self.in_at, self.out_at = [], [], 0, 0

    def add(self, spec, rate, in_pad=0, out_pad=0, count=None):
        """spec: float32 [n_bins, n_frames, 2]"""
        spec = np.ascontiguousarray(spec, np.float32)
        f = spec.shape[1]
        count = pm.out_frames(f, rate) if count is None else count
        self.in_at += GUARD
        self.out_at += GUARD
        self.recs.append((self.in_at, self.out_at, float(rate), f, f + in_pad, count, count + out_pad))
        self.slabs.append(spec)
        self.in_at += 2 * self.n_bins * (f + in_pad)
        self.out_at += 2 * self.n_bins * (count + out_pad)
        return len(self.recs) - 1

    def planes(self):
        d_in = np.full(self.in_at + GUARD, np.nan, np.float32)
        rec = np.zeros(len(self.recs), afgpu.PVOC_ROW_DTYPE)
        for k, ((i, o, rate, f, ip, count, op), s) in enumerate(zip(self.recs, self.slabs)):
            d_in[i:i + 2 * self.n_bins * ip].reshape(self.n_bins, ip, 2)[:, :f] = s
            rec[k] = (i, o, rate, f, ip, count, op, (0, 0))
        return rec, d_in, np.full(self.out_at + GUARD, SENTINEL, np.uint32)

    def device(self, rec, d_in, before, **kw):
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_src = torch.from_numpy(d_in.view(np.int32).copy()).cuda()
        d_out = torch.from_numpy(before.view(np.int32).copy()).cuda()
        afgpu.lds_fill()
        try:
            afgpu.pvoc(len(rec), d_rec, kw.get("prm", self.prm), d_src, kw.get("in_floats", len(d_in)), d_out, kw.get("out_floats", len(before)))
        finally:
            torch.cuda.synchronize()
            got = self.last = d_out.cpu().numpy().view(np.uint32)
        return got

    def slab(self, got, k):
        """the delivered [n_bins, out_frames, 2] of record k"""
        i, o, rate, f, ip, count, op = self.recs[k]
        return got[o:o + 2 * self.n_bins * op].view(np.float32).reshape(self.n_bins, op, 2)[:, :count]

    def written(self, before):
        w = np.zeros(len(before), bool)
        for (i, o, rate, f, ip, count, op) in self.recs:
            w[o:o + 2 * self.n_bins * op].reshape(self.n_bins, op, 2)[:, :count] = True
        return w

    def model(self, k):
        s = self.slabs[k]
        return pm.model(s[:, :, 0], s[:, :, 1], self.n_fft, self.hop, self.recs[k][2], self.bins)

    def share(self, got, k):
        y = self.slab(got, k)[self.bins]
        return pm.share(y[:, :, 0], y[:, :, 1], *self.model(k))

    def run(self, skip=()):
        """every component of every slab inside its interval, everything else untouched; returns (got, largest share of E_t)"""
        rec, d_in, before = self.planes()
        got = self.device(rec, d_in, before)
        used = 0.0
        for k, r in enumerate(self.recs):
            if r[5] == 0 or k in skip:
                continue
            sh = self.share(got, k)
            assert sh <= 1.0, (k, r, sh)
            used = max(used, sh)
            assert not np.isnan(self.slab(got, k)).any(), k               # (the bins the model leaves out read nothing foreign either)
        assert (got[~self.written(before)] == SENTINEL).all()
        return got, used


@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r:.4g}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_slabs_of_every_geometry(gpu, shape, rate):
    n_fft, hop, bins = shape
    rng = np.random.default_rng(n_fft + int(rate * 1000))
    la = Launch(n_fft, hop, bins)
    targets = TARGETS if bins is None else ([2, 65] if rate > 2 else [2, 65, T_ + 1, 2 * T_ + 1])
    made = set()
    for j, target in enumerate(targets):
        f = frames_for(rate, target)
        made.add(pm.out_frames(f, rate))
        la.add(noise_spec(rng, la.n_bins, f), rate, in_pad=(0, 5)[j & 1], out_pad=(3, 0)[j & 1] if j % 3 else 0)
    if rate >= 1:
        assert made == set(targets)
    f = frames_for(rate, 70)
    la.add(noise_spec(rng, la.n_bins, f, spread=True), rate, out_pad=1)            # magnitudes over 1e-30 .. 1e30
    la.add(noise_spec(rng, la.n_bins, 3), rate, count=0)                           # nothing to deliver
    got, used = la.run()
    print(f"pvoc {n_fft}/{hop} rate {rate:.4g}: F_out {sorted(made)}, largest share of E_t used {used:.4f}")
    assert (la.slab(got, 0) != 0).any()


def test_rate_one_gives_back_its_input(gpu):
    rng = np.random.default_rng(41)
    la = Launch(30, 7)
    spec = noise_spec(rng, la.n_bins, 2 * T_ + 9)
    la.add(spec, 1.0)
    got, used = la.run()
    y = la.slab(got, 0).astype(np.float64)
    m = np.hypot(spec[..., 0].astype(np.float64), spec[..., 1].astype(np.float64))[..., None]
    E = m * pm.bracket(np.arange(spec.shape[1]))[None, :, None]
    assert (np.abs(y - spec) <= E).all()
    print(f"pvoc rate 1: largest share of E_t used {used:.4f}, against the input itself {float((np.abs(y - spec) / E).max()):.4f}")


def test_the_same_slab_gives_the_same_bits_wherever_it_stands(gpu):
    rng = np.random.default_rng(42)
    la = Launch(30, 7)
    spec = noise_spec(rng, la.n_bins, 431)
    la.add(noise_spec(rng, la.n_bins, 90), 0.5, out_pad=2)
    a = la.add(spec, 0.8)
    la.add(noise_spec(rng, la.n_bins, 700), 2.0, in_pad=3)
    la.add(noise_spec(rng, la.n_bins, 17), 1.0 / 3.0)
    b = la.add(spec, 0.8, in_pad=4, out_pad=7)                                     # the twin, elsewhere and at other pitches
    la.add(noise_spec(rng, la.n_bins, 5), 1.1)
    got, _ = la.run()
    alone = Launch(30, 7)
    alone.add(spec, 0.8)
    got1, _ = alone.run()
    ya, yb, y1 = (s.view(np.uint32) for s in (la.slab(got, a), la.slab(got, b), alone.slab(got1, 0)))
    assert ya.shape[1] == pm.out_frames(431, 0.8) > 2 * T_
    assert (ya == yb).all() and (ya == y1).all()


def test_a_second_long_row_stays_inside_the_bound_at_its_last_step(gpu):
    rng = np.random.default_rng(43)
    la = Launch(16, 4)
    spec = noise_spec(rng, la.n_bins, 16001)
    k = la.add(spec, 0.8)                                                          # F_out 20002: 79 tiles
    got, used = la.run()
    y = la.slab(got, k)
    yr, yi, m = la.model(k)
    t = y.shape[1] - 1
    last = max(float((np.abs(y[:, t, 0] - yr[:, t]) / (m[:, t] * pm.bracket(t))).max()), float((np.abs(y[:, t, 1] - yi[:, t]) / (m[:, t] * pm.bracket(t))).max()))
    print(f"pvoc long row: F_out {t + 1}, largest share of E_t used {used:.4f}, at the last step at most {last:.4f}; the float32 rounding alone is"
          f" {2.0 ** -24 / pm.bracket(t):.4f} of the bracket there")
    assert t + 1 >= 20000 and used <= 1.0 and last <= 1.0


def test_zeros_and_signed_zeros(gpu):
    rng = np.random.default_rng(44)
    la = Launch(16, 4)
    z = la.add(np.zeros((la.n_bins, 300, 2), np.float32), 0.8)
    spec = noise_spec(rng, la.n_bins, 300)
    spec[2, 10] = (-0.0, 0.0)                                                      # atan2(+0, -0) = pi
    spec[3, 11] = (0.0, -0.0)                                                      # atan2(-0, +0) = -0
    spec[4, 12] = (-0.0, -0.0)                                                     # atan2(-0, -0) = -pi
    spec[5, 0] = (-0.0, 0.0)                                                       # th_0 itself
    s = la.add(spec, 0.8)
    s2 = la.add(spec, 1.25)
    got, used = la.run()
    assert (la.slab(got, z) == 0).all()                                            # a zero of either sign
    print(f"pvoc signed zeros: largest share of E_t used {used:.4f}")
    assert s != s2


def test_a_nan_reaches_only_the_steps_behind_it_in_its_bin(gpu):
    rng = np.random.default_rng(45)
    for rate in (0.8, 1.25):
        la = Launch(30, 7)
        f, kb, fb = 700, 6, 333
        clean = noise_spec(rng, la.n_bins, f)
        hit = clean.copy()
        hit[kb, fb, 1] = np.nan
        inf = clean.copy()
        inf[kb + 1, fb + 40, 0] = np.inf
        a, b, c = la.add(clean, rate), la.add(hit, rate), la.add(inf, rate)
        d = la.add(noise_spec(rng, la.n_bins, 80), 0.5)
        rec, d_in, before = la.planes()
        got = la.device(rec, d_in, before)
        i = pm.steps(f, rate)[1]
        ya = la.slab(got, a).view(np.uint32)
        for k, (bin_, frame) in ((b, (kb, fb)), (c, (kb + 1, fb + 40))):
            y = la.slab(got, k).view(np.uint32)
            before_it = i + 1 < frame
            assert before_it.any() and not before_it.all()
            other = np.arange(la.n_bins) != bin_
            assert (y[other] == ya[other]).all()                                   # every other bin: the clean slab's bits
            assert (y[bin_][before_it] == ya[bin_][before_it]).all()               # and its own bin in front of the frame
        assert np.isnan(la.slab(got, b)[kb][i >= fb]).all()
        for k in (a, d):
            assert la.share(got, k) <= 1.0
        assert (got[~la.written(before)] == SENTINEL).all()


def test_a_record_that_breaks_a_rule_is_refused_and_nothing_is_written(gpu):
    rng = np.random.default_rng(46)
    la = Launch(16, 4)
    la.add(noise_spec(rng, la.n_bins, 50), 0.8)
    la.add(noise_spec(rng, la.n_bins, 20), 2.0, in_pad=2, out_pad=2)
    rec, d_in, before = la.planes()
    assert (la.device(rec, d_in, before) != before).any()                          # as it stands it runs
    seen = set()

    def refused(change=None, **kw):
        bad = rec.copy()
        if change:
            change(bad)
        with pytest.raises(afgpu.AfgError) as e:
            la.device(bad, d_in, before, **kw)
        assert "invalid argument" in str(e.value)
        seen.add(str(e.value))
        assert (la.last == before).all()                                           # nothing was written

    refused(lambda b: b["rate"].__setitem__(0, float("nan")))
    refused(lambda b: b["rate"].__setitem__(1, 65.0))
    refused(lambda b: b["out_frames"].__setitem__(0, int(rec[0]["out_frames"]) + 1))
    refused(lambda b: b["out_frames"].__setitem__(0, int(rec[0]["out_frames"]) - 1))
    refused(lambda b: b["in_pitch"].__setitem__(1, 19))
    refused(lambda b: b["out_pitch"].__setitem__(1, 9))
    refused(lambda b: b["n_frames"].__setitem__(0, 0))
    refused(out_floats=len(before) - GUARD - 2 * 2 - 1)                            # the last slab's last pair
    refused(in_floats=len(d_in) - GUARD - 2 * 2 - 1)
    refused(lambda b: b["in_off"].__setitem__(0, (1 << 64) - 8))
    refused(lambda b: b["out_off"].__setitem__(1, 1 << 63))
    refused(lambda b: b["reserved"].__setitem__((0, 1), 1))
    refused(prm=afgpu.PvocParams(16, 17))
    refused(prm=afgpu.PvocParams(16, 4, (1, 0, 0, 0, 0, 0)))
    assert len(seen) == 14


def test_phase_vocoder_tensor_with_a_rate_per_slab_and_valid_frames(gpu):
    n_fft, hop, F = 30, 7, 300
    rng = np.random.default_rng(47)
    n_bins = n_fft // 2 + 1
    spec = np.stack([noise_spec(rng, n_bins, F) for _ in range(6)]).reshape(2, 3, n_bins, F, 2)
    rates = np.array([0.8, 1.25, 1.0, 0.5, 2.0, 1.1])
    valid = np.array([F, 1, 0, 17, F - 1, 257])
    d = torch.from_numpy(spec).cuda()
    afgpu.lds_fill()
    out, counts = afgpu.phase_vocoder_tensor(torch.view_as_complex(d), rates, n_fft, hop, valid_frames=valid)
    want = [pm.out_frames(v, r) if v else 0 for v, r in zip(valid, rates)]
    assert list(counts) == want and out.dtype == torch.complex64 and tuple(out.shape) == (2, 3, n_bins, max(want))
    got = torch.view_as_real(out).cpu().numpy().reshape(6, n_bins, -1, 2)
    used = 0.0
    for r in range(6):
        assert (got[r, :, want[r]:] == 0).all()                                    # zero behind each slab's own frames
        if want[r]:
            s = spec.reshape(6, n_bins, F, 2)[r, :, :valid[r]]
            sh = pm.share(got[r, :, :want[r], 0], got[r, :, :want[r], 1], *pm.model(s[..., 0], s[..., 1], n_fft, hop, rates[r]))
            assert sh <= 1.0, (r, sh)
            used = max(used, sh)
    print(f"phase_vocoder_tensor: counts {want}, largest share of E_t used {used:.4f}")
    # one rate for all, the float32 view, and an out tensor that is longer than needed and dirty
    n1 = pm.out_frames(F, 0.9)
    dirty = torch.full((2, 3, n_bins, n1 + 5, 2), 7.0, device="cuda")
    res, c1 = afgpu.phase_vocoder_tensor(d, 0.9, n_fft, hop, out=dirty)
    assert res.data_ptr() == dirty.data_ptr() and (c1 == n1).all() and (dirty[..., n1:, :] == 0).all() and (dirty[..., :n1, :] != 7.0).any()
    both, _ = afgpu.phase_vocoder_tensor(d, np.full(6, 0.9), n_fft, hop)
    assert torch.equal(both, dirty[..., :n1, :])
    with pytest.raises(afgpu.AfgError):
        afgpu.phase_vocoder_tensor(d, 100.0, n_fft, hop)
    with pytest.raises(ValueError):
        afgpu.phase_vocoder_tensor(d[:, :, :-1], 1.0, n_fft, hop)


def test_stft_tensor_is_stft_over_hand_built_records(gpu):
    n_fft, hop, n = 400, 160, 160 * 30
    rng = np.random.default_rng(48)
    x = torch.from_numpy((rng.standard_normal((2, 3, n)) * 0.5).astype(np.float32)).cuda()
    got = afgpu.stft_tensor(x, n_fft, hop)
    n_bins, F = n_fft // 2 + 1, 1 + n // hop
    assert got.dtype == torch.complex64 and tuple(got.shape) == (2, 3, n_bins, F)
    prm = afgpu.stft_params(n_fft, hop, None, True, afgpu.MEL_PAD_REFLECT, afgpu.STFT_COMPLEX)
    rows = np.zeros(6, afgpu.MEL_ROW_DTYPE)
    rows["in_off"], rows["out_off"] = np.arange(6) * n, np.arange(6) * (2 * n_bins * F)
    rows["in_frames"], rows["out_frames"] = n, F
    tiles = afgpu.stft_layout(rows, prm)
    table = torch.from_numpy(afgpu.mel_fft_tables(n_fft, n_fft)).cuda()
    want = torch.zeros((2, 3, n_bins, F, 2), dtype=torch.float32, device="cuda")
    afgpu.stft(6, torch.from_numpy(rows.view(np.uint8).copy()).cuda(), tiles, prm, x, x.numel(), table, table.numel(), want, want.numel())
    assert torch.equal(torch.view_as_real(got).view(torch.int32), want.view(torch.int32))
    power = afgpu.stft_tensor(x, n_fft, hop, out_kind=afgpu.STFT_POWER)
    assert power.dtype == torch.float32 and tuple(power.shape) == (2, 3, n_bins, F)
    # valid: every row framed as its own samples, packed at the front of its slab
    valid = np.array([n, 1600, 0, 801, n - 1, 201])
    packed, frames = afgpu.stft_tensor(x, n_fft, hop, valid=valid)
    assert list(frames) == [1 + v // hop if v else 0 for v in valid]
    flat = torch.view_as_real(packed).reshape(6, -1)
    for r, (v, f) in enumerate(zip(valid, frames)):
        assert (flat[r, 2 * n_bins * f:] == 0).all()
        if v:
            alone = afgpu.stft_tensor(x.reshape(6, n)[r, :v].contiguous(), n_fft, hop)
            assert torch.equal(flat[r, :2 * n_bins * f].view(torch.int32), torch.view_as_real(alone).reshape(-1).view(torch.int32))


def test_time_stretch_tensor_is_the_three_calls_and_keeps_the_pitch(gpu):
    sr, n_fft, hop, n = 16000, 400, 160, 16000
    t = np.arange(n) / sr
    x = torch.from_numpy(np.stack([0.5 * np.sin(2 * np.pi * 440.0 * t), 0.5 * np.sin(2 * np.pi * 440.0 * t + 1.0)]).astype(np.float32)).cuda()
    rates = np.array([0.8, 1.25])
    y, lengths = afgpu.time_stretch_tensor(x, rates, n_fft, hop)
    # the three calls made separately
    spec = afgpu.stft_tensor(x, n_fft, hop)
    st, counts = afgpu.phase_vocoder_tensor(spec, rates, n_fft, hop)
    want_len = np.minimum(np.floor(n / rates + 0.5).astype(np.int64), hop * (counts - 1))
    assert list(lengths) == list(want_len) and list(counts) == [pm.out_frames(1 + n // hop, r) for r in rates]
    assert tuple(y.shape) == (2, int(want_len.max())) and y.dtype == torch.float32
    z = afgpu.istft_tensor(st, n_fft, hop, valid_frames=counts)
    for r in range(2):
        assert torch.equal(y[r, :want_len[r]].view(torch.int32), z[r, :want_len[r]].view(torch.int32))
        assert (y[r, want_len[r]:] == 0).all()
        # the pitch stays: the largest bin of a float64 FFT over the middle half
        L = int(want_len[r])
        mid = y[r, L // 4:L // 4 + L // 2].cpu().numpy().astype(np.float64)
        peak = int(np.abs(np.fft.rfft(mid * np.hanning(len(mid)))).argmax())
        assert abs(peak * sr / len(mid) - 440.0) <= sr / len(mid), (r, peak * sr / len(mid))
    # one rate, rows of their own lengths
    valid = np.array([16000, 9000])
    y2, l2 = afgpu.time_stretch_tensor(x, 1.25, n_fft, hop, valid=valid)
    assert list(l2) == [min(int(np.floor(v / 1.25 + 0.5)), hop * (pm.out_frames(1 + v // hop, 1.25) - 1)) for v in valid]
    alone, _ = afgpu.time_stretch_tensor(x[1:2, :9000].contiguous(), 1.25, n_fft, hop)
    assert torch.equal(y2[1, :l2[1]].view(torch.int32), alone[0].view(torch.int32)) and (y2[1, l2[1]:] == 0).all()
