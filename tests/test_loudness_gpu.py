"""afg_loudness_hip on the device against tests/loudness_model.py over the groups of tests/loudness_fixtures.py: every block
energy inside the interval B_j of include/afg.h round the model's, the model's gate counts (test_loudness_model.py shows that
no block of these groups is close to a threshold), the energy inside its bound, the gain within a float32 ulp, the peak bit
for bit; the product bit for bit x * recorded gain, in place and out of place; the clamps; the same group at two places bit for
bit; a NaN that stays in its group; and nothing written outside the valid elements."""
import numpy as np
import pytest

import afgpu
import loudness_fixtures as lf
import loudness_model as lm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(1234.5)


def launch(rate, gs, apply=False, in_place=False, first=(1, 3), **kw):
    """the groups gs ([rows, valid] arrays) through one launch: rows at odd offsets and strides in a plane of NaN, the output
    (when it is another plane) in a plane of sentinels at another alignment.  Returns (stats, [z per group], [output per
    group] or None), after checking that no float outside the valid elements was written and the input is as it was"""
    prm = afgpu.loudness_params(rate, weights=lf.WEIGHTS, apply=apply, **kw)
    rec = np.zeros(len(gs), afgpu.LOUDNESS_GROUP_DTYPE)
    at = first[0]
    for k, g in enumerate(gs):
        rows, valid = g.shape
        stride = valid + 1 + k % 3
        rec[k]["in_off"], rec[k]["stride"], rec[k]["rows"], rec[k]["valid"] = at, stride, rows, valid
        at += rows * stride + 2
    floats = at + 2
    shift = 0 if in_place else first[1] - first[0]
    rec["out_off"] = rec["in_off"] + np.uint64(shift)
    plane = np.full(floats, np.nan, np.float32)
    inside = np.zeros(floats, bool)
    for r, g in zip(rec, gs):
        for q in range(g.shape[0]):
            o = int(r["in_off"]) + q * int(r["stride"])
            plane[o:o + g.shape[1]] = g[q]
            inside[o:o + g.shape[1]] = True
    counts = afgpu.loudness_layout(rec, prm)
    d_in = torch.from_numpy(plane).cuda()
    d_out = None
    if apply:
        d_out = d_in if in_place else torch.full((floats + shift,), float(SENTINEL), dtype=torch.float32, device="cuda")
    afgpu.loudness_check_groups(rec, counts, prm, floats, floats + shift if apply else 0, in_place)
    d_sub = torch.full((max(counts.n_sub, 1),), float("nan"), dtype=torch.float64, device="cuda")
    d_blocks = torch.full((max(counts.n_blocks, 1),), float("nan"), dtype=torch.float64, device="cuda")
    d_stats = torch.full((len(gs) * afgpu.LOUDNESS_STATS_DTYPE.itemsize,), 0xee, dtype=torch.uint8, device="cuda")
    afgpu.loudness(len(gs), torch.from_numpy(rec.view(np.uint8)).cuda(), counts, prm, d_in, floats, d_out, floats + shift if apply else 0, d_sub,
                   d_blocks, d_stats)
    torch.cuda.synchronize()
    stats = d_stats.cpu().numpy().view(afgpu.LOUDNESS_STATS_DTYPE).copy()
    blocks = d_blocks.cpu().numpy()
    z = [blocks[int(r["first_block"]):int(r["first_block"]) + lm.blocks_of(g.shape[1], lm.step_of(rate))].copy() for r, g in zip(rec, gs)]
    assert sum(len(v) for v in z) == counts.n_blocks
    if not apply:
        assert (d_in.cpu().numpy().view(np.uint32) == plane.view(np.uint32)).all(), "the input plane was written"
        return stats, z, None
    got = d_out.cpu().numpy()
    if in_place:
        assert (got[~inside].view(np.uint32) == plane[~inside].view(np.uint32)).all(), "a float outside the valid elements was written"
    else:
        outside = np.ones(floats + shift, bool)
        outside[shift:][inside] = False
        assert (got[outside].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "a float outside the valid elements was written"
        assert (d_in.cpu().numpy().view(np.uint32) == plane.view(np.uint32)).all(), "the input plane was written"
    out = [np.stack([got[int(r["out_off"]) + q * int(r["stride"]):][:g.shape[1]] for q in range(g.shape[0])]) for r, g in zip(rec, gs)]
    return stats, z, out


def ulp32(a):
    return float(np.spacing(np.float32(abs(a))))


def same_records(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rate", lf.RATES)
def test_every_group_lies_inside_the_contract(rate):
    gs, twins = lf.groups(rate)
    ms = lf.model(rate)
    stats, zs, _ = launch(rate, gs)
    used = 0.0
    for k, (g, m, st, z) in enumerate(zip(gs, ms, stats, zs)):
        what = f"{rate} Hz, group {k} ({g.shape[0]} x {g.shape[1]})"
        assert st["n_blocks"] == m["n_blocks"] == len(z), what
        assert st["peak"].view(np.uint32) == m["peak"].view(np.uint32), f"{what}: peak {st['peak']!r}, want {m['peak']!r}"
        if len(z):
            B = lm.block_bounds(z, m["Sb"], m["peak"], rate, lf.WEIGHTS)
            err = np.abs(z.astype(lm.WIDE) - m["z"]).astype(np.float64)
            bad = np.flatnonzero(~(err <= B))
            assert bad.size == 0, f"{what}: block {bad[0]}: got {z[bad[0]]!r}, want {float(m['z'][bad[0]])!r}, allowed {B[bad[0]]!r}"
            used = max(used, float((err / B).max()))
            assert st["n_abs"] == m["n_abs"] and st["n_gated"] == int(m["gated"].sum()), what
            assert abs(st["rel_threshold"] - float(m["rel"])) <= 0.1 * B.mean() * (1.0 + 2.0 ** -50) + 2.0 ** -52 * float(m["rel"]), what
        n_gated = int(m["gated"].sum())
        if n_gated:
            allowed = B[m["gated"]].mean() * (1.0 + 2.0 ** -50)
            assert abs(st["energy"] - float(m["energy"])) <= allowed, f"{what}: energy {st['energy']!r}, want {float(m['energy'])!r}, allowed {allowed!r}"
            want, flags = lm.gain_of(float(m["energy"]), m["peak"])
            assert abs(float(st["gain"]) - float(want)) <= ulp32(want), f"{what}: gain {st['gain']!r}, want {want!r}"
            assert st["flags"] == flags == 0, what
            assert st["gain"].view(np.uint32) == lm.gain_of(st["energy"], st["peak"])[0].view(np.uint32), f"{what}: the gain of the recorded energy"
        else:
            assert st["energy"] == 0.0 and st["gain"] == np.float32(1.0) and st["flags"] == afgpu.LOUDNESS_UNGATED and st["n_gated"] == 0, what
    print(f"loudness {rate} Hz: {len(gs)} groups, {sum(len(z) for z in zs)} blocks: largest share of B_j used {used:.3g} (K_L = {afgpu.LOUDNESS_K})")
    # the same group at two positions and alignments of the launch
    for a, b in twins:
        assert same_records(stats[a], stats[b]) and zs[a].tobytes() == zs[b].tobytes(), f"{rate} Hz: groups {a} and {b} differ"
    # with the product: out of place and in place, bit for bit x * the recorded gain; the records are the measurement's
    apart_stats, apart_z, apart = launch(rate, gs, apply=True)
    same_stats, _, same = launch(rate, gs, apply=True, in_place=True, first=(2, 2))
    assert same_records(apart_stats, stats) and same_records(same_stats, stats)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(apart_z, zs))
    moved = 0
    for k, (g, st) in enumerate(zip(gs, stats)):
        want = g * st["gain"]
        assert want.dtype == np.float32
        assert (apart[k].view(np.uint32) == want.view(np.uint32)).all(), f"{rate} Hz, group {k}: the product out of place"
        assert (same[k].view(np.uint32) == want.view(np.uint32)).all(), f"{rate} Hz, group {k}: the product in place"
        moved += bool(g.size and (want != g).any())
    assert moved >= 4


def test_the_clamps_and_the_target():
    rate = 11025
    gs, _ = lf.groups(rate)
    k = 2 * lf.lengths(rate).index(lf.long_length(rate)) + 1    # two rows with a loud part, a passage and a tail
    part = [gs[k], gs[0], gs[k][:1]]
    plain, _, _ = launch(rate, part, target_lufs=-16.0)
    free = lm.gain_of(plain[0]["energy"], plain[0]["peak"], -16.0)[0]
    assert plain[0]["gain"].view(np.uint32) == free.view(np.uint32) and plain[0]["flags"] == 0
    low = float(free) / 8 * float(plain[0]["peak"])              # a ceiling the free gain would exceed eight times
    seen = []
    for kw in (dict(max_gain=float(free) / 2), dict(max_peak=low), dict(max_gain=float(free) / 2, max_peak=low), dict(max_gain=100.0, max_peak=64.0)):
        stats, _, out = launch(rate, part, apply=True, target_lufs=-16.0, **kw)
        for st, ref, g in zip(stats, plain, part):
            assert st["energy"] == ref["energy"] and st["peak"].view(np.uint32) == ref["peak"].view(np.uint32)
            want, flags = lm.gain_of(st["energy"], st["peak"], -16.0, kw.get("max_peak", 0.0), kw.get("max_gain", 0.0))
            assert st["gain"].view(np.uint32) == want.view(np.uint32) and st["flags"] == flags, (kw, st, want, flags)
        seen.append(int(stats[0]["flags"]))
        if kw.get("max_peak") == low:
            assert 0 < np.abs(out[0]).max() <= np.float32(low) * (1 + 2.0 ** -22)
        assert (out[0].view(np.uint32) == (part[0] * stats[0]["gain"]).view(np.uint32)).all()
        assert stats[1]["flags"] == afgpu.LOUDNESS_UNGATED and stats[1]["gain"] == 1.0      # no samples: the clamps do not touch it
    assert seen == [afgpu.LOUDNESS_GAIN_CLAMPED, afgpu.LOUDNESS_PEAK_CLAMPED, afgpu.LOUDNESS_GAIN_CLAMPED | afgpu.LOUDNESS_PEAK_CLAMPED, 0]


@pytest.mark.parametrize("where", [(0, 0), (1, 4097), (0, -1)])
def test_a_nan_stays_in_its_group(where):
    rate = 8000
    gs, _ = lf.groups(rate)
    k = 2 * lf.lengths(rate).index(lf.long_length(rate))
    part = [gs[k], gs[k + 1], gs[k]]
    want_stats, want_z, want_out = launch(rate, part, apply=True, in_place=True)
    bad = gs[k + 1].copy()
    bad[where] = np.nan
    stats, z, out = launch(rate, [gs[k], bad, gs[k]], apply=True, in_place=True)        # (launch checks what lies outside)
    for q in (0, 2):
        assert same_records(stats[q], want_stats[q]) and z[q].tobytes() == want_z[q].tobytes()
        assert (out[q].view(np.uint32) == want_out[q].view(np.uint32)).all()
    assert same_records(stats[0], stats[2])


def test_loudness_tensor_brings_every_file_to_the_target():
    rate = 16000
    rng = np.random.default_rng(9)
    x = (rng.uniform(-1.0, 1.0, (3, 2, 12000)) * np.array([0.5, 0.05, 0.2])[:, None, None]).astype(np.float32)
    valid = np.array([12000, 9000, 6399])
    t = torch.from_numpy(x).cuda()
    out, stats = afgpu.loudness_tensor(t, valid, samplerate=rate, target_lufs=-20.0)
    got = out.cpu().numpy()
    for i, n in enumerate(valid):
        m = lm.measure(x[i], int(n), rate)
        if m["n_blocks"]:
            assert abs(afgpu.loudness_lufs(stats[i]["energy"]) - lm.lufs(float(m["energy"]))) < 1e-9
            after = lm.measure(got[i], int(n), rate)
            assert abs(lm.lufs(float(after["energy"])) + 20.0) < 1e-4
        else:
            assert stats[i]["flags"] == afgpu.LOUDNESS_UNGATED and stats[i]["gain"] == 1.0
        assert (got[i, :, :n].view(np.uint32) == (x[i, :, :n] * stats[i]["gain"]).view(np.uint32)).all()
        assert (got[i, :, n:].view(np.uint32) == x[i, :, n:].view(np.uint32)).all()
    none, measured = afgpu.loudness_tensor(t, valid, samplerate=rate, apply=False)
    assert none is None and (measured["energy"] == stats["energy"]).all()
    u = t.clone()
    same, _ = afgpu.loudness_tensor(u, valid, samplerate=rate, target_lufs=-20.0, out=u)
    assert same is u and (u.cpu().numpy().view(np.uint32) == got.view(np.uint32)).all()
    with pytest.raises(ValueError):
        afgpu.loudness_tensor(t, valid, samplerate=4000)
