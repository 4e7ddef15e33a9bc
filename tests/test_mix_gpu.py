"""afg_mix_hip (csrc/mix.hip) against tests/mix_model.py, as bit patterns: the statistics records and every float of the output
plane, for groups whose lengths sit on both sides of a lane, a short tile, a tile border and the chain over tiles, with one to
three rows, every alignment of the three planes, clips shorter and longer than a tile read from their start, middle and last
sample, shared and per-row noise, both modes -- all in one launch, and each group singly."""
import numpy as np
import pytest
import torch

import afgpu
import mix_model as mm
import normalize_model as nm

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc00123                                            # a NaN no operation makes
LENGTHS = (0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5)
CLIPS = (1, 2, 3, 5, 63, 64, 4095, 4096, 4097, 10000)
SNRS = (-5.0, 0.0, 20.0)
BAD = 47                                                         # the group the refusals damage: three rows of 4096 in SNR mode, N = 4096


def starts(N):
    return (0, 1 % N, N // 2, N - 1)


def shapes():
    """(rows, valid, stride, in_off % 4, out_off % 4, noise_off % 4, N, start, per-row noise, mode, snr or gain): every length
    with every clip once, the other axes cycling at periods that are coprime to the clips' ten"""
    out, k = [], 0
    for valid in LENGTHS:
        for N in CLIPS:
            rows = 1 + k % 3
            per_row = k % 2 == 1
            mode = mm.GAIN if k % 7 == 3 else mm.SNR
            level = 0.375 if mode == mm.GAIN else SNRS[k % 3]
            out.append((rows, valid, valid + 5, k % 4, (k // 4) % 4, (k // 3) % 4, N, starts(N)[(k // 2) % 4], per_row, mode, level))
            k += 1
    # whole tiles at 16-byte aligned addresses in every plane and row, the noise contiguous (and not) under them
    for N, start, noff in ((10000, 0, 0), (10000, 4, 0), (10000, 3, 1), (10000, 9000, 0), (4096, 0, 0), (4096, 4, 0), (8192, 0, 0), (8200, 8, 2)):
        out.append((2, 2 * 4096 + 5, 8200, 0, 0, noff, N, start, N % 8 == 0, mm.SNR, 0.0))
    out.append((2, 4096, 4100, 0, 2, 0, 10000, 16, False, mm.SNR, 20.0))      # ... in the input only
    return out


SHAPES = shapes()
SPECIAL = {"silent noise": len(SHAPES), "silent signal": len(SHAPES) + 1, "nan in signal": len(SHAPES) + 2, "inf in signal": len(SHAPES) + 3,
           "nan in noise": len(SHAPES) + 4, "inf in noise": len(SHAPES) + 5, "gain 0": len(SHAPES) + 6, "gain overflow": len(SHAPES) + 7,
           "nan with gain": len(SHAPES) + 8}
for _ in SPECIAL:                                                # two rows of 4100 against a clip of 5000 of their own
    SHAPES.append((2, 4100, 4104, 1, 2, 3, 5000, 77, True, mm.SNR, 0.0))
TWINS = (6 * len(CLIPS) + 9, len(SHAPES))                        # (2 * 4096 + 5 against N = 10000) and its copy at another place
SHAPES.append(SHAPES[TWINS[0]][:3] + (3, 1, 2) + SHAPES[TWINS[0]][6:])


def place(at, residue):
    return at + (residue - at) % 4


@pytest.fixture(scope="module")
def case(gpu):
    rng = np.random.default_rng(2025)
    n = len(SHAPES)
    groups = np.zeros(n, afgpu.MIX_GROUP_DTYPE)
    a = b = c = 3
    for k, (rows, valid, stride, ri, ro, rn, N, start, per_row, mode, level) in enumerate(SHAPES):
        g = groups[k]
        a, b, c = place(a, ri), place(b, ro), place(c, rn)
        g["in_off"], g["out_off"], g["stride"], g["rows"], g["valid"] = a, b, stride, rows, valid
        g["noise_off"], g["noise_len"], g["noise_start"], g["noise_stride"] = c, N, start, (N + 3 if per_row else 0)
        g["flags"] = mode
        if mode == mm.GAIN:
            g["gain"] = level
        else:
            g["ratio"] = afgpu.mix_ratio(level)
        a += rows * stride + 2
        b += rows * stride + 9
        c += (rows if per_row else 1) * (N + 3) + 1
    n_in, n_out, n_noise = a + 3, b + 3, c + 3
    tiles = afgpu.mix_layout(groups)
    x = (rng.standard_normal(n_in) * 10.0 ** rng.integers(-3, 3, n_in)).astype(np.float32)      # mixed magnitude: the order shows
    z = (0.3 * rng.standard_normal(n_noise) * 10.0 ** rng.integers(-2, 2, n_noise)).astype(np.float32)
    # NaN sentinels round the valid elements of every row and round every clip
    used_x, used_z = np.zeros(n_in, bool), np.zeros(n_noise, bool)
    for g in groups:
        for r in range(int(g["rows"])):
            used_x[int(g["in_off"]) + r * int(g["stride"]):][:int(g["valid"])] = True
            if g["noise_stride"] or r == 0:
                used_z[int(g["noise_off"]) + r * int(g["noise_stride"]):][:int(g["noise_len"])] = True
    x.view(np.uint32)[~used_x] = SENTINEL
    z.view(np.uint32)[~used_z] = SENTINEL

    def rows_of(plane, name, off, stride, length):
        g = groups[SPECIAL[name]]
        return [plane[int(g[off]) + r * int(g[stride]):][:int(g[length])] for r in range(2)]

    sig = lambda name: rows_of(x, name, "in_off", "stride", "valid")
    noi = lambda name: rows_of(z, name, "noise_off", "noise_stride", "noise_len")
    for r in noi("silent noise"):
        r[:] = 0.0
    for r in sig("silent signal"):
        r[:] = 0.0
    sig("nan in signal")[1][4098] = np.nan                       # in the second row's second tile
    sig("inf in signal")[0][77] = np.inf
    noi("nan in noise")[1][100] = np.nan
    noi("inf in noise")[0][4000] = -np.inf                       # (samples 77 .. 4176 of the clip lie under the rows)
    groups[SPECIAL["gain 0"]]["flags"], groups[SPECIAL["gain 0"]]["gain"] = mm.GAIN, 0.0
    sig("gain 0")[0][5] = np.nan
    x.view(np.uint32)[int(groups[SPECIAL["gain 0"]]["in_off"]) + 6] = 0xffc00bad          # a NaN whose bits come back
    for r in sig("gain overflow"):
        r[:] = 1e30
    for r in noi("gain overflow"):
        r[:] = 1e-30
    groups[SPECIAL["nan with gain"]]["flags"], groups[SPECIAL["nan with gain"]]["gain"] = mm.GAIN, 2.0
    x.view(np.uint32)[int(groups[SPECIAL["nan with gain"]]["in_off"]) + 9] = 0xffc00bad   # ... and one that becomes the one NaN
    # the twin's signal and noise are the original's
    g0, g1 = groups[TWINS[0]], groups[TWINS[1]]
    for r in range(int(g0["rows"])):
        x[int(g1["in_off"]) + r * int(g1["stride"]):][:int(g1["valid"])] = x[int(g0["in_off"]) + r * int(g0["stride"]):][:int(g0["valid"])]
        z[int(g1["noise_off"]) + r * int(g1["noise_stride"]):][:int(g1["noise_len"])] = z[int(g0["noise_off"]) + r * int(g0["noise_stride"]):][:int(g0["noise_len"])]
    x.setflags(write=False)
    z.setflags(write=False)
    for off in ("in_off", "out_off", "noise_off"):
        assert sorted({int(v) % 4 for v in groups[off]}) == [0, 1, 2, 3]
    assert {int(v) for v in groups["rows"]} == {1, 2, 3} and {int(v) for v in groups["flags"]} == {0, 1}
    sentinel_out = np.full(n_out, SENTINEL, np.uint32).view(np.float32)
    want_plane, want_stats = mm.mix(x, z, sentinel_out, groups.view(mm.GROUP_DTYPE))
    g = groups.copy()
    g["out_off"] = g["in_off"]
    place_plane, place_stats = mm.mix(x, z, x, g.view(mm.GROUP_DTYPE))
    assert place_stats.tobytes() == want_stats.tobytes()
    return {"groups": groups, "tiles": tiles, "x": x, "z": z, "n_out": n_out, "d_x": torch.from_numpy(x.copy()).cuda(),
            "d_z": torch.from_numpy(z.copy()).cuda(), "want": (want_plane, want_stats), "in_place": (place_plane, g)}


def sentinel_plane(n):
    return torch.from_numpy(np.full(n, SENTINEL, np.uint32).view(np.float32)).cuda()


def run(case, groups, d_in, d_out, tiles=None):
    tiles = case["tiles"] if tiles is None else tiles
    partials = torch.full((max(tiles, 1) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    stats = torch.full((len(groups) * 24,), 0xAB, dtype=torch.uint8, device="cuda")
    afgpu.mix(len(groups), torch.from_numpy(groups.view(np.uint8).copy()).cuda(), tiles, d_in, d_in.numel(), case["d_z"], case["d_z"].numel(), d_out,
              d_out.numel(), partials, stats)
    torch.cuda.synchronize()
    return stats.cpu().numpy().view(afgpu.MIX_STATS_DTYPE), partials


def inputs_intact(case):
    return (case["d_x"].cpu().numpy().view(np.uint32) == case["x"].view(np.uint32)).all() and \
        (case["d_z"].cpu().numpy().view(np.uint32) == case["z"].view(np.uint32)).all()


def test_records_and_output_are_the_models_bit_for_bit_in_one_launch(case):
    d_out = sentinel_plane(case["n_out"])
    stats, _ = run(case, case["groups"], case["d_x"], d_out)
    want_plane, want_stats = case["want"]
    assert mm.same_stats(stats, want_stats) == []
    bad = nm.same_bits(d_out.cpu().numpy(), want_plane)          # the sentinel's bits outside the valid elements included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
    untouched = want_plane.view(np.uint32) == SENTINEL
    assert untouched.sum() == case["n_out"] - int((case["groups"]["rows"].astype(np.int64) * case["groups"]["valid"]).sum())
    assert inputs_intact(case)
    # the model's gains are what they should be about: the SNR groups reach their level
    ok = [k for k, g in enumerate(case["groups"]) if g["flags"] == mm.SNR and g["valid"] >= 4095 and want_stats[k]["flags"] == 0]
    assert len(ok) > 30
    for k in ok:
        st = want_stats[k]
        snr = 10 * np.log10(st["signal_energy"] / (float(st["gain"]) ** 2 * st["noise_energy"]))
        assert abs(snr + 10 * np.log10(case["groups"][k]["ratio"])) < 1e-5, k


def test_in_place(case):
    want_plane, g = case["in_place"]
    d = case["d_x"].clone()
    stats, _ = run(case, g, d, d)
    assert mm.same_stats(stats, case["want"][1]) == []
    bad = nm.same_bits(d.cpu().numpy(), want_plane)              # the sentinels round the rows included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
    assert inputs_intact(case)


def test_every_group_singly(case):
    """each group in a launch of its own into one plane: the same bits as in the launch of all"""
    d_out = sentinel_plane(case["n_out"])
    want_plane, want_stats = case["want"]
    singles = list(range(0, len(SHAPES), 3)) + list(SPECIAL.values()) + list(TWINS)
    mask = np.zeros(case["n_out"], bool)
    for k in singles:
        g = case["groups"][k:k + 1].copy()
        tiles = afgpu.mix_layout(g)
        stats, _ = run(case, g, case["d_x"], d_out, tiles)
        assert mm.same_stats(stats, want_stats[k:k + 1]) == [], k
        for r in range(int(g["rows"][0])):
            mask[int(g["out_off"][0]) + r * int(g["stride"][0]):][:int(g["valid"][0])] = True
    got = d_out.cpu().numpy().view(np.uint32)
    assert (got[mask] == want_plane.view(np.uint32)[mask]).all() and (got[~mask] == SENTINEL).all()


def test_degenerate_groups_are_as_the_definition_says(case):
    groups, x = case["groups"], case["x"]
    plane, stats = case["want"]                                  # (the device's records and plane equal these: the first test)

    def back(name):
        g = groups[SPECIAL[name]]
        return all((plane[int(g["out_off"]) + r * int(g["stride"]):][:int(g["valid"])].view(np.uint32) ==
                    x[int(g["in_off"]) + r * int(g["stride"]):][:int(g["valid"])].view(np.uint32)).all() for r in range(int(g["rows"])))

    for name, why in (("silent noise", afgpu.MIX_SILENT_NOISE), ("silent signal", afgpu.MIX_SILENT_SIGNAL), ("nan in signal", afgpu.MIX_ENERGY_NOT_FINITE),
                      ("inf in signal", afgpu.MIX_ENERGY_NOT_FINITE), ("nan in noise", afgpu.MIX_ENERGY_NOT_FINITE),
                      ("inf in noise", afgpu.MIX_ENERGY_NOT_FINITE), ("gain overflow", afgpu.MIX_GAIN_NOT_FINITE), ("gain 0", 0)):
        st = stats[SPECIAL[name]]
        assert st["flags"] == why and st["gain"] == 0 and back(name), name
    assert np.isnan(stats[SPECIAL["nan in signal"]]["signal_energy"]) and stats[SPECIAL["inf in signal"]]["signal_energy"] == np.inf
    assert np.isnan(stats[SPECIAL["nan in noise"]]["noise_energy"]) and stats[SPECIAL["inf in noise"]]["noise_energy"] == np.inf
    assert stats[SPECIAL["silent noise"]]["noise_energy"] == 0 and stats[SPECIAL["silent signal"]]["signal_energy"] == 0
    g = groups[SPECIAL["nan with gain"]]
    assert plane.view(np.uint32)[int(g["out_off"]) + 9] == 0x7fc00000 and stats[SPECIAL["nan with gain"]]["gain"] == 2.0
    assert stats[0].tobytes() == bytes(24)                       # valid == 0: a record of zeros
    # twin groups at different places and alignments: the same record, the same output bits
    a, b = (groups[k] for k in TWINS)
    assert stats[TWINS[0]].tobytes() == stats[TWINS[1]].tobytes() and stats[TWINS[0]]["gain"] > 0
    for r in range(int(a["rows"])):
        ya = plane[int(a["out_off"]) + r * int(a["stride"]):][:int(a["valid"])]
        yb = plane[int(b["out_off"]) + r * int(b["stride"]):][:int(b["valid"])]
        assert (ya.view(np.uint32) == yb.view(np.uint32)).all()
    assert int(a["out_off"]) % 4 != int(b["out_off"]) % 4 or int(a["in_off"]) % 4 != int(b["in_off"]) % 4


def test_a_bad_record_is_refused_and_nothing_is_written(case):
    g5 = case["groups"][BAD]
    for change in (dict(in_off=case["x"].size - 10), dict(out_off=case["n_out"] - 10), dict(noise_off=case["z"].size - 10), dict(rows=0),
                   dict(first_tile=int(g5["first_tile"]) + 1), dict(noise_start=int(g5["noise_len"])), dict(flags=2), dict(ratio=float("nan")),
                   dict(noise_stride=1) if g5["noise_len"] > 1 else dict(noise_len=0)):
        g = case["groups"].copy()
        for k, v in change.items():
            g[BAD][k] = v
        d_out = sentinel_plane(case["n_out"])
        partials = torch.full((case["tiles"] * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        stats = torch.full((len(SHAPES) * 24,), 0xAB, dtype=torch.uint8, device="cuda")
        with pytest.raises(afgpu.AfgError) as e:
            afgpu.mix(len(SHAPES), torch.from_numpy(g.view(np.uint8).copy()).cuda(), case["tiles"], case["d_x"], case["x"].size, case["d_z"],
                      case["z"].size, d_out, case["n_out"], partials, stats)
        assert f"group {BAD}" in str(e.value), change
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (stats.cpu().numpy() == 0xAB).all() and (partials.cpu().numpy() == 0xAB).all()
        assert inputs_intact(case)
    # an output inside the noise plane, and an output over another group's input, are refused too
    partials = torch.full((case["tiles"] * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    stats = torch.full((len(SHAPES) * 24,), 0xAB, dtype=torch.uint8, device="cuda")
    big = torch.zeros(case["x"].size + case["z"].size + case["n_out"], dtype=torch.float32, device="cuda")
    with pytest.raises(afgpu.AfgError, match="noise plane"):
        afgpu.mix(len(SHAPES), torch.from_numpy(case["groups"].view(np.uint8).copy()).cuda(), case["tiles"], case["d_x"], case["x"].size,
                  big[:case["z"].size + 8], case["z"].size, big[case["z"].size - 8:], case["n_out"], partials, stats)
    g = case["groups"].copy()
    g["out_off"] = g["in_off"]
    g[BAD + 1]["out_off"] = g[BAD]["in_off"]
    d = case["d_x"].clone()
    with pytest.raises(afgpu.AfgError, match="overlaps"):
        afgpu.mix(len(SHAPES), torch.from_numpy(g.view(np.uint8).copy()).cuda(), case["tiles"], d, d.numel(), case["d_z"], case["z"].size, d, d.numel(),
                  partials, stats)
    torch.cuda.synchronize()
    assert (d.cpu().numpy().view(np.uint32) == case["x"].view(np.uint32)).all() and (stats.cpu().numpy() == 0xAB).all()


def test_add_noise_tensor_is_the_kernel_entry_and_torchaudios_expression(gpu):
    rng = np.random.default_rng(77)
    t = torch.from_numpy(rng.standard_normal((2, 3, 2, 5000)).astype(np.float32)).cuda()
    bank = torch.from_numpy((0.2 * rng.standard_normal((4, 3000))).astype(np.float32)).cuda()
    lengths, index, start, snr = [3000, 2999, 64, 5], [0, 1, 2, 3, 1, 0], [0, 2999 + 7, 1, 2, 3, 4], [-5, 0, 20, 0, -5, 20]
    valid = [5000, 4097, 0, 1, 4096, 4999]
    out, stats = afgpu.add_noise_tensor(t, bank, snr_db=snr, noise_lengths=lengths, noise_index=index, noise_start=start, valid=valid)
    torch.cuda.synchronize()
    x, z, y = t.cpu().numpy().reshape(6, 2, 5000), bank.cpu().numpy(), out.cpu().numpy().reshape(6, 2, 5000)
    for i in range(6):
        v, N = valid[i], lengths[index[i]]
        n = mm.noise_under(z[index[i], :N], start[i] % N, v)
        st = mm.group_stats(x[i, :, :v], np.stack([n, n]), mm.SNR, afgpu.mix_ratio(snr[i]))
        assert mm.same_stats(stats[i:i + 1], st.reshape(1)) == [], i
        scaled = torch.from_numpy(n) * float(st["gain"])         # torchaudio: scale * noise, then waveform + scaled_noise
        want = (torch.from_numpy(x[i, :, :v].copy()) + scaled).numpy()
        assert (y[i, :, :v].view(np.uint32) == want.view(np.uint32)).all(), i
        assert (y[i, :, v:].view(np.uint32) == x[i, :, v:].view(np.uint32)).all()
    # per-channel banks, the gain mode, in place
    bank3 = torch.from_numpy((0.2 * rng.standard_normal((2, 2, 700))).astype(np.float32)).cuda()
    keep = t.clone()
    same, stats = afgpu.add_noise_tensor(t, bank3, gain=0.5, noise_index=1, noise_start=699, out=t)
    torch.cuda.synchronize()
    assert same is t and (stats["gain"] == 0.5).all() and (stats["flags"] == 0).all()
    z3 = bank3.cpu().numpy()
    n = np.stack([mm.noise_under(z3[1, r], 699, 5000) for r in range(2)])
    want = mm.apply(keep.cpu().numpy().reshape(6, 2, 5000), n[None], 0.5)
    assert nm.same_bits(t.cpu().numpy().reshape(6, 2, 5000), want).size == 0
    for kw in (dict(), dict(snr_db=0, gain=1.0), dict(snr_db=float("nan")), dict(gain=-1.0), dict(snr_db=0, noise_index=4), dict(snr_db=0, noise_lengths=[1, 2, 3]),
               dict(snr_db=0, noise_lengths=0), dict(snr_db=[0, 1]), dict(snr_db=0, valid=[5001] * 6), dict(snr_db=0, out=bank), dict(snr_db=0, noise_start=-1)):
        with pytest.raises(ValueError):
            afgpu.add_noise_tensor(keep, bank, **kw)
    with pytest.raises(ValueError):
        afgpu.add_noise_tensor(keep, bank3[:, :1], snr_db=0)     # a bank of one channel against two (and not contiguous)
    with pytest.raises(ValueError, match="noise plane"):
        afgpu.add_noise_tensor(keep[0, 0, 0, :100].reshape(1, 100), keep.reshape(-1, 5000), snr_db=0, out=keep[0, 0, 1, :100].reshape(1, 100))
