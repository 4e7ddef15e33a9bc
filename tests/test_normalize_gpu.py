"""afg_normalize_hip (csrc/normalize.hip) against tests/normalize_model.py, as bit patterns: the statistics records and
every float of the output plane, for groups whose lengths sit on both sides of a lane, a short tile, a tile border and the
chain over tiles, with one to three rows, every alignment of either plane, all in one launch, in every mode."""
import numpy as np
import pytest
import torch

import afgpu
import normalize_model as nm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc00123                                            # a NaN no operation makes
# (rows, valid, in_off % 4, out_off % 4); the stride is valid + 5 unless given (a multiple of 4 keeps every row aligned)
SHAPES = [(1, 0, 0, 0), (2, 1, 1, 2), (3, 3, 2, 2), (1, 255, 3, 0), (2, 1024, 0, 1), (3, 4095, 1, 1), (1, 4096, 2, 3), (2, 4097, 3, 3),
          (3, 2 * 4096 + 5, 0, 0, 8200),                         # whole tiles at 16-byte aligned addresses in both planes, in every row
          (2, 4096, 0, 2, 4100),                                 # ... in the input only
          (1, 300, 1, 0), (2, 4100, 2, 1), (1, 500, 3, 2)]       # all zero; one NaN; one +inf
ZERO, WITH_NAN, WITH_INF = 10, 11, 12
PARAMS = {"none": {}, "peak": dict(target=0.5), "rms": dict(target=0.1), "standard": dict(eps=1e-5), "standard0": {},
          "dynamic_range": dict(range=2.5, shift=1.0, gain=0.5), "whisper": {}}


def place(at, residue):
    return at + (residue - at) % 4


@pytest.fixture(scope="module")
def case(gpu):
    rng = np.random.default_rng(2024)
    groups = np.zeros(len(SHAPES), afgpu.NORM_GROUP_DTYPE)
    a = b = 3
    for k, s in enumerate(SHAPES):
        rows, valid, ri, ro = s[:4]
        stride = s[4] if len(s) > 4 else valid + 5
        a, b = place(a, ri), place(b, ro)
        groups[k]["in_off"], groups[k]["out_off"], groups[k]["stride"], groups[k]["rows"], groups[k]["valid"] = a, b, stride, rows, valid
        a += rows * stride + 2
        b += rows * stride + 9
    n_in, n_out = a + 3, b + 3
    tiles = afgpu.norm_layout(groups)
    x = (rng.standard_normal(n_in) * 10.0 ** rng.integers(-3, 3, n_in)).astype(np.float32)     # mixed magnitude: the order shows
    g = groups[ZERO]
    x[int(g["in_off"]):int(g["in_off"]) + int(g["valid"])] = 0.0
    x[int(groups[WITH_NAN]["in_off"]) + 4100 + 5 + 4098] = np.nan                               # in the second row's second tile
    x[int(groups[WITH_INF]["in_off"]) + 77] = np.inf
    x.setflags(write=False)
    # the test can tell orders apart: another order of the tiles, and a plain running sum, give other bits
    big = groups[8]
    rows = np.stack([x[int(big["in_off"]) + r * 8200:][:int(big["valid"])] for r in range(3)])
    mine = nm.group_sums(rows)
    assert nm.group_sums(rows, tile_order=list(range(9))[::-1]) != mine
    assert float(np.add.accumulate(rows.ravel().astype(np.float64))[-1]) != float(mine[0])
    assert sorted({int(v) % 4 for v in groups["in_off"]}) == [0, 1, 2, 3] == sorted({int(v) % 4 for v in groups["out_off"]})
    return {"groups": groups, "tiles": tiles, "x": x, "n_out": n_out, "d_groups": torch.from_numpy(groups.view(np.uint8).copy()).cuda(),
            "d_x": torch.from_numpy(x.copy()).cuda(), "model": {}}


def model(case, name, in_place=False):
    """the model's (plane, records) for a parameter set, made once"""
    key = (name, in_place)
    if key not in case["model"]:
        g = case["groups"].copy()
        if in_place:
            g["out_off"] = g["in_off"]
            out = case["x"].copy()
        else:
            out = np.full(case["n_out"], SENTINEL, np.uint32).view(np.float32)
        case["model"][key] = nm.normalize(case["x"], out, g.view(nm.GROUP_DTYPE), params_of(name, nm))
    return case["model"][key]


def params_of(name, where):
    mode = {"standard0": "standard", "whisper": "dynamic_range"}.get(name, name)
    kw = dict(PARAMS[name])
    if where is nm:
        return nm.params(getattr(nm, mode.upper()), **kw)
    return afgpu.norm_params(name if name == "whisper" else mode, **kw)


def run(case, name, d_in, d_out, out_floats, d_groups=None):
    g = case["d_groups"] if d_groups is None else d_groups
    partials = torch.full((case["tiles"] * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    stats = torch.full((len(SHAPES) * 40,), 0xAB, dtype=torch.uint8, device="cuda")
    afgpu.normalize(len(SHAPES), g, case["tiles"], params_of(name, afgpu), d_in, d_in.numel(), d_out, out_floats, partials, stats)
    torch.cuda.synchronize()
    return stats.cpu().numpy().view(afgpu.NORM_STATS_DTYPE), partials


def sentinel_plane(n):
    return torch.from_numpy(np.full(n, SENTINEL, np.uint32).view(np.float32)).cuda()


@pytest.mark.parametrize("name", [n for n in PARAMS if n != "none"])
def test_statistics_and_output_are_the_models_bit_for_bit(case, name):
    d_out = sentinel_plane(case["n_out"])
    stats, _ = run(case, name, case["d_x"], d_out, case["n_out"])
    want_plane, want_stats = model(case, name)
    assert nm.same_stats(stats, want_stats) == []
    got = d_out.cpu().numpy()
    bad = nm.same_bits(got, want_plane)                          # the sentinel's bits outside the valid elements included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
    untouched = want_plane.view(np.uint32) == SENTINEL
    assert untouched.sum() == case["n_out"] - int((case["groups"]["rows"].astype(np.int64) * case["groups"]["valid"]).sum())
    assert (case["d_x"].cpu().numpy().view(np.uint32) == case["x"].view(np.uint32)).all()


def test_degenerate_groups_are_as_the_definition_says(case):
    groups, x = case["groups"], case["x"]
    for name in ("peak", "rms"):
        plane, stats = model(case, name)
        for k in (ZERO, WITH_INF):                               # scale 1: the input's bits
            g = groups[k]
            assert stats[k]["scale"] == 1 and stats[k]["offset"] == 0
            a, b, n = int(g["in_off"]), int(g["out_off"]), int(g["valid"])
            assert (plane[b:b + n].view(np.uint32) == x[a:a + n].view(np.uint32)).all()
    _, stats = model(case, "standard")
    assert stats[ZERO]["sum"] == 0 and stats[ZERO]["min"] == 0 and stats[ZERO]["max"] == 0 and stats[ZERO]["count"] == 300
    assert np.isnan(stats[WITH_NAN]["sum"]) and np.isnan(stats[WITH_NAN]["sumsq"]) and np.isnan(stats[WITH_NAN]["offset"])
    assert np.isfinite(stats[WITH_NAN]["min"]) and np.isfinite(stats[WITH_NAN]["max"]) and stats[WITH_NAN]["min"] < stats[WITH_NAN]["max"]
    assert stats[WITH_INF]["max"] == np.inf and stats[WITH_INF]["sum"] == np.inf and np.isfinite(stats[WITH_INF]["min"])
    assert stats[0].tobytes() == bytes(40)                       # valid == 0: a record of zeros
    # (the device's records and planes equal these: test_statistics_and_output_are_the_models_bit_for_bit)


def test_in_place(case):
    g = case["groups"].copy()
    g["out_off"] = g["in_off"]
    d_groups = torch.from_numpy(g.view(np.uint8).copy()).cuda()
    for name in ("standard", "whisper"):
        d = case["d_x"].clone()
        stats, _ = run(case, name, d, d, d.numel(), d_groups)
        want_plane, want_stats = model(case, name, in_place=True)
        assert nm.same_stats(stats, want_stats) == []
        bad = nm.same_bits(d.cpu().numpy(), want_plane)
        assert bad.size == 0, (bad.size, bad[:5].tolist())


def test_statistics_only_needs_no_output(case):
    stats, partials = run(case, "none", case["d_x"], None, 0)
    _, want = model(case, "none")
    assert nm.same_stats(stats, want) == []
    assert (stats["offset"][1:] == 0).all() and (stats["scale"][1:] == 1).all()
    # a tile's partial is its sums, min and max
    p = partials.cpu().numpy().view(np.dtype([("sum", np.float64), ("sumsq", np.float64), ("min", np.float32), ("max", np.float32), ("pad", np.uint32, (2,))]))
    g = case["groups"][3]                                        # one row of 255 floats: one tile
    row = case["x"][int(g["in_off"]):int(g["in_off"]) + 255]
    s, q = nm.tile_sums(np.ascontiguousarray(row))
    t = p[int(g["first_tile"])]
    assert (t["sum"], t["sumsq"], t["min"], t["max"]) == (s, q, row.min(), row.max())


def test_a_bad_record_is_refused_and_nothing_is_written(case):
    for change in (dict(in_off=case["x"].size - 10), dict(out_off=case["n_out"] - 10), dict(rows=0), dict(first_tile=1)):
        g = case["groups"].copy()
        for k, v in change.items():
            g[5][k] = v
        d_groups = torch.from_numpy(g.view(np.uint8).copy()).cuda()
        d_out = sentinel_plane(case["n_out"])
        partials = torch.full((case["tiles"] * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        stats = torch.full((len(SHAPES) * 40,), 0xAB, dtype=torch.uint8, device="cuda")
        with pytest.raises(afgpu.AfgError) as e:
            afgpu.normalize(len(SHAPES), d_groups, case["tiles"], params_of("peak", afgpu), case["d_x"], case["x"].size, d_out, case["n_out"], partials, stats)
        assert "group 5" in str(e.value)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (stats.cpu().numpy() == 0xAB).all() and (partials.cpu().numpy() == 0xAB).all()
        assert (case["d_x"].cpu().numpy().view(np.uint32) == case["x"].view(np.uint32)).all()


@pytest.mark.parametrize("lengths", RECORD_CASES)
def test_record_counts_and_groups_without_tiles(gpu, lengths):
    """1, 2 and 5 groups, with groups of no floats first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(37)
    valids = record_lengths(4096)[lengths]
    groups = np.zeros(len(valids), afgpu.NORM_GROUP_DTYPE)
    at = 3
    for k, valid in enumerate(valids):
        g, rows = groups[k], 1 + k % 2
        g["in_off"], g["out_off"], g["stride"], g["rows"], g["valid"] = at, at, valid + 5, rows, valid
        at += rows * (valid + 5) + 2
    n = at + 3
    tiles = afgpu.norm_layout(groups)
    x = rng.standard_normal(n).astype(np.float32)
    d_out = sentinel_plane(n)
    partials = torch.full((max(tiles, 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    stats = torch.full((len(valids) * 40,), 0xAB, dtype=torch.uint8, device="cuda")
    afgpu.normalize(len(valids), torch.from_numpy(groups.view(np.uint8).copy()).cuda(), tiles, params_of("peak", afgpu), torch.from_numpy(x).cuda(), n,
                    d_out, n, partials, stats)
    torch.cuda.synchronize()
    want_plane, want_stats = nm.normalize(x, np.full(n, SENTINEL, np.uint32).view(np.float32), groups.view(nm.GROUP_DTYPE), params_of("peak", nm))
    assert nm.same_stats(stats.cpu().numpy().view(afgpu.NORM_STATS_DTYPE), want_stats) == []
    bad = nm.same_bits(d_out.cpu().numpy(), want_plane)          # the sentinel's bits outside the valid elements included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
