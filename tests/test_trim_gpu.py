"""afg_trim_hip (csrc/trim.hip) against tests/trim_model.py, as bit patterns: the blocks' powers, the region records and every
float of the output plane -- the sentinels round the slabs included -- for groups whose lengths sit on both sides of a block, a
frame and a tile, with one to three rows, every alignment of either plane and of `begin`, all groups of a case in one launch."""
import numpy as np
import pytest
import torch

import afgpu
import trim_model as tm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc00123                                            # a NaN no operation makes
GUARD = 0x7fc00456                                               # ... and another, round every input row
# (frame_length, hop, reference, lead, trail, top_db)
CASES = {"2048/512": (2048, 512, "max", 0, 0, 60.0), "2048/512 margins": (2048, 512, "max", 3, 7, 40.0),
         "2048/512 abs": (2048, 512, "abs", 0, 1, 30.0), "400/200": (400, 200, "max", 201, 0, 60.0), "320/160 abs": (320, 160, "abs", 2, 162, 25.0),
         "10/5": (10, 5, "max", 0, 0, 50.0), "64/64": (64, 64, "max", 1, 1, 60.0), "3/3": (3, 3, "max", 0, 2, 45.0)}
KINDS = ("burst",) * 8 + ("silent", "loud", "nan", "inf", "burst", "burst", "burst", "burst")


def place(at, residue):
    return at + (residue - at) % 4


def signal(rng, kind, rows, valid, hop, shift):
    x = np.zeros((rows, valid), np.float32)
    if kind == "silent" or valid == 0:
        return x
    loud = (rng.standard_normal((rows, valid)) * 0.3 * 10.0 ** rng.integers(-2, 1, (rows, valid))).astype(np.float32)
    if kind == "loud" or valid < 4:
        return loud
    a, b = valid // 3 + shift, valid - valid // 4
    x[:, a:b] = loud[:, a:b]
    if kind == "nan":
        x[rows - 1, a + (b - a) // 2] = np.nan
    if kind == "inf":
        x[0, a + (b - a) // 3] = np.inf
    return x


def build(name):
    fl, hop, reference, lead, trail, top_db = CASES[name]
    rng = np.random.default_rng(fl * 1000 + hop + lead)
    ref = tm.REF_ABS if reference == "abs" else tm.REF_MAX
    prm = tm.params(top_db, fl, hop, ref, 1.0, lead, trail)
    big = 3 * fl + hop + 1
    valids = [0, 1, hop - 1, hop, hop + 1, fl - 1, fl + 1, 2 * 4096 + 5, big, big, big, big, big + 1, big + 2, big + 3, 4 * fl + 2]
    groups = np.zeros(len(valids), afgpu.TRIM_GROUP_DTYPE)
    xs, a, b = [], 3, 5
    for i, valid in enumerate(valids):
        rows = 1 + i % 3
        x = signal(rng, KINDS[i], rows, valid, hop, i % 4)
        begin, end = tm.region(x, prm)[:2]
        n = end - begin
        out_frames = (max(n - 3, 0), n, n + 5)[i % 3] if n else (0, 5, 4097)[i % 3]
        if i == 7:
            out_frames = 2 * 4096 + 9                            # three tiles a row, the last one short and partly zero
        g = groups[i]
        a, b = place(a, i % 4), place(b, (i // 4 + i) % 4)
        g["in_off"], g["out_off"], g["rows"], g["valid"] = a, b, rows, valid
        g["in_stride"], g["out_stride"] = valid + 2 + i % 3, out_frames + 1 + i % 4
        g["out_rows"], g["out_frames"] = rows + i % 2, out_frames
        xs.append(x)
        a += rows * int(g["in_stride"]) + 2
        b += int(g["out_rows"]) * int(g["out_stride"]) + 3
    plane = np.full(a + 3, GUARD, np.uint32).view(np.float32)    # NaN guards round every row's valid part
    for g, x in zip(groups, xs):
        for r in range(x.shape[0]):
            at = int(g["in_off"]) + r * int(g["in_stride"])
            plane[at:at + x.shape[1]] = x[r]
    plane.setflags(write=False)
    n_out = b + 3
    blocks, tiles = afgpu.trim_layout(groups, afgpu.trim_params(top_db, fl, hop, reference, 1.0, lead, trail))
    mine = groups.view(tm.GROUP_DTYPE).copy()
    assert tm.layout(mine, prm) == (blocks, tiles) and (mine == groups.view(tm.GROUP_DTYPE)).all()
    sentinel = np.full(n_out, SENTINEL, np.uint32).view(np.float32)
    want_out, want_regions, want_powers = tm.trim(plane, sentinel, mine, prm)
    return {"groups": groups, "blocks": blocks, "tiles": tiles, "plane": plane, "n_out": n_out, "out": want_out, "regions": want_regions,
            "powers": want_powers, "params": afgpu.trim_params(top_db, fl, hop, reference, 1.0, lead, trail)}


def run(case, d_groups=None, d_in=None, d_out=None, out_floats=None):
    g = torch.from_numpy(case["groups"].view(np.uint8).copy()).cuda() if d_groups is None else d_groups
    d_in = torch.from_numpy(case["plane"].copy()).cuda() if d_in is None else d_in
    d_out = torch.from_numpy(np.full(case["n_out"], SENTINEL, np.uint32).view(np.float32)).cuda() if d_out is None else d_out
    powers = torch.full((max(case["blocks"], 1) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    regions = torch.full((len(case["groups"]) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    afgpu.trim(len(case["groups"]), g, case["blocks"], case["tiles"], case["params"], d_in, d_in.numel(), d_out,
               d_out.numel() if out_floats is None else out_floats, powers, regions)
    torch.cuda.synchronize()
    return d_in, d_out, powers, regions


@pytest.mark.parametrize("name", list(CASES))
def test_regions_and_slabs_are_the_models_bit_for_bit(gpu, name):
    case = build(name)
    d_in, d_out, powers, regions = run(case)
    got_powers = powers.cpu().numpy().view(np.float64)[:case["blocks"]]
    want = case["powers"]
    assert got_powers.size == want.size
    nan = np.isnan(want)
    assert (np.isnan(got_powers) == nan).all()
    assert tm.same_bits(got_powers[~nan], want[~nan]).size == 0
    got_regions = regions.cpu().numpy().view(afgpu.TRIM_REGION_DTYPE)
    for field in ("begin", "end", "ref_power"):
        bad = tm.same_bits(np.ascontiguousarray(got_regions[field]), np.ascontiguousarray(case["regions"][field]))
        assert bad.size == 0, (field, bad[:5].tolist(), got_regions[bad[:3]], case["regions"][bad[:3]])
    bad = tm.same_bits(d_out.cpu().numpy(), case["out"])         # the sentinel's bits outside the slabs included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
    assert (d_in.cpu().numpy().view(np.uint32) == case["plane"].view(np.uint32)).all()
    # what the case covers
    g, r = case["groups"], case["regions"]
    n = r["end"].astype(np.int64) - r["begin"]
    assert (n[:8] >= 0).all() and (n[12:] > 0).all() and n[8] == 0 and n[9] == g["valid"][9]      # all silent; all loud
    assert {int(v) % 4 for v in g["in_off"]} == {0, 1, 2, 3} == {int(v) % 4 for v in g["out_off"]}
    assert (g["out_frames"] < n).any() and (g["out_frames"] == n).any() and (g["out_frames"] > n).any()
    assert np.isnan(want).any() and np.isinf(r["ref_power"]).any()
    if name in ("10/5", "3/3"):
        assert {int(v) % 4 for v in r["begin"][n > 0]} == {0, 1, 2, 3}, r["begin"]


def test_a_bad_record_or_overlapping_planes_are_refused_and_nothing_is_written(gpu):
    case = build("400/200")
    for change in (dict(in_off=case["plane"].size - 10), dict(out_off=case["n_out"] - 10), dict(rows=0), dict(out_rows=0), dict(first_tile=1),
                   dict(first_block=1)):
        g = case["groups"].copy()
        for k, v in change.items():
            g[5][k] = v
        with pytest.raises(afgpu.AfgError) as e:
            run(case, d_groups=torch.from_numpy(g.view(np.uint8).copy()).cuda())
        assert "afg_trim_group 5" in str(e.value), change
    g = torch.from_numpy(case["groups"].view(np.uint8).copy()).cuda()
    d_in = torch.from_numpy(case["plane"].copy()).cuda()
    d_out = torch.from_numpy(np.full(case["n_out"], SENTINEL, np.uint32).view(np.float32)).cuda()
    powers = torch.full((case["blocks"] * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    regions = torch.full((len(case["groups"]) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    bad = case["groups"].copy()
    bad[3]["valid"] += 1                                         # (its first_block no longer fits the next group's)
    with pytest.raises(afgpu.AfgError):
        afgpu.trim(len(bad), torch.from_numpy(bad.view(np.uint8).copy()).cuda(), case["blocks"], case["tiles"], case["params"], d_in, d_in.numel(),
                   d_out, d_out.numel(), powers, regions)
    # one allocation, the output plane beginning inside the input plane's last floats
    both = torch.from_numpy(np.concatenate([case["plane"], np.full(case["n_out"], SENTINEL, np.uint32).view(np.float32)])).cuda()
    n_in = case["plane"].size
    for lo in (n_in - 1, n_in - 100, 0):
        with pytest.raises(afgpu.AfgError) as e:
            afgpu.trim(len(case["groups"]), g, case["blocks"], case["tiles"], case["params"], both[:n_in], n_in, both[lo:lo + case["n_out"]],
                       case["n_out"], powers, regions)
        assert "overlaps" in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert (powers.cpu().numpy() == 0xAB).all() and (regions.cpu().numpy() == 0xAB).all()
    assert (both.cpu().numpy()[:n_in].view(np.uint32) == case["plane"].view(np.uint32)).all()
    assert (both.cpu().numpy()[n_in:].view(np.uint32) == SENTINEL).all()
    # side by side in one allocation is no overlap
    _, d_out, _, _ = run(case, d_in=both[:n_in], d_out=both[n_in:])
    assert tm.same_bits(d_out.cpu().numpy(), case["out"]).size == 0


@pytest.mark.parametrize("lengths", RECORD_CASES)
def test_record_counts_and_groups_without_blocks_or_tiles(gpu, lengths):
    """1, 2 and 5 groups, with groups of no samples and no output first, in the middle and last (record_cases.py): the edges of
    the search by block and of the search by tile"""
    fl, hop = 2048, 512
    rng = np.random.default_rng(41)
    prm, lib_prm = tm.params(60.0, fl, hop, tm.REF_MAX, 1.0, 0, 0), afgpu.trim_params(60.0, fl, hop, "max", 1.0, 0, 0)
    valids = record_lengths(4096)[lengths]
    groups = np.zeros(len(valids), afgpu.TRIM_GROUP_DTYPE)
    xs, a, b = [], 3, 5
    for i, valid in enumerate(valids):
        g, rows = groups[i], 1 + i % 2
        xs.append(signal(rng, "loud", rows, valid, hop, 0))
        g["in_off"], g["out_off"], g["rows"], g["valid"] = a, b, rows, valid
        g["in_stride"], g["out_stride"], g["out_rows"], g["out_frames"] = valid + 2, valid + 1, rows, valid
        a += rows * (valid + 2) + 2
        b += rows * (valid + 1) + 3
    plane = np.full(a + 3, GUARD, np.uint32).view(np.float32)
    for g, x in zip(groups, xs):
        for r in range(x.shape[0]):
            at = int(g["in_off"]) + r * int(g["in_stride"])
            plane[at:at + x.shape[1]] = x[r]
    blocks, tiles = afgpu.trim_layout(groups, lib_prm)
    assert blocks == sum(-(-v // hop) for v in valids) and tiles == sum((1 + i % 2) * -(-v // 4096) for i, v in enumerate(valids))
    want_out, want_regions, want_powers = tm.trim(plane, np.full(b + 3, SENTINEL, np.uint32).view(np.float32), groups.view(tm.GROUP_DTYPE).copy(), prm)
    case = {"groups": groups, "blocks": blocks, "tiles": tiles, "plane": plane, "n_out": b + 3, "params": lib_prm}
    d_in, d_out, powers, regions = run(case)
    assert tm.same_bits(powers.cpu().numpy().view(np.float64)[:blocks], want_powers).size == 0
    got_regions = regions.cpu().numpy().view(afgpu.TRIM_REGION_DTYPE)
    for field in ("begin", "end", "ref_power"):
        assert tm.same_bits(np.ascontiguousarray(got_regions[field]), np.ascontiguousarray(want_regions[field])).size == 0, field
    bad = tm.same_bits(d_out.cpu().numpy(), want_out)            # the sentinel's bits outside the slabs included
    assert bad.size == 0, (bad.size, bad[:5].tolist())
