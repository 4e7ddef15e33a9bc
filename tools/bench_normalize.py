#!/usr/bin/env python3
"""tools/bench_normalize.py -- what the normalisation stage costs, written to profiles/normalize_bench.json.

(a) kernel leg: 1024 rows of 480 000 device-resident floats (30 s at 16 kHz), every row a group, in each mode:
    afg_normalize_hip beside afg_copy_probe_hip over the same bytes (one read and one write of the plane) and beside the
    equivalent torch expression on the same tensor.
(b) mel leg: 1024 slabs of [80, 3000] floats, every slab a group, in the dynamic-range mode with Whisper's numbers, against
    the same two.
The sides alternate in one process; medians of 5.  The stage reads the plane twice (statistics, then apply) and writes it
once, the copy reads and writes once.  No ratio is promised and nothing gates on one.

    python tools/bench_normalize.py [--rows 1024] [--slabs 1024] [--out profiles/normalize_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
SAMPLES = 480000
MEL = (80, 3000)


def median(v):
    return sorted(v)[len(v) // 2]


def torch_expression(mode, x, prm):
    import torch
    if mode == "none":
        return torch.sum(x, 1), torch.sum(x * x, 1), torch.amin(x, 1), torch.amax(x, 1)
    if mode == "peak":
        return x * (prm.target / x.abs().amax(1, keepdim=True))
    if mode == "rms":
        return x * (prm.target / x.pow(2).mean(1, keepdim=True).sqrt())
    if mode == "standard":
        return (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-7)
    return (torch.maximum(x, x.amax(1, keepdim=True) - prm.range) + prm.shift) * prm.gain


def leg(n_rows, row_floats, modes, make):
    """n_rows groups of one row of row_floats each, out of place"""
    import torch
    import afgpu
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps=2):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3 / reps

    x = make(torch.empty((n_rows, row_floats), dtype=torch.float32, device="cuda"))
    y = torch.empty_like(x)
    groups = np.zeros(n_rows, afgpu.NORM_GROUP_DTYPE)
    groups["in_off"] = groups["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(row_floats)
    groups["stride"], groups["rows"], groups["valid"] = row_floats, 1, row_floats
    tiles = afgpu.norm_layout(groups)
    d_groups = torch.from_numpy(groups.view(np.uint8).copy()).cuda()
    d_partials = torch.empty(tiles * 32, dtype=torch.uint8, device="cuda")
    d_stats = torch.empty(n_rows * afgpu.NORM_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    nbytes = x.numel() * 4
    out = []
    for mode in modes:
        prm = afgpu.norm_params(mode)

        def run_kernel():
            afgpu.normalize(n_rows, d_groups, tiles, prm, x, x.numel(), None if mode == "none" else y, y.numel(), d_partials, d_stats)

        def run_copy():
            afgpu.copy_probe(y, x, nbytes)

        def run_torch():
            return torch_expression(mode, x, prm)

        run_kernel()
        worst = None
        if mode != "none":
            worst = float((run_torch() - y).abs().max().item())
        tk, tc, tt = [], [], []
        for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit all alike
            tk.append(timed(run_kernel))
            tc.append(timed(run_copy))
            tt.append(timed(run_torch))
        sk, sc, st = median(tk), median(tc), median(tt)
        passes = 1 if mode == "none" else 3                       # plane reads and writes of the stage
        out.append({"mode": mode, "groups": n_rows, "floats_per_group": row_floats, "tiles": tiles, "plane_bytes": nbytes,
                    "max_abs_difference_from_torch": worst, "normalize_seconds": sk, "copy_probe_seconds": sc, "torch_seconds": st,
                    "normalize_over_copy": sk / sc, "torch_over_normalize": st / sk, "normalize_GBps_moved": passes * nbytes / sk / 1e9,
                    "copy_GBps_moved": 2 * nbytes / sc / 1e9})
        print(json.dumps(out[-1]), flush=True)
    del x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--slabs", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_normalize.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through the public afg_normalize_hip, which fetches the groups and waits for its stream before every launch "
                   "(the batch path checks its host copy and does not)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():                                                    # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    res["kernel"] = leg(args.rows, SAMPLES, ["none", "peak", "rms", "standard", "dynamic_range"], lambda t: t.normal_() * 0.1)
    save()
    res["mel"] = leg(args.slabs, MEL[0] * MEL[1], ["whisper"], lambda t: t.uniform_(-10.0, 2.0))
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
