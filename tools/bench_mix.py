#!/usr/bin/env python3
"""tools/bench_mix.py -- what the mixing stage costs, written to profiles/mix_bench.json.

1024 rows of 480 000 device-resident floats (30 s at 16 kHz), one and two rows a group, out of place, at 10 dB, against a
bank of 64 clips of 10 s (160 000 samples: every row loops its clip three times) and of 30 s (480 000: one pass, wrapping
once from the start position): afg_mix_hip beside afg_copy_probe_hip over the same bytes (one read and one write of the
plane) and beside the torch expression on the same tensors -- the clip of every group repeated to the row's length and rolled
to its start, then torchaudio.functional.add_noise's lines (the two energies, their logarithms, the scale, the sum).  The
sides alternate in one process; medians of 5.  The stage reads the plane and the noise under it twice (statistics, then
apply) and writes the plane once; the copy reads and writes once.  No ratio is promised and nothing gates on one.

    python tools/bench_mix.py [--rows 1024] [--out profiles/mix_bench.json]
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
CLIPS = 64
SNR_DB = 10.0
START = 12345                                                    # the same for every group: torch.roll takes one shift


def median(v):
    return sorted(v)[len(v) // 2]


def torch_expression(x, bank, index, rows, snr_db):
    """x [groups * rows, T]; the noise of a group's clip under every one of its rows, then add_noise's lines per group"""
    import torch
    T, N = x.shape[1], bank.shape[1]
    noise = torch.roll(bank[index].repeat(1, -(-T // N)), -START, 1)[:, :T]     # (whole periods: the roll wraps as the clip does)
    noise = noise.repeat_interleave(rows, 0) if rows > 1 else noise
    xs, ns = x.reshape(-1, rows * T), noise.reshape(-1, rows * T)
    energy_signal = torch.linalg.vector_norm(xs, ord=2, dim=-1) ** 2
    energy_noise = torch.linalg.vector_norm(ns, ord=2, dim=-1) ** 2
    original_snr_db = 10 * (torch.log10(energy_signal) - torch.log10(energy_noise))
    scale = 10 ** ((original_snr_db - snr_db) / 20.0)
    return (xs + scale.unsqueeze(-1) * ns).reshape(x.shape)


def leg(n_rows, rows, clip_samples):
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

    n = n_rows // rows
    x = torch.empty((n_rows, SAMPLES), dtype=torch.float32, device="cuda").normal_() * 0.1
    bank = torch.empty((CLIPS, clip_samples), dtype=torch.float32, device="cuda").normal_() * 0.03
    y = torch.empty_like(x)
    index = np.arange(n) % CLIPS
    d_index = torch.from_numpy(index).cuda()
    groups = np.zeros(n, afgpu.MIX_GROUP_DTYPE)
    groups["in_off"] = groups["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(rows * SAMPLES)
    groups["stride"], groups["rows"], groups["valid"] = SAMPLES, rows, SAMPLES
    groups["noise_off"] = index.astype(np.uint64) * np.uint64(clip_samples)
    groups["noise_len"], groups["noise_start"], groups["noise_stride"] = clip_samples, START % clip_samples, 0
    groups["flags"], groups["ratio"] = afgpu.MIX_SNR, afgpu.mix_ratio(SNR_DB)
    tiles = afgpu.mix_layout(groups)
    d_groups = torch.from_numpy(groups.view(np.uint8).copy()).cuda()
    d_partials = torch.empty(tiles * 2, dtype=torch.float64, device="cuda")
    d_stats = torch.empty(n * afgpu.MIX_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    nbytes = x.numel() * 4

    def run_kernel():
        afgpu.mix(n, d_groups, tiles, x, x.numel(), bank, bank.numel(), y, y.numel(), d_partials, d_stats)

    def run_copy():
        afgpu.copy_probe(y, x, nbytes)

    def run_torch():
        return torch_expression(x, bank, d_index, rows, SNR_DB)

    run_kernel()
    torch.cuda.synchronize()
    stats = d_stats.cpu().numpy().view(afgpu.MIX_STATS_DTYPE)
    worst = float((run_torch() - y).abs().max().item())
    tk, tc, tt = [], [], []
    for _ in range(PASSES):                                      # alternating, so that clocks and neighbours hit all alike
        tk.append(timed(run_kernel))
        tc.append(timed(run_copy))
        tt.append(timed(run_torch))
    sk, sc, st = median(tk), median(tc), median(tt)
    out = {"rows_per_group": rows, "groups": n, "floats_per_row": SAMPLES, "clips": CLIPS, "clip_samples": clip_samples, "tiles": tiles,
           "plane_bytes": nbytes, "snr_db": SNR_DB, "flags_set": int((stats["flags"] != 0).sum()), "max_abs_difference_from_torch": worst,
           "mix_seconds": sk, "copy_probe_seconds": sc, "torch_seconds": st, "mix_over_copy": sk / sc, "torch_over_mix": st / sk,
           "mix_GBps_moved": 5 * nbytes / sk / 1e9, "copy_GBps_moved": 2 * nbytes / sc / 1e9}
    print(json.dumps(out), flush=True)
    del x, y, bank
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_mix.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through the public afg_mix_hip, which fetches the groups and waits for its stream before every launch (the batch "
                   "path checks its host copy and does not); mix_GBps_moved counts two reads of the plane, two of the noise under it and "
                   "one write",
           "legs": []}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for rows in (1, 2):
        for clip_samples in (160000, 480000):
            res["legs"].append(leg(args.rows, rows, clip_samples))
            with open(args.out, "w") as fh:                      # after every leg: a later one that fails loses nothing
                json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
