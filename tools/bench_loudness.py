"""Times the loudness stage on the GPU: 1024 rows of 480 000 device-resident floats (30 s at 16 kHz), one and two rows to the
group, through afg_loudness_hip measuring only and measuring and applying the gain in place, beside
  - afg_copy_probe_hip over the bytes each must move: the input once; the input twice and the output once;
  - the composition the stage replaces: afg_filter_hip with the K-weighting into a scratch tensor, then afg_normalize_hip's
    statistics (AFG_NORM_NONE) over the scratch -- which still lacks the blocks and the gates;
  - for orientation, that filter launch followed by the blocks and gates as a torch expression.
The sides alternate in one process; medians of 5.  No ratio is promised and nothing gates on one.

    python tools/bench_loudness.py [--rows 1024] [--out profiles/loudness_bench.json]
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

from bench_filter import median, timer

PASSES = 5
RATE, SAMPLES = 16000, 480000
GAMMA_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)


def torch_gates(v, per_group):
    """block energies, both gates and the energy of the K-weighted tensor v [rows, SAMPLES], rows in groups of per_group"""
    import torch
    step = (RATE + 5) // 10
    n = SAMPLES // step
    sub = (v[:, :n * step].double() ** 2).view(-1, per_group, n, step).sum(dim=(1, 3))
    z = (sub[:, :-3] + sub[:, 1:-2] + sub[:, 2:-1] + sub[:, 3:]) / (4 * step)
    above = z > GAMMA_ABS
    rel = 0.1 * (z * above).sum(1) / above.sum(1).clamp(min=1)
    gated = above & (z > rel[:, None])
    return (z * gated).sum(1) / gated.sum(1).clamp(min=1)


def kernel_leg(n_rows):
    import torch
    import afgpu
    timed = timer()
    out = []
    x = torch.empty((n_rows, SAMPLES), dtype=torch.float32, device="cuda").uniform_(-0.5, 0.5)
    scratch = torch.empty_like(x)
    nbytes = x.numel() * 4
    src = torch.empty(3 * nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    kw = afgpu.filter_params(afgpu.kweight_design(RATE))
    frows = np.zeros(n_rows, afgpu.FILTER_ROW_DTYPE)
    frows["in_off"] = frows["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
    frows["frames"] = SAMPLES
    d_frows = torch.from_numpy(frows.view(np.uint8).copy()).cuda()
    for per_group in (1, 2):
        n_groups = n_rows // per_group
        groups = np.zeros(n_groups, afgpu.LOUDNESS_GROUP_DTYPE)
        groups["in_off"] = groups["out_off"] = np.arange(n_groups, dtype=np.uint64) * np.uint64(per_group * SAMPLES)
        groups["stride"], groups["rows"], groups["valid"] = SAMPLES, per_group, SAMPLES
        measure, both = afgpu.loudness_params(RATE, apply=False), afgpu.loudness_params(RATE, target_lufs=-23.0, max_gain=1.0)
        counts = afgpu.loudness_layout(groups, measure)
        d_groups = torch.from_numpy(groups.view(np.uint8).copy()).cuda()
        d_sub = torch.empty(counts.n_sub, dtype=torch.float64, device="cuda")
        d_blocks = torch.empty(counts.n_blocks, dtype=torch.float64, device="cuda")
        d_stats = torch.zeros(n_groups * afgpu.LOUDNESS_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        work = x.clone()                                         # (max_gain 1: applying in place over and over never grows the samples)
        ngroups = np.zeros(n_groups, afgpu.NORM_GROUP_DTYPE)
        ngroups["in_off"] = ngroups["out_off"] = groups["in_off"]
        ngroups["stride"], ngroups["rows"], ngroups["valid"] = SAMPLES, per_group, SAMPLES
        n_tiles = afgpu.norm_layout(ngroups)
        d_ngroups = torch.from_numpy(ngroups.view(np.uint8).copy()).cuda()
        d_partials = torch.empty(n_tiles * 32, dtype=torch.uint8, device="cuda")
        d_nstats = torch.zeros(n_groups * afgpu.NORM_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        none = afgpu.norm_params("none")

        def run_measure():
            afgpu.loudness(n_groups, d_groups, counts, measure, x, x.numel(), None, 0, d_sub, d_blocks, d_stats)

        def run_both():
            afgpu.loudness(n_groups, d_groups, counts, both, work, work.numel(), work, work.numel(), d_sub, d_blocks, d_stats)

        def run_filter():
            afgpu.filter_rows(n_rows, d_frows, kw, x, x.numel(), scratch, scratch.numel())

        def run_composition():
            run_filter()
            afgpu.normalize(n_groups, d_ngroups, n_tiles, none, scratch, scratch.numel(), None, 0, d_partials, d_nstats)

        def run_torch():
            run_filter()
            torch_gates(scratch, per_group)

        t = {k: [] for k in ("measure", "measure_apply", "probe_read", "probe_apply", "composition", "torch")}
        for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit all alike
            t["measure"].append(timed(run_measure))
            t["probe_read"].append(timed(lambda: afgpu.copy_probe(dst, src, nbytes // 2)))
            t["measure_apply"].append(timed(run_both))
            t["probe_apply"].append(timed(lambda: afgpu.copy_probe(dst, src, 3 * nbytes // 2)))
            t["composition"].append(timed(run_composition))
            t["torch"].append(timed(run_torch))
        s = {k: median(v) for k, v in t.items()}
        stats = d_stats.cpu().numpy().view(afgpu.LOUDNESS_STATS_DTYPE)
        out.append({"rows_per_group": per_group, "rows": n_rows, "frames": SAMPLES, "input_bytes": nbytes,
                    "measure_seconds": s["measure"], "measure_apply_seconds": s["measure_apply"],
                    "copy_probe_input_once_seconds": s["probe_read"], "copy_probe_input_twice_and_output_seconds": s["probe_apply"],
                    "filter_plus_normalize_statistics_seconds": s["composition"], "filter_plus_torch_gates_seconds": s["torch"],
                    "measure_of_the_probe": s["probe_read"] / s["measure"], "measure_apply_of_the_probe": s["probe_apply"] / s["measure_apply"],
                    "composition_over_measure": s["composition"] / s["measure"], "torch_over_measure": s["torch"] / s["measure"],
                    "samples_per_second_measure": n_rows * SAMPLES / s["measure"],
                    "first_group_lufs": afgpu.loudness_lufs(float(stats[0]["energy"]))})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_loudness.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through the public entries, which fetch their records and wait for their stream before every launch "
                   "(the batch path checks its host copy and does not)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    res["kernel"] = kernel_leg(args.rows)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
