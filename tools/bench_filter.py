"""Times the filter stage on the GPU: 1024 rows of 480 000 device-resident floats (30 s at 16 kHz) through afg_filter_hip with
cascades of 1, 2 and 8 sections, out of place and in place, beside afg_copy_probe_hip over the same bytes (every float read
once and written once).  The sides alternate in one process; medians of 5.  No ratio is promised and nothing gates on one.

    python tools/bench_filter.py [--rows 1024] [--out profiles/filter_bench.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
RATE, SAMPLES = 16000, 480000


def median(v):
    return sorted(v)[len(v) // 2]


def timer():
    import torch
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
    return timed


def cascades():
    import afgpu
    hp = afgpu.biquad("highpass", RATE, 80.0)
    lp = afgpu.biquad("lowpass", RATE, 7000.0)
    eight = [afgpu.biquad("lowpass", RATE, 0.1 * RATE, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / 32.0))) for k in range(8)]
    return {1: [hp], 2: [hp, lp], 8: eight}


def kernel_leg(n_rows):
    import torch
    import afgpu
    timed = timer()
    out = []
    x = torch.empty((n_rows, SAMPLES), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0)
    y = torch.empty_like(x)
    z = x.clone()
    rows = np.zeros(n_rows, afgpu.FILTER_ROW_DTYPE)
    rows["in_off"] = rows["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
    rows["frames"] = SAMPLES
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    nbytes = x.numel() * 4
    src, dst = x.view(torch.uint8).reshape(-1), y.view(torch.uint8).reshape(-1)
    for n_sec, sos in cascades().items():
        prm = afgpu.filter_params(sos)
        for in_place in (False, True):
            a, b = (z, z) if in_place else (x, y)

            def run_kernel():
                afgpu.filter_rows(n_rows, d_rows, prm, a, a.numel(), b, b.numel())

            tk, tc = [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit all alike
                tk.append(timed(run_kernel))
                tc.append(timed(lambda: afgpu.copy_probe(dst, src, nbytes)))
            sk, sc = median(tk), median(tc)
            out.append({"sections": n_sec, "in_place": in_place, "rows": n_rows, "frames": SAMPLES, "bytes_moved": 2 * nbytes,
                        "filter_seconds": sk, "copy_probe_seconds": sc, "filter_GBps_moved": 2 * nbytes / sk / 1e9,
                        "copy_GBps_moved": 2 * nbytes / sc / 1e9, "of_the_probe": sc / sk,
                        "samples_per_second": n_rows * SAMPLES / sk})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_filter.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through the public afg_filter_hip, which fetches the rows and waits for its stream before every launch "
                   "(the batch path checks its host copy and does not)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    res["kernel"] = kernel_leg(args.rows)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
