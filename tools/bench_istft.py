#!/usr/bin/env python3
"""tools/bench_istft.py -- what the inverse STFT stage costs, written to profiles/istft_bench.json.

Slabs of device-resident complex64 spectra to rows of 30 s at 16 kHz: [201, 3000] with Whisper's framing (n_fft 400, hop 160,
479 840 samples) and [513, 1876] with n_fft 1024, hop 256 (480 000 samples).  afgpu.istft_tensor -- the public entry, which
lays the records out, uploads them and lets afg_istft_hip fetch and check them before the launch -- beside torch.istft on
the same complex tensor and afg_copy_probe_hip over the bytes the stage must move (slab once, row once), all alternating in
one process, medians of 5.  The largest |ours - torch.istft| over a few rows is informational.  No ratio is promised and
nothing gates on one.

    python tools/bench_istft.py [--rows 1024] [--out profiles/istft_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
SHAPES = [dict(n_fft=400, hop=160, frames=3000), dict(n_fft=1024, hop=256, frames=1876)]


def median(v):
    return sorted(v)[len(v) // 2]


def run(n_rows):
    import torch
    import afgpu
    out = []
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

    for s in SHAPES:
        n_fft, hop, frames, n_bins = s["n_fft"], s["hop"], s["frames"], s["n_fft"] // 2 + 1
        length = hop * (frames - 1)
        spec = torch.view_as_complex(torch.empty((n_rows, n_bins, frames, 2), dtype=torch.float32, device="cuda").normal_())
        window = torch.hann_window(n_fft, periodic=True, device="cuda")
        y = torch.empty((n_rows, length), dtype=torch.float32, device="cuda")
        prm = afgpu.istft_params(n_fft, hop)

        def ours():
            afgpu.istft_tensor(spec, n_fft, hop, out=y)

        def theirs():
            return torch.istft(spec, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, length=length)

        ours()
        few = min(n_rows, 8)
        worst = float((y[:few] - torch.istft(spec[:few], n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, length=length)).abs().max().item())
        moved = int(spec.numel() * 8 + y.numel() * 4)
        probe_bytes = moved // 2 // 16 * 16                        # the probe reads and writes what it is given
        src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
        to, tt, tc = [], [], []
        for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit all alike
            to.append(timed(ours))
            tt.append(timed(theirs))
            tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
        so, st, sc = median(to), median(tt), median(tc)
        tile = afgpu.istft_tile_samples(prm)
        out.append({"n_fft": n_fft, "hop": hop, "rows": n_rows, "frames": frames, "samples": length, "tile_samples": tile,
                    "tiles": n_rows * -(-length // tile), "bytes_moved": moved, "istft_seconds": so, "torch_seconds": st, "copy_probe_seconds": sc,
                    "istft_GBps_moved": moved / so / 1e9, "copy_GBps_moved": 2 * probe_bytes / sc / 1e9, "of_the_probe": sc / so,
                    "torch_over_istft": st / so, "max_abs_difference_to_torch": worst})
        print(json.dumps(out[-1]), flush=True)
        del spec, y, src, dst
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "istft_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_istft.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through afgpu.istft_tensor: record layout, upload, afg_istft_hip's fetch and checks, one launch; unit-variance complex noise"}
    res["kernel"] = run(args.rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
