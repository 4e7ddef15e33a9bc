#!/usr/bin/env python3
"""tools/bench_convolve.py -- what the convolution stage costs, written to profiles/convolve_bench.json.

Rows of 30 s at 16 kHz (480 000 samples), device resident, convolved to rows of the same length (mode "same") with kernels
of 2, 64 and 128 taps (the direct path) and 129, 4 000, 16 000 and 32 000 taps (the FFT path), once with one kernel shared
by all rows and once with a kernel per row.  afgpu.convolve_tensor -- the public entry, which lays the records out, uploads
them, allocates the work plane and lets afg_convolve_hip fetch and check the records before its launches -- beside the
torch.fft.rfft * product * irfft * crop expression on the same tensors, torch.nn.functional.conv1d for the kernels of at
most 128 taps, and afg_copy_probe_hip over the bytes the stage must move (row once in, row once out), all alternating in
one process, medians of 3.  The bank transform (ConvolveBank) is timed on its own.  The largest |ours - torch| over a few
rows is informational.  No ratio is promised and nothing gates on one.

    python tools/bench_convolve.py [--rows 1024] [--out profiles/convolve_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 3
FRAMES = 480000
TAPS = [2, 64, 128, 129, 4000, 16000, 32000]


def median(v):
    return sorted(v)[len(v) // 2]


def run(n_rows):
    import numpy as np
    import torch
    import torch.nn.functional as F
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

    x = torch.empty((n_rows, FRAMES), dtype=torch.float32, device="cuda").normal_()
    y = torch.empty_like(x)
    moved = int(x.numel() * 4 + y.numel() * 4)
    probe_bytes = moved // 2 // 16 * 16                           # the probe reads and writes what it is given
    src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
    for taps in TAPS:
        for per_row in (False, True):
            n_k = n_rows if per_row else 1
            decay = torch.exp(-3.0 * torch.arange(taps, device="cuda") / taps)
            h = (torch.empty((n_k, taps), dtype=torch.float32, device="cuda").normal_() * decay).contiguous()
            hs = [k for k in h.cpu().numpy()]
            bank = afgpu.ConvolveBank(hs)
            t_bank = timed(lambda: afgpu.convolve_bank(n_k, bank.d_records, bank.bank, bank.bank.numel(), bank.spec, bank.spec_floats))
            kernel = torch.arange(n_rows) if per_row else 0
            first = (taps - 1) // 2
            n_fft = 1 << (FRAMES + taps - 2).bit_length()

            def ours():
                afgpu.convolve_tensor(x, bank, kernel, "same", out=y)

            def by_fft(xx=x, hh=h):
                return torch.fft.irfft(torch.fft.rfft(xx, n_fft) * torch.fft.rfft(hh, n_fft), n_fft)[..., first:first + FRAMES]

            def by_conv1d():
                if per_row:
                    return F.conv1d(x[None], h.flip(-1)[:, None, :], padding=taps - 1, groups=n_rows)[0, :, first:first + FRAMES]
                return F.conv1d(x[:, None, :], h.flip(-1)[None], padding=taps - 1)[:, 0, first:first + FRAMES]

            ours()
            few = min(n_rows, 4)
            worst = float((y[:few] - by_fft(x[:few], h[:few] if per_row else h)).abs().max().item())
            rows = np.zeros(1, afgpu.CONV_ROW_DTYPE)
            rows["frames"], rows["out_first"], rows["out_frames"] = FRAMES, first, FRAMES
            _, work_row = afgpu.convolve_layout(rows, bank.records[:1].copy(), afgpu.convolve_params())
            to, tt, tc, t1 = [], [], [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit all alike
                to.append(timed(ours))
                tt.append(timed(by_fft))
                tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
                if taps <= 128:
                    t1.append(timed(by_conv1d))
            so, st, sc = median(to), median(tt), median(tc)
            rec = {"taps": taps, "path": "direct" if taps <= 128 else "fft", "kernels": n_k, "rows": n_rows, "frames": FRAMES,
                   "partitions": -(-taps // 1024), "bytes_moved": moved, "work_plane_bytes": 4 * work_row * n_rows, "convolve_seconds": so,
                   "torch_fft_seconds": st, "copy_probe_seconds": sc, "bank_transform_seconds": t_bank, "convolve_GBps_moved": moved / so / 1e9,
                   "copy_GBps_moved": 2 * probe_bytes / sc / 1e9, "of_the_probe": sc / so, "torch_fft_over_convolve": st / so,
                   "max_abs_difference_to_torch_fft": worst}
            if t1:
                rec["torch_conv1d_seconds"] = median(t1)
                rec["torch_conv1d_over_convolve"] = median(t1) / so
            out.append(rec)
            print(json.dumps(rec), flush=True)
            del bank, h, hs
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_convolve.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through afgpu.convolve_tensor: record layout, upload, the work plane's allocation, afg_convolve_hip's fetch and "
                   "checks, one launch (direct) or two (FFT); unit-variance noise rows, decaying-noise kernels; mode same"}
    res["kernel"] = run(args.rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
