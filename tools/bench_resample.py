#!/usr/bin/env python3
"""tools/bench_resample.py -- what the tensor at one sample rate costs, written to profiles/resample_bench.json.

(a) kernel leg: 512 rows of 60 s device-resident input for 44100 -> 16000, 48000 -> 16000, 16000 -> 16000 and 44100 -> 48000,
    plain (one input row per output row) and mono from 2 rows: afg_resample_hip beside afg_copy_probe_hip over the same
    number of bytes read and written, alternating in one process, medians of 5.
(b) call leg: 1024 generated MP3 files (44.1 kHz stereo) into a [1024, 1, 160000] tensor at 16 kHz mono through
    afgpu.batch_decode_tensor_resampled, against afgpu.batch_decode_tensor at the files' rate followed by a mean over the
    channels and one strided torch.nn.functional.conv1d with the same taps (a kernel per output phase, stride M).  The two
    alternate in one process; medians of 5.

    python tools/bench_resample.py [--rows 512] [--call-files 1024] [--distinct 32] [--out profiles/resample_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
PAIRS = [(44100, 16000), (48000, 16000), (16000, 16000), (44100, 48000)]


def median(v):
    return sorted(v)[len(v) // 2]


def kernel_leg(n_rows, seconds=60):
    import torch
    import afgpu
    out = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e-3 / reps

    for in_rate, out_rate in PAIRS:
        taps, M, L, W = afgpu.resample_taps(in_rate, out_rate)
        n_in, n_out = seconds * in_rate, seconds * out_rate
        d_taps = torch.from_numpy(taps.reshape(-1).copy()).cuda() if taps.size else None
        for in_rows in (1, 2):
            stride = n_in + 3                                         # rows at no particular alignment
            d_in = torch.empty(n_rows * in_rows * stride + 8, dtype=torch.float32, device="cuda").normal_()
            d_out = torch.empty(n_rows * n_out, dtype=torch.float32, device="cuda")
            rec = np.zeros(n_rows, afgpu.RESAMPLE_ROW_DTYPE)
            rec["in_off"] = 1 + np.arange(n_rows, dtype=np.uint64) * np.uint64(in_rows * stride)
            rec["in_stride"], rec["in_rows"], rec["in_frames"] = stride, in_rows, n_in
            rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(n_out)
            rec["out_frames"], rec["M"], rec["L"], rec["W"] = n_out, M, L, W
            tiles = afgpu.resample_layout(rec)
            d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            read, written = n_rows * in_rows * n_in * 4, n_rows * n_out * 4
            half = (read + written) // 2 // 16 * 16                   # the probe reads and writes `half` bytes each
            p_src = torch.empty(half // 4, dtype=torch.float32, device="cuda").normal_()
            p_dst = torch.empty(half // 4, dtype=torch.float32, device="cuda")

            def run_kernel():
                afgpu.resample(n_rows, d_rec, tiles, d_in, d_in.numel(), d_taps, taps.size, d_out, d_out.numel())

            def run_probe():
                afgpu.copy_probe(p_dst, p_src, half)

            tk, tp = [], []
            for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit both alike
                tk.append(timed(run_kernel))
                tp.append(timed(run_probe))
            sk, sp = median(tk), median(tp)
            out.append({"in_rate": in_rate, "out_rate": out_rate, "in_rows": in_rows, "rows": n_rows, "seconds": seconds, "taps": 2 * W,
                        "phases": L, "bytes_read": read, "bytes_written": written, "resample_seconds": sk,
                        "resample_GBps": (read + written) / sk / 1e9, "out_samples_per_s": n_rows * n_out / sk,
                        "copy_probe_seconds": sp, "copy_probe_GBps": 2 * half / sp / 1e9, "resample_over_probe": sk / sp, "tiles": tiles})
            print(json.dumps(out[-1]), flush=True)
            del d_in, d_out, p_src, p_dst
            torch.cuda.empty_cache()
    return out


def call_leg(blobs, T, out_rate, in_rate, threads):
    """files of in_rate, stereo, to [files, 1, T] at out_rate, mono"""
    import torch
    import afgpu
    taps, M, L, W = afgpu.resample_taps(in_rate, out_rate)
    K = 2 * W
    # one kernel per output frame of a block of L: phase (i * M) % L, placed floor(i * M / L) input frames into the block
    width = K + (L - 1) * M // L
    kern = np.zeros((L, 1, width), np.float32)
    for i in range(L):
        kern[i, 0, i * M // L:i * M // L + K] = taps[(i * M) % L]
    d_kern = torch.from_numpy(kern).cuda()
    blocks = -(-T // L)
    T_in = (blocks - 1) * M + width - (W - 1)                        # input frames the T outputs reach
    out = torch.empty((len(blobs), 1, T), dtype=torch.float32, device="cuda")

    def old():
        t, _ = afgpu.batch_decode_tensor(blobs, T_in, 2, n_threads=threads)
        mono = t.mean(1, keepdim=True)
        mono = torch.nn.functional.pad(mono, (W - 1, 0))
        y = torch.nn.functional.conv1d(mono, d_kern, stride=M)      # [files, L, blocks]
        y = y.transpose(1, 2).reshape(len(blobs), 1, -1)[:, :, :T].contiguous()
        torch.cuda.synchronize()
        return y

    def new():
        t, _ = afgpu.batch_decode_tensor_resampled(blobs, T, 1, out_rate, mono=True, out=out, n_threads=threads)
        torch.cuda.synchronize()
        return t

    a, b = old(), new()                                              # warm-up; the two agree to float32 rounding, not bit for bit
    worst = float((a - b).abs().max().item())
    wall = {"old": [], "new": []}
    cpu = {"old": [], "new": []}
    for _ in range(PASSES):
        for name, fn in (("old", old), ("new", new)):
            t0, c0 = time.perf_counter(), time.process_time()
            fn()
            wall[name].append(time.perf_counter() - t0)
            cpu[name].append(time.process_time() - c0)
    samples = len(blobs) * T
    rec = {"files": len(blobs), "frames": T, "in_rate": in_rate, "out_rate": out_rate, "max_abs_difference": worst}
    for name in ("old", "new"):
        rec[name + "_seconds"] = median(wall[name])
        rec[name + "_cpu_seconds"] = median(cpu[name])
        rec[name + "_tensor_samples_per_s"] = samples / median(wall[name])
    rec["speedup"] = rec["old_seconds"] / rec["new_seconds"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--call-files", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    res = {"what": "tools/bench_resample.py", "passes": PASSES,
           "note": "kernel leg: timed through the public afg_resample_hip, which fetches the rows and waits for its stream before every "
                   "launch (the batch path checks its host copy and does not): resample_over_probe is an upper bound"}
    distinct = {}
    if not args.skip_call:                                         # (worker processes: before anything touches the GPU)
        from e2e_files import generate_files
        distinct = generate_files({"mp3": 150}, args.distinct)
    import afgpu
    res["device"] = afgpu.device_name(0)
    res["host_cpus"] = os.cpu_count()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():                                                    # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if not args.skip_kernel:
        res["kernel"] = kernel_leg(args.rows)
        save()
    if not args.skip_call:
        blobs = [bytes(bytearray(distinct["mp3"][i % len(distinct["mp3"])])) for i in range(args.call_files)]
        res["call"] = [call_leg(blobs, 160000, 16000, 44100, args.threads)]
        save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
