#!/usr/bin/env python3
"""tools/bench_collate.py -- what the collate path costs, written to profiles/collate_bench.json.

(a) kernel leg: 512 files x 60 s (16 kHz) device-resident, 1 / 2 / 6 channels, every file at an odd in_off and a first_frame
    that is no multiple of anything, into T = 10 s (a crop) and T = 90 s (copy + padding as zero runs): afg_collate_hip
    beside afg_copy_probe_hip over the same number of bytes read and written, alternating in one process, medians of 5.
(b) call leg: 1024 generated FLAC files and 1024 generated MP3 files through afgpu.batch_decode_tensor against what a caller
    had before it: afgpu.batch_decode, numpy pad / transpose / stack, torch.from_numpy(...).cuda().  The two alternate in
    one process; medians of 5, with the CPU seconds (every thread of the process) per call.

    python tools/bench_collate.py [--files 512] [--call-files 1024] [--distinct 32] [--out profiles/collate_bench.json]
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
RATE = 16000


def median(v):
    return sorted(v)[len(v) // 2]


def kernel_leg(files):
    import torch
    import afgpu
    out = []
    seconds, first_frame = 60, 1237
    for ch in (1, 2, 6):
        n = seconds * RATE * ch                                   # samples per file
        stride = n + 1 + (n & 1)                                  # every file starts at an odd float
        d_in = torch.empty(files * stride + 8, dtype=torch.float32, device="cuda").normal_()
        for T_s in (10, 90):
            T = T_s * RATE
            spans = []
            for i in range(files):
                lo, hi = first_frame * ch, min(n, (first_frame + T) * ch)          # the crop, as the batch path cuts it on the host
                spans.append(dict(in_off=1 + i * stride + lo, count=hi - lo, sample0=lo, out_off=i * ch * T, first_frame=first_frame,
                                  frames=T, channels=ch, out_channels=ch))
                filled = (hi - lo) // ch
                for k in range(ch):
                    if filled < T:
                        spans.append(dict(out_off=i * ch * T + k * T + filled, count=T - filled))
            rec = np.zeros(len(spans), afgpu.COLLATE_SPAN_DTYPE)
            for k, sp in enumerate(spans):
                for name, v in sp.items():
                    rec[k][name] = v
            tiles = afgpu.collate_layout(rec)
            d_spans = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            d_out = torch.empty(files * ch * T, dtype=torch.float32, device="cuda")
            read = int(rec["count"][rec["channels"] != 0].sum()) * 4
            written = files * ch * T * 4
            half = (read + written) // 2 // 16 * 16               # the probe reads and writes `half` bytes each
            p_src = torch.empty(half // 4, dtype=torch.float32, device="cuda").normal_()
            p_dst = torch.empty(half // 4, dtype=torch.float32, device="cuda")
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

            def run_collate():
                afgpu.collate(len(rec), d_spans, tiles, d_in, d_in.numel(), d_out, d_out.numel())

            def run_probe():
                afgpu.copy_probe(p_dst, p_src, half)

            tc, tp = [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit both alike
                tc.append(timed(run_collate))
                tp.append(timed(run_probe))
            sc, sp_ = median(tc), median(tp)
            out.append({"channels": ch, "T_seconds": T_s, "files": files, "bytes_read": read, "bytes_written": written,
                        "collate_seconds": sc, "collate_GBps": (read + written) / sc / 1e9, "copy_probe_seconds": sp_,
                        "copy_probe_GBps": 2 * half / sp_ / 1e9, "collate_over_probe": sc / sp_,
                        "samples_per_s": read / 4 / sc, "spans": len(rec), "tiles": tiles})
            print(json.dumps(out[-1]), flush=True)
            del d_out, p_src, p_dst
        del d_in
        torch.cuda.empty_cache()
    return out


def call_leg(kind, blobs, C, T, threads):
    import torch
    import afgpu

    def old():
        items = afgpu.batch_decode(blobs, threads)
        host = np.zeros((len(items), C, T), np.float32)
        for i, it in enumerate(items):
            if it["pcm"] is None:
                continue
            x = it["pcm"][:T, :C]
            host[i, :x.shape[1], :x.shape[0]] = x.T
        t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        return t

    out = torch.empty((len(blobs), C, T), dtype=torch.float32, device="cuda")

    def new():
        t, _ = afgpu.batch_decode_tensor(blobs, T, C, out=out, n_threads=threads)
        torch.cuda.synchronize()
        return t

    a, b = old(), new()                                            # warm-up, and the two agree
    same = bool((a.view(torch.int32) == b.view(torch.int32)).all().item())
    wall = {"old": [], "new": []}
    cpu = {"old": [], "new": []}
    for _ in range(PASSES):
        for name, fn in (("old", old), ("new", new)):
            t0, c0 = time.perf_counter(), time.process_time()
            fn()
            wall[name].append(time.perf_counter() - t0)
            cpu[name].append(time.process_time() - c0)
    samples = len(blobs) * C * T
    rec = {"kind": kind, "files": len(blobs), "channels": C, "frames": T, "bit_identical": same}
    for name in ("old", "new"):
        rec[name + "_seconds"] = median(wall[name])
        rec[name + "_cpu_seconds"] = median(cpu[name])
        rec[name + "_tensor_samples_per_s"] = samples / median(wall[name])
    rec["speedup"] = rec["old_seconds"] / rec["new_seconds"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--call-files", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_bench.json"))
    args = ap.parse_args()
    res = {"what": "tools/bench_collate.py", "passes": PASSES,
           "note": "kernel leg: timed through the public afg_collate_hip, which fetches the spans and waits for its stream before every "
                   "launch (the batch path checks its host copy and does not): each rep carries one host round trip the copy probe "
                   "beside it does not have, so collate_over_probe is an upper bound, loosest for the short T = 10 s launches"}
    distinct = {}
    if not args.skip_call:                                         # (worker processes: before anything touches the GPU)
        from e2e_files import generate_files
        distinct = generate_files({"flac": 40, "mp3": 150}, args.distinct)
    import torch
    import afgpu
    res["device"] = afgpu.device_name(0)
    res["host_cpus"] = os.cpu_count()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():                                                    # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if not args.skip_kernel:
        res["kernel"] = kernel_leg(args.files)
        save()
    if not args.skip_call:
        res["call"] = []
        for kind in ("flac", "mp3"):
            blobs = [bytes(bytearray(distinct[kind][i % len(distinct[kind])])) for i in range(args.call_files)]
            res["call"].append(call_leg(kind, blobs, 2, 131072, args.threads))
            save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
