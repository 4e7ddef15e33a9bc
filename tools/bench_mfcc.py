#!/usr/bin/env python3
"""tools/bench_mfcc.py -- what the cepstral stage costs, written to profiles/mfcc_bench.json.

(a) kernel leg: 1024 device-resident log-mel slabs of [80, 3000] and of [128, 3000] floats to 13 / 40 coefficients with
    delta_order 0 and 2 (N = 2): afg_cepstra_hip beside afg_copy_probe_hip over the bytes the kernel must move (the slab read
    once, every output plane written once) and beside the torch expression a caller runs today on the same tensor: matmul,
    replicate pad, two grouped conv1d, cat.
(b) call leg: 128 generated MP3 files (44.1 kHz stereo, 30 s) to [files, 1, 39, 3000] through afgpu.batch_decode_mfcc, against
    afgpu.batch_decode_mel followed by the same torch expression; wall clock around a device synchronise.
The sides alternate in one process; medians of 5.  No ratio is promised and nothing gates on one.

    python tools/bench_mfcc.py [--slabs 1024] [--call-files 128] [--distinct 32] [--out profiles/mfcc_bench.json]
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
FRAMES = 3000
SAMPLES, RATE = 480000, 16000
WIN = 2
SHAPES = [(n_mels, n_ceps, order) for n_mels in (80, 128) for n_ceps in (13, 40) for order in (0, 2)]


def median(v):
    return sorted(v)[len(v) // 2]


def torch_cepstra(x, d_dct, order, N):
    """[slabs, n_mels, F] -> [slabs, (1 + order) * n_ceps, F]: what a caller of torchaudio's MFCC and ComputeDeltas runs"""
    import torch
    import torch.nn.functional as Fn
    planes = [torch.matmul(d_dct, x)]
    if order:
        n_ceps = d_dct.shape[0]
        w = torch.arange(-N, N + 1, dtype=torch.float32, device=x.device) / (2.0 * sum(n * n for n in range(1, N + 1)))
        w = w.repeat(n_ceps, 1, 1)
        for _ in range(order):
            planes.append(Fn.conv1d(Fn.pad(planes[-1], (N, N), mode="replicate"), w, groups=n_ceps))
    return torch.cat(planes, 1) if order else planes[0]


def kernel_leg(n_slabs):
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

    out = []
    for n_mels, n_ceps, order in SHAPES:
        x = torch.empty((n_slabs, n_mels, FRAMES), dtype=torch.float32, device="cuda").uniform_(-10.0, 2.0)
        out_rows = (1 + order) * n_ceps
        y = torch.empty((n_slabs, out_rows, FRAMES), dtype=torch.float32, device="cuda")
        prm = afgpu.cep_params(n_mels, n_ceps, order, WIN)
        dct = afgpu.cep_dct(n_ceps, n_mels, "ortho")
        d_dct = torch.from_numpy(dct.copy()).cuda()
        rows = np.zeros(n_slabs, afgpu.CEP_ROW_DTYPE)
        rows["in_off"] = np.arange(n_slabs, dtype=np.uint64) * np.uint64(n_mels * FRAMES)
        rows["out_off"] = np.arange(n_slabs, dtype=np.uint64) * np.uint64(out_rows * FRAMES)
        rows["frames"] = FRAMES
        tiles = afgpu.cep_layout(rows, prm)
        d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
        moved = (x.numel() + y.numel()) * 4                       # the slab read once, every plane written once
        half = moved // 2 // 16 * 16                              # the copy reads and writes this much: `moved` in all
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")

        def run_kernel():
            afgpu.cepstra(n_slabs, d_rows, tiles, prm, x, x.numel(), d_dct, d_dct.numel(), y, y.numel())

        def run_copy():
            afgpu.copy_probe(dst, src, half)

        def run_torch():
            return torch_cepstra(x, d_dct, order, WIN)

        run_kernel()
        worst = float((run_torch() - y).abs().max().item())
        tk, tc, tt = [], [], []
        for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit all alike
            tk.append(timed(run_kernel))
            tc.append(timed(run_copy))
            tt.append(timed(run_torch))
        sk, sc, st = median(tk), median(tc), median(tt)
        flops = 2.0 * n_slabs * FRAMES * (n_ceps * n_mels + order * n_ceps * (3 * WIN + 1))
        out.append({"slabs": n_slabs, "n_mels": n_mels, "frames": FRAMES, "n_ceps": n_ceps, "delta_order": order, "delta_win": WIN,
                    "tiles": tiles, "bytes_moved": moved, "flops": flops, "max_abs_difference_from_torch": worst,
                    "cepstra_seconds": sk, "copy_probe_seconds": sc, "torch_seconds": st, "cepstra_over_copy": sk / sc,
                    "torch_over_cepstra": st / sk, "cepstra_GBps_moved": moved / sk / 1e9, "copy_GBps_moved": 2 * half / sc / 1e9,
                    "cepstra_GFLOPs": flops / sk / 1e9})
        print(json.dumps(out[-1]), flush=True)
        del x, y, src, dst
        torch.cuda.empty_cache()
    return out


def call_leg(blobs, threads):
    import torch
    import afgpu
    d_dct = torch.from_numpy(afgpu.cep_dct(13, 80, "ortho").copy()).cuda()
    out = torch.empty((len(blobs), 1, 39, FRAMES), dtype=torch.float32, device="cuda")
    mel = torch.empty((len(blobs), 1, 80, FRAMES), dtype=torch.float32, device="cuda")

    def old():
        t, _ = afgpu.batch_decode_mel(blobs, SAMPLES, RATE, n_out=FRAMES, out=mel, n_threads=threads)
        y = torch_cepstra(t[:, 0], d_dct, 2, WIN)
        torch.cuda.synchronize()
        return y

    def new():
        t, _ = afgpu.batch_decode_mfcc(blobs, SAMPLES, 13, 2, WIN, samplerate=RATE, n_out=FRAMES, out=out, n_threads=threads)
        torch.cuda.synchronize()
        return t[:, 0]

    worst = float((old() - new()).abs().max().item())            # warm-up; the two agree to float32 rounding, not bit for bit
    wall = {"old": [], "new": []}
    for _ in range(PASSES):
        for name, fn in (("old", old), ("new", new)):
            t0 = time.perf_counter()
            fn()
            wall[name].append(time.perf_counter() - t0)
    rec = {"files": len(blobs), "samples": SAMPLES, "frames": FRAMES, "n_mfcc": 13, "delta_order": 2, "max_abs_difference": worst,
           "old_seconds": median(wall["old"]), "new_seconds": median(wall["new"])}
    rec["speedup"] = rec["old_seconds"] / rec["new_seconds"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", type=int, default=1024)
    ap.add_argument("--call-files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfcc_bench.json"))
    args = ap.parse_args()
    res = {"what": "tools/bench_mfcc.py", "passes": PASSES,
           "note": "kernel leg: timed through the public afg_cepstra_hip, which fetches the records and waits for its stream before every "
                   "launch (the batch path checks its host copy and does not).  old: batch_decode_mel + torch; new: batch_decode_mfcc"}
    distinct = {}
    if not args.skip_call:                                         # (worker processes: before anything touches the GPU)
        from e2e_files import generate_files
        distinct = generate_files({"mp3": 30}, args.distinct)
    import afgpu
    res["device"] = afgpu.device_name(0)
    res["host_cpus"] = os.cpu_count()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():                                                    # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if not args.skip_kernel:
        res["kernel"] = kernel_leg(args.slabs)
        save()
    if not args.skip_call:
        blobs = [bytes(bytearray(distinct["mp3"][i % len(distinct["mp3"])])) for i in range(args.call_files)]
        res["call"] = [call_leg(blobs, args.threads)]
        save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
