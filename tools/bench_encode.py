#!/usr/bin/env python3
"""Development bench for the encode side, shaped like tools/bench_wav.py: afg_wav_pack_hip on device-resident batches of
60-second stereo files at 44.1 kHz -- 1024 and 4096 files, each sample format, with and without the dither -- timed with
events on the launch stream.  The yardstick is afg_copy_probe_hip over the same number of bytes (read + written), timed in
the same process.  Then the batch leg: float PCM in host memory to file bytes in host memory through afg_batch_encode,
2048 stereo files of 5 s per call (WAV s16 with the LCG31 dither, and QOA), next to a page-locked upload + download of the
same bytes (the bus alone).  Nothing here is compared with a CPU.
Writes profiles/encode_bench.json and prints it."""
import argparse
import ctypes as C
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "audio-formats_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import afgpu  # noqa: E402

HBM_PEAK_BS = 8.0e12
FORMAT_NAMES = ["s8", "s16", "s24", "fp32", "fp64"]
FILE_SAMPLES = 60 * 44100 * 2


def timed(fn, reps):
    s = torch.cuda.current_stream()
    fn()                                                          # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(x, 3) for x in ms]


def time_format(fmt, dither, n_files, reps, rng):
    """n_files spans of FILE_SAMPLES samples, back to back in the input, each at a 16-byte aligned output offset."""
    dev = torch.device("cuda:0")
    width = afgpu.WAV_FORMAT_BYTES[fmt]
    file_bytes = (FILE_SAMPLES * width + 15) // 16 * 16
    in_floats, out_bytes = FILE_SAMPLES * n_files, file_bytes * n_files
    moved = in_floats * 4 + out_bytes
    name = FORMAT_NAMES[fmt] + ("+lcg31" if dither else "")
    free, _ = torch.cuda.mem_get_info()                           # (the packer's planes, then the probe's: never both)
    if moved > 0.9 * free:
        return {"format": name, "files": n_files, "skipped": f"needs {moved >> 30} GiB of device memory, {free >> 30} free"}
    one = rng.uniform(-1, 1, FILE_SAMPLES).astype(np.float32)
    d_in = torch.from_numpy(one).to(dev).repeat(n_files)
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    spans = np.zeros(n_files, afgpu.WAV_PACK_SPAN_DTYPE)
    spans["in_off"] = np.arange(n_files, dtype=np.uint64) * np.uint64(FILE_SAMPLES)
    spans["out_off"] = np.arange(n_files, dtype=np.uint64) * np.uint64(file_bytes)
    spans["count"], spans["format"], spans["dither"] = FILE_SAMPLES, fmt, 1 if dither else 0
    spans["seed"] = np.arange(n_files, dtype=np.uint32) + 1
    tiles = afgpu.wav_pack_layout(spans)
    d_spans = torch.from_numpy(spans.view(np.uint8).copy()).to(dev)
    ms, all_ms = timed(lambda: afgpu.wav_pack(n_files, d_spans, tiles, d_in, in_floats, d_out, out_bytes), reps)
    del d_in, d_out
    torch.cuda.empty_cache()
    half = moved // 2 // 16 * 16                                  # the probe reads `half` bytes and writes as many
    a = torch.empty(half, dtype=torch.uint8, device=dev)
    b = torch.zeros(half, dtype=torch.uint8, device=dev)
    copy_ms, copy_all = timed(lambda: afgpu.copy_probe(a, b, half), reps)
    del a, b
    torch.cuda.empty_cache()
    rate, copy_rate = moved / (ms / 1e3), 2 * half / (copy_ms / 1e3)
    return {"format": name, "files": n_files, "samples": int(in_floats), "bytes_read": int(in_floats * 4), "bytes_written": int(out_bytes),
            "ms": round(ms, 3), "ms_all": all_ms, "bytes_per_s": rate, "samples_per_s": in_floats / (ms / 1e3),
            "copy_probe_ms": round(copy_ms, 3), "copy_probe_ms_all": copy_all, "copy_probe_bytes_per_s": copy_rate,
            "ratio_to_copy_probe": round(rate / copy_rate, 4), "fraction_of_8TBs": round(rate / HBM_PEAK_BS, 4)}


def batch_leg(what, n_files, seconds, reps, rng):
    """Float PCM in host memory to file bytes in host memory: stereo files of `seconds`, one afg_batch_encode call."""
    frames = seconds * 44100
    distinct = [(rng.uniform(-0.5, 0.5, (frames, 2))).astype(np.float32) for _ in range(8)]
    arr = (afgpu.EncodeInput * n_files)()
    for i in range(n_files):
        arr[i] = afgpu.EncodeInput(distinct[i % 8].ctypes.data, frames, 2, 44100.0)
    if what == "qoa":
        fmt, opts, size = afgpu.FORMAT_QOA, None, afgpu.qoa_encoded_size(frames, 2)
    else:
        fmt, opts, size = afgpu.FORMAT_WAV, afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LCG31, 1), 44 + frames * 4
    L = afgpu.lib()
    res = afgpu.EncodeResult()

    def call():
        afgpu.check(L.afg_batch_encode(arr, n_files, fmt, None if opts is None else C.byref(opts), 0, C.byref(res)))
        for i in (0, n_files // 2, n_files - 1):
            assert res.items[i].status == 0 and res.items[i].size == size, (res.items[i].status, res.items[i].size)
        L.afg_encode_free(C.byref(res))
    call()                                                        # warm-up (pools)
    walls, cpus = [], []
    for _ in range(reps):
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        walls.append(t1 - t0)
        cpus.append((r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime))
    up, down = frames * 2 * 4 * n_files, size * n_files
    # the bus alone: the same bytes up and down between page-locked memory and the device, one after the other
    h_up, h_down = torch.empty(up, dtype=torch.uint8).pin_memory(), torch.empty(down, dtype=torch.uint8).pin_memory()
    d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda:0"), torch.empty(down, dtype=torch.uint8, device="cuda:0")
    bus = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_up.copy_(h_up, non_blocking=True)
        h_down.copy_(d_down, non_blocking=True)
        torch.cuda.synchronize()
        bus.append(time.perf_counter() - t0)
    w, b = float(np.median(walls)), float(np.median(bus[1:]))
    return {"format": what, "files": n_files, "seconds_per_file": seconds, "bytes_up": int(up), "bytes_down": int(down), "s": round(w, 4),
            "s_all": [round(x, 4) for x in walls], "samples_per_s": frames * 2 * n_files / w, "bus_bytes_per_s": (up + down) / w,
            "cpu_s_per_call": round(float(np.median(cpus)), 3), "pinned_copy_of_the_same_bytes_s": round(b, 4),
            "ratio_to_pinned_copy": round(b / w, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-files", type=int, default=2048)
    ap.add_argument("--batch-seconds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    out = {"bench": "encode", "device": afgpu.device_name(0), "runs_per_figure": args.reps, "file": "60 s stereo at 44.1 kHz", "pack": []}
    for n in args.files:
        for fmt in range(5):
            for dither in ((False, True) if fmt <= afgpu.WAV_S24LE else (False,)):
                out["pack"].append(time_format(fmt, dither, n, args.reps, rng))
    out["batch"] = [batch_leg(w, args.batch_files, args.batch_seconds, max(2, args.reps // 2), rng) for w in ("wav_s16_lcg31", "qoa")] \
        if args.batch_files else None
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
