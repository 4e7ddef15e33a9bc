#!/usr/bin/env python3
"""Development bench for the conversion to float64 (afg_pcm_to_f64_hip), shaped like tools/bench_wav.py: a device-resident
batch of 1024 60-second stereo files at 44.1 kHz of each of the seven sample kinds, timed with events on the launch stream.
The yardstick is afg_copy_probe_hip over the same number of bytes (read + written), timed in the same process, and the
figure to look at is the ratio of the two.  Then the batch leg: 2048 s16 WAV files of 5 s, and the 2048-file FLAC batch of
tools/bench_codecs.py, file bytes in host memory to samples in host memory through afg_batch_decode_ex, each at
AFG_SAMPLE_F32 and AFG_SAMPLE_F64 in the same session: samples/s and CPU seconds per call.  The float leg is the baseline
of the double one.  Nothing here is compared with a CPU.  Writes profiles/f64_bench.json and prints it."""
import argparse
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import afgpu  # noqa: E402

HBM_PEAK_BS = 8.0e12
KIND_NAMES = ["u8", "s16", "s24", "s32", "f32", "f64", "flac_s32"]
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


def time_kind(kind, n_files, reps, rng):
    """n_files spans of FILE_SAMPLES samples, each at a 16-byte aligned input offset, back to back in the output."""
    dev = torch.device("cuda:0")
    width = afgpu.F64_KIND_BYTES[kind]
    file_bytes = (FILE_SAMPLES * width + 15) // 16 * 16
    in_bytes, out_doubles = file_bytes * n_files, FILE_SAMPLES * n_files
    moved = in_bytes + out_doubles * 8
    free, _ = torch.cuda.mem_get_info()                           # (the conversion's planes, then the probe's: never both)
    if moved > 0.9 * free:
        return {"kind": KIND_NAMES[kind], "files": n_files, "skipped": f"needs {moved >> 30} GiB of device memory, {free >> 30} free"}
    if kind in (afgpu.WAV_KIND_F32, afgpu.WAV_KIND_F64):          # programme material, not random bit patterns
        one = (rng.standard_normal(FILE_SAMPLES) * 0.25).astype("<f4" if kind == afgpu.WAV_KIND_F32 else "<f8").view(np.uint8)
    else:
        one = rng.integers(0, 256, FILE_SAMPLES * width, dtype=np.uint8)
    one = np.concatenate([one, np.zeros(file_bytes - one.size, np.uint8)])
    d_in = torch.from_numpy(one).to(dev).repeat(n_files)
    d_out = torch.empty(out_doubles, dtype=torch.float64, device=dev)
    spans = np.zeros(n_files, afgpu.WAV_SPAN_DTYPE)
    spans["in_off"] = np.arange(n_files, dtype=np.uint64) * np.uint64(file_bytes)
    spans["out_off"] = np.arange(n_files, dtype=np.uint64) * np.uint64(FILE_SAMPLES)
    spans["count"], spans["kind"] = FILE_SAMPLES, kind
    tiles = afgpu.wav_layout(spans)
    d_spans = torch.from_numpy(spans.view(np.uint8).copy()).to(dev)
    ms, all_ms = timed(lambda: afgpu.pcm_to_f64(n_files, d_spans, tiles, d_in, in_bytes, d_out, out_doubles), reps)
    del d_in, d_out
    torch.cuda.empty_cache()
    half = moved // 2 // 16 * 16                                  # the probe reads `half` bytes and writes as many
    a = torch.empty(half, dtype=torch.uint8, device=dev)
    b = torch.zeros(half, dtype=torch.uint8, device=dev)
    copy_ms, copy_all = timed(lambda: afgpu.copy_probe(a, b, half), reps)
    del a, b
    torch.cuda.empty_cache()
    rate, copy_rate = moved / (ms / 1e3), 2 * half / (copy_ms / 1e3)
    return {"kind": KIND_NAMES[kind], "files": n_files, "samples": int(out_doubles), "bytes_read": int(in_bytes), "bytes_written": int(out_doubles * 8),
            "ms": round(ms, 3), "ms_all": all_ms, "bytes_per_s": rate, "samples_per_s": out_doubles / (ms / 1e3),
            "copy_probe_ms": round(copy_ms, 3), "copy_probe_ms_all": copy_all, "copy_probe_bytes_per_s": copy_rate,
            "ratio_to_copy_probe": round(rate / copy_rate, 4), "fraction_of_8TBs": round(rate / HBM_PEAK_BS, 4)}


def batch_leg(name, files, reps):
    """one afg_batch_decode_ex call over `files`, float32 then float64: median wall seconds, samples/s, CPU seconds per call"""
    out = {"batch": name, "files": len(files)}
    for label, dtype in (("f32", np.float32), ("f64", np.float64)):
        job = afgpu.BatchDecoded(files, dtype=dtype)
        job.run()                                                     # warm-up (pools)
        samples = sum(it["frames"] * it["channels"] for it in job.items)
        assert all(it["status"] == 0 for it in job.items)
        walls, cpus = [], []
        for _ in range(reps):
            r0 = resource.getrusage(resource.RUSAGE_SELF)
            t0 = time.perf_counter()
            job.run()
            t1 = time.perf_counter()
            r1 = resource.getrusage(resource.RUSAGE_SELF)
            walls.append(t1 - t0)
            cpus.append((r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime))
        job.close()
        w = float(np.median(walls))
        out[label] = {"samples": int(samples), "s": round(w, 4), "s_all": [round(x, 4) for x in walls], "samples_per_s": samples / w,
                      "cpu_s_per_call": round(float(np.median(cpus)), 3)}
    out["f64_to_f32_samples_per_s"] = round(out["f64"]["samples_per_s"] / out["f32"]["samples_per_s"], 4)
    return out


def batch_legs(n_files, reps, rng):
    import wav_bitstream as wb
    from e2e_files import generate_files
    samples = 5 * 44100 * 2
    distinct = [wb.wav_file(1, 2, 44100, wb.random_samples(rng, 1, samples)) for _ in range(8)]
    legs = [batch_leg("s16 WAV stereo, 5 s", [distinct[i % 8] for i in range(n_files)], reps)]
    flac = generate_files({"flac": 8}, 16)["flac"]
    legs.append(batch_leg("FLAC 16-bit stereo, frames of 4096 (tools/bench_codecs.py)", [bytes(bytearray(flac[i % len(flac)])) for i in range(n_files)], reps))
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-files", type=int, default=2048, help="0: no batch leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    out = {"bench": "f64", "device": afgpu.device_name(0), "runs_per_figure": args.reps, "file": "60 s stereo at 44.1 kHz", "convert": []}
    for kind in range(7):
        out["convert"].append(time_kind(kind, args.files, args.reps, rng))
    out["batch"] = batch_legs(args.batch_files, max(3, args.reps), rng) if args.batch_files else None
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
