#!/usr/bin/env python3
"""Development bench for the decode stages' packer (afg_pcm_pack_hip) and for afg_batch_transcode, shaped like
tools/bench_f64.py.

Kernel leg: a device-resident batch of 60-second stereo files at 44.1 kHz, one span per file, every span starting one float
and one byte off alignment (what a decode plane gives the kernel), s8 / s16 / s24 with dither off and on, timed with events
on the launch stream.  The yardstick is afg_copy_probe_hip over the same number of bytes (read + written), timed in the
same process; the figure to look at is the ratio of the two.

Transcode leg: the generated FLAC and MP3 corpora of tools/bench_codecs.py, file bytes in host memory to s16 WAV files in
host memory: one afg_batch_transcode call against the two calls that did this before it existed -- afg_batch_decode_ex to
float, then afg_batch_encode -- on the same files in the same process, alternating.  Wall seconds, samples/s and CPU seconds
per call of both.  Nothing here is compared with a CPU.  Writes profiles/transcode_bench.json and prints it."""
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
FORMAT_NAMES = ["s8", "s16", "s24"]
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
    dev = torch.device("cuda:0")
    width = afgpu.WAV_FORMAT_BYTES[fmt]
    in_stride, out_stride = FILE_SAMPLES + 3, FILE_SAMPLES * width + 1       # the next file starts off alignment again
    in_floats, out_bytes = 1 + in_stride * n_files, 1 + out_stride * n_files
    samples = FILE_SAMPLES * n_files
    moved = samples * 4 + samples * width
    one = np.clip(rng.standard_normal(in_stride) * 0.25, -1, 1).astype(np.float32)
    d_in = torch.cat([torch.zeros(1, device=dev), torch.from_numpy(one).to(dev).repeat(n_files)])
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    spans = np.zeros(n_files, afgpu.PCM_PACK_SPAN_DTYPE)
    spans["in_off"] = 1 + np.arange(n_files, dtype=np.uint64) * np.uint64(in_stride)
    spans["out_off"] = 1 + np.arange(n_files, dtype=np.uint64) * np.uint64(out_stride)
    spans["count"], spans["format"], spans["dither"], spans["seed"] = FILE_SAMPLES, fmt, dither, 12345
    tiles = afgpu.pcm_pack_layout(spans)
    d_spans = torch.from_numpy(spans.view(np.uint8).copy()).to(dev)
    ms, all_ms = timed(lambda: afgpu.pcm_pack(n_files, d_spans, tiles, d_in, in_floats, d_out, out_bytes), reps)
    del d_in, d_out
    torch.cuda.empty_cache()
    half = moved // 2 // 16 * 16                                  # the probe reads `half` bytes and writes as many
    a = torch.empty(half, dtype=torch.uint8, device=dev)
    b = torch.zeros(half, dtype=torch.uint8, device=dev)
    copy_ms, copy_all = timed(lambda: afgpu.copy_probe(a, b, half), reps)
    del a, b
    torch.cuda.empty_cache()
    rate, copy_rate = moved / (ms / 1e3), 2 * half / (copy_ms / 1e3)
    return {"format": FORMAT_NAMES[fmt], "dither": bool(dither), "files": n_files, "samples": int(samples), "bytes_read": int(samples * 4),
            "bytes_written": int(samples * width), "ms": round(ms, 3), "ms_all": all_ms, "bytes_per_s": rate,
            "samples_per_s": samples / (ms / 1e3), "copy_probe_ms": round(copy_ms, 3), "copy_probe_ms_all": copy_all,
            "copy_probe_bytes_per_s": copy_rate, "ratio_to_copy_probe": round(rate / copy_rate, 4),
            "fraction_of_8TBs": round(rate / HBM_PEAK_BS, 4)}


def measured(fn):
    r0 = resource.getrusage(resource.RUSAGE_SELF)
    t0 = time.perf_counter()
    res = fn()
    t1 = time.perf_counter()
    r1 = resource.getrusage(resource.RUSAGE_SELF)
    return res, t1 - t0, (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime)


def transcode_leg(name, files, reps):
    """s16 without dither: one afg_batch_transcode call, and afg_batch_decode_ex + afg_batch_encode, alternating"""
    opts = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF)
    job = afgpu.BatchDecoded(files)

    def two_calls():
        job.run()
        try:
            return afgpu.batch_encode([(it["pcm"], it["samplerate"]) for it in job.items], afgpu.FORMAT_WAV, opts)
        finally:
            job.close()

    def one_call():
        return afgpu.batch_transcode(files, opts)

    a, b = two_calls(), one_call()                                # warm-up (pools), and: the two ways agree
    assert all(x["status"] == 0 for x in a) and [x["bytes"] for x in a] == [x["bytes"] for x in b]
    samples = sum((len(x["bytes"]) - 44) // 2 for x in b)
    del a, b
    rows = {"two_calls": ([], []), "transcode": ([], [])}
    for _ in range(reps):
        for label, fn in (("two_calls", two_calls), ("transcode", one_call)):
            _, wall, cpu = measured(fn)
            rows[label][0].append(wall)
            rows[label][1].append(cpu)
    out = {"batch": name, "files": len(files), "samples": int(samples)}
    for label, (walls, cpus) in rows.items():
        w = float(np.median(walls))
        out[label] = {"s": round(w, 4), "s_all": [round(x, 4) for x in walls], "samples_per_s": samples / w,
                      "cpu_s_per_call": round(float(np.median(cpus)), 3)}
    out["transcode_to_two_calls_samples_per_s"] = round(out["transcode"]["samples_per_s"] / out["two_calls"]["samples_per_s"], 4)
    return out


def transcode_legs(n_files, reps):
    from e2e_files import generate_files
    gen = generate_files({"flac": 8, "mp3": 8}, 16)
    return [transcode_leg(f"{kind} corpus of tools/bench_codecs.py -> s16 WAV", [bytes(bytearray(gen[kind][i % len(gen[kind])])) for i in range(n_files)], reps)
            for kind in ("flac", "mp3")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-files", type=int, default=1024, help="0: no transcode leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcode_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    out = {"bench": "transcode", "device": afgpu.device_name(0), "runs_per_figure": args.reps, "file": "60 s stereo at 44.1 kHz",
           "spans": "one per file, in_off % 4 == 1, out_off % 16 varies", "pack": []}
    for fmt in range(3):
        for dither in (0, 1):
            out["pack"].append(time_format(fmt, dither, args.files, args.reps, rng))
    out["batch"] = transcode_legs(args.batch_files, max(3, args.reps)) if args.batch_files else None
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
