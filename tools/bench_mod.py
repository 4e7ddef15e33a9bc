#!/usr/bin/env python3
"""Development bench for the ProTracker MOD mixer (afg_mod_render_hip), following tools/bench_codecs.py: device-resident
batches of generated 60-second songs -- 1024 four-channel songs (2.65 G frames, 21 GB of PCM), and 8- and 32-channel songs
at the same output size -- timed with events on the launch stream; then MOD files end to end through afg_batch_decode.
Prints one JSON line."""
import argparse
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import afgpu  # noqa: E402
import mod_bitstream as mb  # noqa: E402

HBM_PEAK_BS = 8.0e12


def song_60s(rng, channels):
    """8 orders of 64 lines at speed 6, 125 BPM (7.68 s each): notes on every channel every 4 lines, loops and effects."""
    samples = [mb.random_sample(rng, 4000, (2000, 2000), int(rng.integers(0, 16)), 48) for _ in range(8)]
    pats = []
    for _ in range(8):
        p = mb.empty_pattern(channels)
        for r in range(0, 64, 4):
            for c in range(channels):
                eff = int(rng.choice([0x0, 0x4, 0xA, 0x8, 0x0]))
                par = int(rng.integers(0, 256)) if eff != 0xA else 0x01
                p[r][c] = mb.cell(int(rng.integers(1, 9)), int(rng.choice(mb.PERIODS[6:30])), eff, par)
        pats.append(p)
    return mb.build(pats, list(range(8)), samples, channels, 31)


def shape(channels, n_songs, distinct, rng):
    """Device arrays for n_songs songs: `distinct` generated songs, repeated."""
    parsed = [afgpu.mod_parse(song_60s(rng, channels)) for _ in range(distinct)]
    sng, ticks, segs, plane, frames = afgpu.mod_layout(parsed)
    segs = segs[:-1]                                           # (mod_layout's spare record)
    reps = n_songs // distinct
    dev = torch.device("cuda:0")
    d_ticks = torch.from_numpy(ticks.view(np.uint8).copy()).to(dev).repeat(reps)
    d_segs = torch.from_numpy(segs.view(np.uint8).copy()).to(dev).repeat(reps)
    d_plane = torch.from_numpy(plane.copy()).to(dev)
    all_songs = np.zeros(n_songs, afgpu.MOD_SONG_DTYPE)
    for r in range(reps):
        blk = sng.copy()
        blk["out_frame"] += r * frames
        blk["tick_base"] += r * len(ticks)
        blk["seg_base"] += r * len(segs)
        all_songs[r * distinct:(r + 1) * distinct] = blk
    d_songs = torch.from_numpy(all_songs.view(np.uint8).copy()).to(dev)
    total = frames * reps
    rec_bytes = d_ticks.numel() + d_segs.numel() + d_songs.numel()
    return d_songs, d_segs, d_ticks, d_plane, total, rec_bytes


def time_shape(channels, n_songs, distinct, reps, rng):
    d_songs, d_segs, d_ticks, d_plane, frames, rec_bytes = shape(channels, n_songs, distinct, rng)
    d_out = torch.empty(frames * 2, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream()
    afgpu.mod_render(n_songs, d_songs, d_segs, d_ticks, d_plane, d_out)       # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        afgpu.mod_render(n_songs, d_songs, d_segs, d_ticks, d_plane, d_out)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    moved = frames * 8 + rec_bytes
    rec = {"channels": channels, "songs": n_songs, "frames": int(frames), "out_bytes": int(frames * 8), "record_bytes": int(rec_bytes),
           "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms], "frames_per_s": frames / (med / 1e3),
           "bytes_moved_per_s": moved / (med / 1e3), "fraction_of_8TBs": moved / (med / 1e3) / HBM_PEAK_BS}
    del d_out
    torch.cuda.empty_cache()
    return rec


def end_to_end(n_files, reps, rng):
    files = [song_60s(rng, 4) for _ in range(n_files)]
    res = afgpu.BatchDecoded(files)
    res.run(); res.close()                                    # warm-up (pools)
    walls, cpus, frames = [], [], 0
    for _ in range(reps):
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        res.run()
        t1 = time.perf_counter()
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        frames = sum(it["frames"] for it in res.items)
        res.close()
        walls.append(t1 - t0)
        cpus.append((r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime))
    w = float(np.median(walls))
    return {"files": n_files, "frames": int(frames), "s": round(w, 4), "frames_per_s": frames / w,
            "cpu_s_per_call": round(float(np.median(cpus)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e-files", type=int, default=64)
    args = ap.parse_args()
    rng = np.random.default_rng(2024)
    out = {"bench": "mod", "device": afgpu.device_name(0), "shapes": []}
    # the same output size for every shape: 1024 four-channel 60-second songs
    for ch in (4, 8, 32):
        out["shapes"].append(time_shape(ch, args.songs, 16, args.reps, rng))
    out["end_to_end"] = end_to_end(args.e2e_files, max(2, args.reps // 2), rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
