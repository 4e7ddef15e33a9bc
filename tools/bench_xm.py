#!/usr/bin/env python3
"""Development bench for the FastTracker II XM mixer (afg_xm_render_hip), shaped like tools/bench_mod.py: device-resident
batches of generated 60-second songs -- 1024 songs at 4, 8 and 32 channels -- timed with events on the launch stream, then
XM files end to end through afg_batch_decode.  The yardstick is the MOD mixer at the same song count, channel count and
length, measured by tools/bench_mod.py's own functions in the same run.  Writes profiles/xm_bench.json and prints it."""
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
import bench_mod  # noqa: E402
import xm_bitstream as xb  # noqa: E402

HBM_PEAK_BS = 8.0e12


def song_60s(rng, channels):
    """8 orders of 64 rows at tempo 6, 125 BPM (7.68 s each): a note on every channel every 4 rows, 8- and 16-bit samples with
    forward and ping-pong loops, vibrato, volume slides and panning: the mix bench_mod.py's songs have, in XM's terms."""
    ins = []
    for k in range(8):
        n = 4000
        bits = 16 if k % 2 else 8
        data = (np.sin(np.arange(n) * rng.uniform(0.05, 0.5)) * (30000 if bits == 16 else 120)).astype(np.int64)
        ins.append(xb.instrument([xb.sample(data, bits, 1 + k % 2, 2000, 2000, 48, 0, int(rng.integers(0, 256)))]))
    pats = []
    for _ in range(8):
        rows = [{} for _ in range(64)]
        for r in range(0, 64, 4):
            for c in range(channels):
                eff = int(rng.choice([0x0, 0x4, 0xA, 0x8, 0x0]))
                par = int(rng.integers(0, 256)) if eff != 0xA else 0x01
                rows[r][c] = (int(rng.integers(37, 61)), int(rng.integers(1, 9)), 0, eff, par)
        pats.append(rows)
    return xb.build(channels, list(range(8)), pats, ins, linear=True, tempo=6, bpm=125)


def shape(channels, n_songs, distinct, rng):
    parsed = [afgpu.xm_parse(song_60s(rng, channels)) for _ in range(distinct)]
    sng, ticks, segs, data, aux, frames = afgpu.xm_layout(parsed)
    segs, aux = segs[:-1], aux[:-1]
    reps = n_songs // distinct
    dev = torch.device("cuda:0")
    d_ticks = torch.from_numpy(ticks.view(np.uint8).copy()).to(dev).repeat(reps)
    d_segs = torch.from_numpy(segs.view(np.uint8).copy()).to(dev).repeat(reps)
    d_aux = torch.from_numpy(np.concatenate([aux, np.zeros(1, np.float32)])).to(dev)
    d_data = torch.from_numpy(data.copy()).to(dev)
    all_songs = np.zeros(n_songs, afgpu.XM_SONG_DTYPE)
    for r in range(reps):
        blk = sng.copy()
        blk["out_frame"] += r * frames
        blk["tick_base"] += r * len(ticks)
        blk["seg_base"] += r * len(segs)
        all_songs[r * distinct:(r + 1) * distinct] = blk
    d_songs = torch.from_numpy(all_songs.view(np.uint8).copy()).to(dev)
    kinds = {"segments": int(len(segs)), "ramp": int((segs["flags"] & afgpu.XM_SEG_RAMP != 0).sum()),
             "fade": int((segs["flags"] & afgpu.XM_SEG_FADE != 0).sum()), "back": int((segs["flags"] & afgpu.XM_SEG_BACK != 0).sum()),
             "aux_floats": int(len(aux))}
    return d_songs, d_segs, d_ticks, d_data, d_aux, frames * reps, d_ticks.numel() + d_segs.numel() + d_songs.numel() + d_aux.numel() * 4, kinds


def time_shape(channels, n_songs, distinct, reps, rng):
    d_songs, d_segs, d_ticks, d_data, d_aux, frames, rec_bytes, kinds = shape(channels, n_songs, distinct, rng)
    d_out = torch.empty(frames * 2, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream()
    afgpu.xm_render(n_songs, d_songs, d_segs, d_ticks, d_data, d_aux, d_out)     # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        afgpu.xm_render(n_songs, d_songs, d_segs, d_ticks, d_data, d_aux, d_out)
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    rec = {"channels": channels, "songs": n_songs, "frames": int(frames), "out_bytes": int(frames * 8), "record_bytes": int(rec_bytes),
           "ms": round(med, 3), "ms_all": [round(x, 3) for x in ms], "frames_per_s": frames / (med / 1e3),
           "fraction_of_8TBs_on_stored_bytes": frames * 8 / (med / 1e3) / HBM_PEAK_BS, "kinds_of_16_distinct": kinds}
    del d_out
    torch.cuda.empty_cache()
    return rec


def end_to_end(n_files, reps, rng):
    """XM files through afg_batch_decode; every item must come back as a decoded XM (MP3 detection runs first and can claim
    an XM whose sample bytes pass for MPEG frames: such a figure would be of something else)."""
    files = []
    while len(files) < n_files:
        f = song_60s(rng, 4)
        try:
            afgpu.mp3_parse(f)                                # claimed by the MP3 front-end: not an XM to this library
        except afgpu.AfgError:
            files.append(f)
    res = afgpu.BatchDecoded(files)
    res.run(); res.close()                                    # warm-up (pools)
    walls, cpus, frames = [], [], 0
    for _ in range(reps):
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        res.run()
        t1 = time.perf_counter()
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        for it in res.items:
            assert it["status"] == 0 and it["format"] == afgpu.FORMAT_XM, (it["status"], it["format"], it["message"])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xm_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(2024)
    out = {"bench": "xm", "device": afgpu.device_name(0), "runs_per_figure": args.reps, "shapes": [], "mod_shapes": [], "xm_over_mod": {}}
    for ch in (4, 8, 32):
        x = time_shape(ch, args.songs, 16, args.reps, rng)
        m = bench_mod.time_shape(ch, args.songs, 16, args.reps, rng)
        out["shapes"].append(x)
        out["mod_shapes"].append(m)
        out["xm_over_mod"][str(ch)] = round(x["ms"] / m["ms"] * m["frames"] / x["frames"], 4)     # time per frame
    out["end_to_end"] = end_to_end(args.e2e_files, max(2, args.reps // 2), rng)
    out["mod_end_to_end"] = bench_mod.end_to_end(args.e2e_files, max(2, args.reps // 2), rng)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
