#!/usr/bin/env python3
"""tools/bench_yin.py -- what the YIN pitch stage costs, written to profiles/yin_bench.json.

Rows of 480 000 device-resident samples (30 s at 16 kHz), fmin 50 / fmax 500 (lags 32 .. 320), the shapes
(frame_length, win_length, hop) = (1024, 512, 160) and (2048, 1024, 512): afg_yin_hip beside a torch expression of librosa's
route on the same tensor (unfold, rfft / irfft autocorrelation, cumsum energies, cumulative mean, troughs under the
threshold, argmax, gather, parabolic shift; float32, on a slice of the rows and scaled) and afg_copy_probe_hip over the
bytes the stage must move (input once, output once), all alternating in one process, medians of 5.  The share of the
float32 vector rate counts the definition's 2 * W * tau_max operations per frame (one subtract and one fmaf per term) against
78.6e12 lane-instructions a second: 256 compute units * 128 lanes * 2.4 GHz, half the 157.3 TFLOPS the data sheet counts
with an fma as two.  No time is promised and nothing gates on one.

    python tools/bench_yin.py [--rows 1024] [--out profiles/yin_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
SAMPLES, RATE, FMIN, FMAX, THRESHOLD = 480000, 16000, 50.0, 500.0, 0.1
SHAPES = [(1024, 512, 160), (2048, 1024, 512)]
TORCH_ROWS = 16                                                  # the torch expression holds [rows, frames, frame_length] planes: a slice, scaled
LANE_RATE = 256 * 128 * 2.4e9


def median(v):
    return sorted(v)[len(v) // 2]


def torch_yin(x, N, W, hop, tau_min, tau_max):
    """librosa.yin's route in torch ops, float32, centred with zeros: [rows, samples] -> f0 [rows, frames]"""
    import torch
    fr = torch.nn.functional.pad(x, (N // 2, N // 2)).unfold(1, N, hop)
    a = torch.fft.rfft(fr, n=N)
    b = torch.fft.rfft(fr[..., 1:W + 1].flip(-1), n=N)
    acf = torch.fft.irfft(a * b, n=N)[..., W:]
    e = torch.cumsum(fr * fr, dim=-1)
    energy = e[..., W:] - e[..., :-W]
    d = (energy[..., :1] + energy - 2.0 * acf)[..., :tau_max + 2]
    tau = torch.arange(1, tau_max + 2, device=x.device, dtype=torch.float32)
    dp = d[..., 1:] * tau / torch.clamp(torch.cumsum(d[..., 1:], dim=-1), min=torch.finfo(torch.float32).tiny)
    v = dp[..., tau_min - 1:tau_max]                             # lags tau_min .. tau_max
    left = torch.cat((torch.ones_like(v[..., :1], dtype=torch.bool), v[..., 1:] < v[..., :-1]), dim=-1)
    right = torch.cat((v[..., :-1] <= v[..., 1:], torch.zeros_like(v[..., :1], dtype=torch.bool)), dim=-1)
    hit = left & right & (v < THRESHOLD)
    first = torch.argmax(hit.to(torch.uint8), dim=-1)
    best = torch.where(hit.any(dim=-1), first, torch.argmin(v, dim=-1))
    idx = (best + tau_min - 1).clamp(1, dp.shape[-1] - 2)
    pa, pb, pc = (torch.gather(dp, -1, (idx + k).unsqueeze(-1)).squeeze(-1) for k in (-1, 0, 1))
    A, B = pc + pa - 2.0 * pb, (pc - pa) * 0.5
    shift = torch.where(B.abs() < A.abs(), -B / A, torch.zeros_like(A))
    return RATE / ((idx + 1).to(torch.float32) + shift)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_bench.json"))
    args = ap.parse_args()
    import torch
    import afgpu
    n_rows = args.rows
    res = {"what": "tools/bench_yin.py", "passes": PASSES, "device": afgpu.device_name(0), "rows": n_rows, "samples": SAMPLES,
           "note": "timed through the public afg_yin_hip, which fetches the rows and waits for its stream before every launch.  torch: librosa's "
                   f"route in float32 tensor ops on {TORCH_ROWS} rows, scaled to the row count.  share_of_vector_rate: 2 * W * tau_max operations "
                   f"per frame over the time, against {LANE_RATE:.4g} lane-instructions a second (256 CUs * 128 lanes * 2.4 GHz)", "cases": []}
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

    t = torch.arange(SAMPLES, dtype=torch.float32, device="cuda") / RATE
    f_row = torch.linspace(70.0, 400.0, n_rows, device="cuda")[:, None]
    x = 0.3 * torch.sin(2.0 * np.pi * f_row * t[None, :]) + 0.15 * torch.sin(4.0 * np.pi * f_row * t[None, :])
    x += 0.01 * torch.empty_like(x).normal_()
    for N, W, hop in SHAPES:
        tau_min, tau_max = afgpu.yin_lags(RATE, FMIN, FMAX, N, W)
        prm = afgpu.yin_params(RATE, N, W, hop, tau_min, tau_max, THRESHOLD)
        frames = afgpu.yin_frames(prm, SAMPLES)
        rec = np.zeros(n_rows, afgpu.MEL_ROW_DTYPE)
        rec["in_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
        rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(2 * frames)
        rec["in_frames"], rec["out_frames"] = SAMPLES, frames
        tiles = afgpu.yin_layout(rec, prm)
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        d_out = torch.empty((n_rows, 2, frames), dtype=torch.float32, device="cuda")
        part = min(TORCH_ROWS, n_rows)

        def run_yin():
            afgpu.yin(n_rows, d_rec, tiles, prm, x, x.numel(), d_out, d_out.numel())

        def run_torch():
            return torch_yin(x[:part], N, W, hop, tau_min, tau_max)

        run_yin()
        ours, theirs = d_out[:part, 0, 4:-4], run_torch()[:, 4:-4]
        close = float(((ours - theirs).abs() < 0.5).float().mean().item())      # frames within half a hertz of the torch route
        hertz = float((d_out[:, 0, 4:-4] - f_row).abs().median().item())
        moved = int(x.numel() * 4 + d_out.numel() * 4)
        probe_bytes = moved // 2 // 16 * 16                      # the probe reads and writes what it is given
        src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
        ty, tt, tc = [], [], []
        for _ in range(PASSES):                                  # alternating, so that clocks and neighbours hit all alike
            ty.append(timed(run_yin))
            tt.append(timed(run_torch) * n_rows / part)
            tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
        sy, st, sc = median(ty), median(tt), median(tc)
        ops = 2.0 * W * tau_max * frames * n_rows
        res["cases"].append({"frame_length": N, "win_length": W, "hop": hop, "tau_min": tau_min, "tau_max": tau_max, "frames": frames, "tiles": tiles,
                             "bytes_moved": moved, "yin_seconds": sy, "torch_seconds": st, "copy_probe_seconds": sc, "torch_over_yin": st / sy,
                             "of_the_probe": sc / sy, "vector_operations": ops, "share_of_vector_rate": ops / sy / LANE_RATE,
                             "frames_within_half_a_hertz_of_torch": close, "median_abs_error_hertz": hertz})
        print(json.dumps(res["cases"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:                          # after every case: a later one that fails loses nothing
            json.dump(res, fh, indent=1)
        del d_out, src, dst
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
