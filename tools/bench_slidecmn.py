#!/usr/bin/env python3
"""tools/bench_slidecmn.py -- what the sliding-window normalisation costs, written to profiles/slidecmn_bench.json.

(a) kernel leg: 1024 slabs of [3000, 80] floats frames-major and 1024 of [80, 3000] col-major (30 s of 10 ms frames), with
    300 frames centred and variance, and with 600 / 100 causal without, out of place and in place: afg_slide_cmn_hip beside
    afg_copy_probe_hip over the same bytes (one read and one write of the plane), beside a vectorised torch expression of the
    same result (window sums as differences of float64 cumulative sums) and, where torchaudio imports, beside
    torchaudio.functional.sliding_window_cmn on 16 slabs, scaled to the slab count.
(b) batch leg: afgpu.batch_decode_fbank_cmn on 128 generated WAV files against afgpu.batch_decode_fbank followed by
    afgpu.sliding_cmn_tensor.
The sides alternate in one process; medians of 5.  The stage reads the plane once, writes and reads its workspace copy once
and writes the result once; the copy probe reads and writes once.  No ratio is promised and nothing gates on one.

    python tools/bench_slidecmn.py [--slabs 1024] [--files 128] [--out profiles/slidecmn_bench.json]
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
FRAMES, COLS = 3000, 80
SETTINGS = {"300-centred-vars": dict(cmn_window=300, min_cmn_window=100, center=True, norm_vars=True),
            "600-100-causal": dict(cmn_window=600, min_cmn_window=100, center=False, norm_vars=False)}


def median(v):
    return sorted(v)[len(v) // 2]


def torch_expression(x, frames_axis, ws, we, norm_vars):
    """the same result from float64 cumulative sums (what a user without the stage would write); x [slabs, ., .]"""
    import torch
    d = x.double().movedim(frames_axis, 1)                       # [slabs, frames, cols]
    zero = torch.zeros_like(d[:, :1])
    c1 = torch.cat([zero, d.cumsum(1)], 1)
    n = (we - ws).double()[None, :, None]
    mean = (c1[:, we] - c1[:, ws]) / n
    y = d - mean
    if norm_vars:
        c2 = torch.cat([zero, (d * d).cumsum(1)], 1)
        var = ((c2[:, we] - c2[:, ws]) / n - mean * mean).clamp_min(1e-10)
        y = y * var.rsqrt()
    return y.float().movedim(1, frames_axis)


def kernel_leg(n_slabs):
    import torch
    import afgpu
    import slidecmn_model as model
    try:
        import torchaudio.functional as taf
    except ImportError:
        taf = None
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
    for layout, shape, axis in (("frames", (n_slabs, FRAMES, COLS), 1), ("cols", (n_slabs, COLS, FRAMES), 2)):
        x = torch.empty(shape, dtype=torch.float32, device="cuda").normal_() * 3.0 + 1.0
        y = torch.empty_like(x)
        z = x.clone()
        nbytes = x.numel() * 4
        for name, kw in SETTINGS.items():
            win = np.array([model.window(t, FRAMES, kw["cmn_window"], kw["min_cmn_window"], kw["center"]) for t in range(FRAMES)])
            ws, we = (torch.from_numpy(win[:, k].copy()).cuda() for k in (0, 1))

            def run_kernel():
                afgpu.sliding_cmn_tensor(x, layout=layout, out=y, **kw)

            def run_in_place():                                  # (the values drift from pass to pass; the work does not)
                afgpu.sliding_cmn_tensor(z, layout=layout, out=z, **kw)

            def run_copy():
                afgpu.copy_probe(y, x, nbytes)

            def run_torch():
                return torch_expression(x, axis, ws, we, kw["norm_vars"])

            run_kernel()
            worst = float((run_torch() - y).abs().max().item())
            tk, ti, tc, tt = [], [], [], []
            for _ in range(PASSES):                              # alternating, so that clocks and neighbours hit all alike
                tk.append(timed(run_kernel))
                ti.append(timed(run_in_place))
                tc.append(timed(run_copy))
                tt.append(timed(run_torch, 1))
            sk, si, sc, st = median(tk), median(ti), median(tc), median(tt)
            row = {"layout": layout, "setting": name, "slabs": n_slabs, "frames": FRAMES, "cols": COLS, "plane_bytes": nbytes,
                   "max_abs_difference_from_torch": worst, "slide_cmn_seconds": sk, "slide_cmn_in_place_seconds": si, "copy_probe_seconds": sc,
                   "torch_cumsum_seconds": st, "slide_cmn_over_copy": sk / sc, "in_place_over_copy": si / sc, "torch_over_slide_cmn": st / sk,
                   "slide_cmn_GBps_moved": 4 * nbytes / sk / 1e9, "copy_GBps_moved": 2 * nbytes / sc / 1e9, "torchaudio_seconds_scaled": None}
            if taf is not None:
                part = x[:16].movedim(axis, 1).contiguous()
                t0 = time.perf_counter()
                taf.sliding_window_cmn(part, kw["cmn_window"], kw["min_cmn_window"], kw["center"], kw["norm_vars"])
                torch.cuda.synchronize()
                row["torchaudio_seconds_scaled"] = (time.perf_counter() - t0) * n_slabs / 16
            out.append(row)
            print(json.dumps(row), flush=True)
        del x, y, z
        torch.cuda.empty_cache()
    return out


def batch_leg(n_files):
    import torch
    import afgpu
    import f64_model as f64m
    import wav_bitstream as wb
    rng = np.random.default_rng(1)
    T = 30 * 16000
    files = [wb.wav_file(f64m.KIND_S16, 1, 16000, wb.random_samples(rng, f64m.KIND_S16, T - 160 * (i % 50))) for i in range(n_files)]
    kw = dict(num_mel_bins=80, scale=32768.0)
    cmn = SETTINGS["300-centred-vars"]

    def one():
        afgpu.batch_decode_fbank_cmn(files, T, **cmn, **kw)
        torch.cuda.synchronize()

    def two():
        feats, _, lengths = afgpu.batch_decode_fbank(files, T, **kw)
        afgpu.sliding_cmn_tensor(feats, valid_frames=lengths, out=feats, **cmn)
        torch.cuda.synchronize()

    def wall(fn):
        fn()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    t1, t2 = [], []
    for _ in range(PASSES):
        t1.append(wall(one))
        t2.append(wall(two))
    row = {"files": n_files, "samples_per_file": T, "one_call_seconds": median(t1), "two_calls_seconds": median(t2),
           "one_over_two": median(t1) / median(t2)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", type=int, default=1024)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slidecmn_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_slidecmn.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through afgpu.sliding_cmn_tensor: the records' upload, the workspace allocation and the public entry's fetch "
                   "of the records are inside the stage's time"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():                                                  # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    res["kernel"] = kernel_leg(args.slabs)
    save()
    res["batch"] = batch_leg(args.files)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
