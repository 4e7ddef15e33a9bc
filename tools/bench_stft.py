#!/usr/bin/env python3
"""tools/bench_stft.py -- what the linear spectrogram stage costs, written to profiles/stft_bench.json.

(a) kernel leg: rows of 480 000 device-resident samples (30 s at 16 kHz) with Whisper's framing (n_fft 400, hop 160) and with
    n_fft 1024, hop 256, each of the four kinds: afg_stft_hip beside afg_melspec_fft_hip on the same input (80 and 128 mels),
    the torch.stft expression of the kind (+ abs, ** 2, log10) on the same tensor, and afg_copy_probe_hip over the bytes the
    stage must move (input once, output once), all alternating in one process, medians of 5.  The largest |ours - torch.stft|
    is given in units of the header's E_f (informational: rocFFT's own error is not ours to bound).
(b) call leg: generated MP3 files (44.1 kHz stereo) to [files, 1, 201, 3000] power through afgpu.batch_decode_stft in one call,
    against afgpu.batch_decode_tensor_resampled followed by torch.stft; medians of 5.
No ratio is promised and nothing gates on one.

    python tools/bench_stft.py [--rows 1024] [--call-files 128] [--distinct 32] [--out profiles/stft_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
SHAPES = [dict(n_fft=400, hop=160, n_mels=80, n_out=3000), dict(n_fft=1024, hop=256, n_mels=128, n_out=0)]
SAMPLES, RATE = 480000, 16000
KIND_NAMES = ["complex", "magnitude", "power", "log10"]


def median(v):
    return sorted(v)[len(v) // 2]


def torch_stft(x, n_fft, hop, window, n_out, kind):
    """x [rows, samples] -> [rows, n_bins, n_out]: complex64, or float32 by kind"""
    import torch
    st = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect", return_complex=True)[:, :, :n_out]
    if kind == 0:
        return st.contiguous()
    if kind == 1:
        return st.abs()
    p = st.real ** 2 + st.imag ** 2
    return p if kind == 2 else torch.log10(torch.clamp(p, min=1e-10))


def kernel_leg(n_rows):
    import torch
    import afgpu
    out = []
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

    x = torch.empty((n_rows, SAMPLES), dtype=torch.float32, device="cuda").normal_() * 0.1
    for s in SHAPES:
        n_fft, hop, n_mels, n_bins = s["n_fft"], s["hop"], s["n_mels"], s["n_fft"] // 2 + 1
        mel_prm = afgpu.mel_params(n_fft, hop, n_mels)
        n_out = s["n_out"] or afgpu.mel_frames(mel_prm, SAMPLES)
        window = torch.hann_window(n_fft, periodic=True, device="cuda")
        table = afgpu.mel_fft_tables(n_fft)
        d_table = torch.from_numpy(table.copy()).cuda()
        bank = afgpu.mel_filters(RATE, n_fft, n_mels)
        d_bank = torch.from_numpy(bank.copy()).cuda()
        # E_f of the header per row and frame, from the samples under each window (float64 on the device)
        w64 = torch.hann_window(n_fft, periodic=True, device="cuda", dtype=torch.float64)
        bound_b = 8 * math.ceil(math.log2(n_fft)) + 8

        def e_f(rows):
            xa = torch.nn.functional.pad(x[:rows].abs().double()[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0, :]
            a = torch.nn.functional.conv1d(xa[:, None, :], w64[None, None, :], stride=hop)[:, 0, :n_out]
            return bound_b * 2.0 ** -24 * a                       # [rows, n_out]

        mel_rec = np.zeros(n_rows, afgpu.MEL_ROW_DTYPE)
        mel_rec["in_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
        mel_rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(n_mels * n_out)
        mel_rec["in_frames"], mel_rec["out_frames"] = SAMPLES, n_out
        mel_tiles = afgpu.mel_fft_layout(mel_rec, mel_prm)
        d_mel_rec = torch.from_numpy(mel_rec.view(np.uint8).copy()).cuda()
        d_mel = torch.empty((n_rows, n_mels, n_out), dtype=torch.float32, device="cuda")

        def run_mel():
            afgpu.melspec_fft(n_rows, d_mel_rec, mel_tiles, mel_prm, x, x.numel(), d_table, table.size, d_bank, bank.size, d_mel, d_mel.numel())

        for kind, name in enumerate(KIND_NAMES):
            comps = 2 if kind == afgpu.STFT_COMPLEX else 1
            prm = afgpu.stft_params(n_fft, hop, out_kind=kind)
            rec = mel_rec.copy()
            rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(comps * n_bins * n_out)
            tiles = afgpu.stft_layout(rec, prm)
            d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            d_out = torch.empty((n_rows, n_bins, n_out * comps), dtype=torch.float32, device="cuda")

            def run_stft():
                afgpu.stft(n_rows, d_rec, tiles, prm, x, x.numel(), d_table, table.size, d_out, d_out.numel())

            def run_torch():
                return torch_stft(x, n_fft, hop, window, n_out, kind)

            run_stft()
            worst_in_e = None
            if kind == afgpu.STFT_COMPLEX:                        # |ours - torch.stft| in units of E_f, over a few rows
                rows = min(n_rows, 8)
                ours = torch.view_as_complex(d_out[:rows].reshape(rows, n_bins, n_out, 2))
                diff = torch.view_as_real(ours - torch_stft(x[:rows], n_fft, hop, window, n_out, 0)).abs().amax(dim=(1, 3)).double()
                worst_in_e = float((diff / e_f(rows)).max().item())
            moved = int(x.numel() * 4 + d_out.numel() * 4)
            probe_bytes = moved // 2 // 16 * 16                    # the probe reads and writes what it is given
            src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            ts, tm, tt, tc = [], [], [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit all alike
                ts.append(timed(run_stft))
                tm.append(timed(run_mel))
                tt.append(timed(run_torch))
                tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
            ss, sm_, st_, sc = median(ts), median(tm), median(tt), median(tc)
            out.append({"n_fft": n_fft, "hop": hop, "kind": name, "rows": n_rows, "samples": SAMPLES, "frames": n_out, "tile_frames": afgpu.stft_tile_frames(prm),
                        "tiles": tiles, "bytes_moved": moved, "stft_seconds": ss, "melspec_fft_seconds": sm_, "n_mels": n_mels, "torch_seconds": st_,
                        "copy_probe_seconds": sc, "stft_GBps_moved": moved / ss / 1e9, "copy_GBps_moved": 2 * probe_bytes / sc / 1e9,
                        "of_the_probe": sc / ss, "torch_over_stft": st_ / ss, "stft_over_melspec_fft": ss / sm_,
                        "max_difference_to_torch_in_E_f": worst_in_e})
            print(json.dumps(out[-1]), flush=True)
            del d_out, src, dst
            torch.cuda.empty_cache()
        del d_mel
        torch.cuda.empty_cache()
    return out


def call_leg(blobs, threads):
    import torch
    import afgpu
    s = SHAPES[0]
    n_bins = s["n_fft"] // 2 + 1
    window = torch.hann_window(s["n_fft"], periodic=True, device="cuda")
    out = torch.empty((len(blobs), 1, n_bins, s["n_out"]), dtype=torch.float32, device="cuda")

    def old():
        t, _ = afgpu.batch_decode_tensor_resampled(blobs, SAMPLES, 1, RATE, mono=True, n_threads=threads)
        y = torch_stft(t[:, 0], s["n_fft"], s["hop"], window, s["n_out"], 2)
        torch.cuda.synchronize()
        return y

    def new():
        t, _ = afgpu.batch_decode_stft(blobs, SAMPLES, RATE, s["n_fft"], s["hop"], n_out=s["n_out"], out=out, n_threads=threads)
        torch.cuda.synchronize()
        return t[:, 0]

    a = old()                                                     # warm-up; the two agree to float32 rounding, not bit for bit
    worst = float((a - new()).abs().max().item())
    wall = {"old": [], "new": []}
    for _ in range(PASSES):
        for name, fn in (("old", old), ("new", new)):
            t0 = time.perf_counter()
            fn()
            wall[name].append(time.perf_counter() - t0)
    rec = {"files": len(blobs), "samples": SAMPLES, "shape": [len(blobs), 1, n_bins, s["n_out"]], "kind": "power", "max_abs_difference": worst,
           "largest_power": float(a.max().item())}
    for name in ("old", "new"):
        rec[name + "_seconds"] = median(wall[name])
    rec["speedup"] = rec["old_seconds"] / rec["new_seconds"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--call-files", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_bench.json"))
    args = ap.parse_args()
    res = {"what": "tools/bench_stft.py", "passes": PASSES,
           "note": "kernel leg: timed through the public afg_stft_hip and afg_melspec_fft_hip, which fetch the rows and wait for their stream "
                   "before every launch (the batch path checks its host copy and does not).  old: resampled tensor + torch.stft; new: "
                   "batch_decode_stft"}
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
        res["kernel"] = kernel_leg(args.rows)
        save()
    if not args.skip_call:
        blobs = [bytes(bytearray(distinct["mp3"][i % len(distinct["mp3"])])) for i in range(args.call_files)]
        res["call"] = [call_leg(blobs, args.threads)]
        save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
