#!/usr/bin/env python3
"""tools/bench_fbank.py -- what the Kaldi-compatible filter-bank stage costs, written to profiles/fbank_bench.json.

Rows of 480 000 device-resident samples (30 s at 16 kHz), Kaldi's framing at that rate (25 ms / 10 ms, n_fft 512, snip_edges,
DC removal, pre-emphasis 0.97, Povey's window, log) with 80 and 23 mels, in both layouts: afg_fbank_hip beside
afg_melspec_fft_hip at n_fft 512 / hop 160 / 80 mels on the same rows -- the same transform and the same product, so the
ratio is the measure --, afg_copy_probe_hip over the bytes the stage must move (input once, output once), and a torch
expression of the definition on the same tensor, all alternating in one process, medians of 5.  No ratio is promised and
nothing gates on one.

    python tools/bench_fbank.py [--rows 1024] [--out profiles/fbank_bench.json]
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
SAMPLES, RATE, WS, HOP, N_FFT = 480000, 16000, 400, 160, 512
TORCH_ROWS = 128                                                 # the torch expression holds every frame: it runs on a slice and is scaled


def median(v):
    return sorted(v)[len(v) // 2]


def torch_fbank(x, window, bank_t):
    """the definition in torch ops, float32: [rows, samples] -> [rows, frames, n_mels]"""
    import torch
    fr = x.unfold(1, WS, HOP)
    fr = fr - fr.mean(dim=2, keepdim=True)
    prev = torch.cat((fr[:, :, :1], fr[:, :, :-1]), dim=2)
    fr = (fr - 0.97 * prev) * window
    p = torch.fft.rfft(fr, n=N_FFT).abs().pow(2.0)
    return torch.clamp(p @ bank_t, min=torch.finfo(torch.float32).eps).log()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_bench.json"))
    args = ap.parse_args()
    import torch
    import afgpu
    n_rows = args.rows
    res = {"what": "tools/bench_fbank.py", "passes": PASSES, "device": afgpu.device_name(0), "rows": n_rows, "samples": SAMPLES,
           "note": "timed through the public afg_fbank_hip and afg_melspec_fft_hip, which fetch the rows and wait for their stream before every "
                   f"launch.  torch: the definition in float32 tensor ops on {TORCH_ROWS} rows, scaled to the row count", "cases": []}
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
    # the FFT mel path on the same rows: n_fft 512, hop 160, 80 mels
    mel_prm = afgpu.mel_params(N_FFT, HOP, 80)
    mel_out = afgpu.mel_frames(mel_prm, SAMPLES)
    mel_rec = np.zeros(n_rows, afgpu.MEL_ROW_DTYPE)
    mel_rec["in_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
    mel_rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(80 * mel_out)
    mel_rec["in_frames"], mel_rec["out_frames"] = SAMPLES, mel_out
    mel_tiles = afgpu.mel_fft_layout(mel_rec, mel_prm)
    d_mel_rec = torch.from_numpy(mel_rec.view(np.uint8).copy()).cuda()
    mel_table = afgpu.mel_fft_tables(N_FFT)
    d_mel_table = torch.from_numpy(mel_table.copy()).cuda()
    mel_bank = afgpu.mel_filters(RATE, N_FFT, 80)
    d_mel_bank = torch.from_numpy(mel_bank.copy()).cuda()
    d_mel = torch.empty((n_rows, 80, mel_out), dtype=torch.float32, device="cuda")

    def run_mel():
        afgpu.melspec_fft(n_rows, d_mel_rec, mel_tiles, mel_prm, x, x.numel(), d_mel_table, mel_table.size, d_mel_bank, mel_bank.size, d_mel, d_mel.numel())

    table = afgpu.fbank_tables("povey", WS, N_FFT)
    d_table = torch.from_numpy(table.copy()).cuda()
    for n_mels in (80, 23):
        bank = afgpu.fbank_filters(RATE, N_FFT, n_mels, 20.0, 0.0)
        d_bank = torch.from_numpy(bank.reshape(-1).copy()).cuda()
        bank_t = d_bank.reshape(n_mels, N_FFT // 2 + 1).T.contiguous()
        window = d_table[:WS]
        for name, layout in (("frames_major", afgpu.FBANK_FRAMES_MAJOR), ("mel_major", afgpu.FBANK_MEL_MAJOR)):
            prm = afgpu.fbank_params(WS, HOP, N_FFT, n_mels, energy_floor=0.0, layout=layout)
            frames = afgpu.fbank_frames(prm, SAMPLES)
            rec = mel_rec.copy()
            rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(n_mels * frames)
            rec["out_frames"] = frames
            tiles = afgpu.fbank_layout(rec, prm)
            d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            d_out = torch.empty((n_rows, frames * n_mels), dtype=torch.float32, device="cuda")

            def run_fbank():
                afgpu.fbank(n_rows, d_rec, tiles, prm, x, x.numel(), d_table, table.size, d_bank, bank.size, d_out, d_out.numel())

            def run_torch():
                return torch_fbank(x[:min(TORCH_ROWS, n_rows)], window, bank_t)

            run_fbank()
            rows = min(n_rows, 8)
            ours = d_out[:rows].reshape(rows, frames, n_mels) if layout == afgpu.FBANK_FRAMES_MAJOR else d_out[:rows].reshape(rows, n_mels, frames).transpose(1, 2)
            worst = float((ours - torch_fbank(x[:rows], window, bank_t)).abs().max().item())
            moved = int(x.numel() * 4 + d_out.numel() * 4)
            probe_bytes = moved // 2 // 16 * 16                    # the probe reads and writes what it is given
            src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            tf, tm, tt, tc = [], [], [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit all alike
                tf.append(timed(run_fbank))
                tm.append(timed(run_mel))
                tt.append(timed(run_torch) * n_rows / min(TORCH_ROWS, n_rows))
                tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
            sf, sm, st, sc = median(tf), median(tm), median(tt), median(tc)
            res["cases"].append({"n_mels": n_mels, "layout": name, "frames": frames, "tiles": tiles, "bytes_moved": moved, "fbank_seconds": sf,
                                 "melspec_fft_80_seconds": sm, "torch_seconds": st, "copy_probe_seconds": sc, "fbank_GBps_moved": moved / sf / 1e9,
                                 "copy_GBps_moved": 2 * probe_bytes / sc / 1e9, "fbank_over_melspec_fft": sf / sm, "torch_over_fbank": st / sf,
                                 "of_the_probe": sc / sf, "max_abs_difference_to_torch_log": worst})
            print(json.dumps(res["cases"][-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:                       # after every case: a later one that fails loses nothing
                json.dump(res, fh, indent=1)
            del d_out, src, dst
            torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
