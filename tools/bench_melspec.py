#!/usr/bin/env python3
"""tools/bench_melspec.py -- what the mel spectrogram features cost, written to profiles/melspec_bench.json.

(a) kernel leg: rows of 480 000 device-resident samples (30 s at 16 kHz) at the Whisper shape (n_fft 400, hop 160, 80 mels,
    3000 of 3001 frames) and at n_fft 1024, hop 256, 128 mels: afg_melspec_hip (the direct product), afg_melspec_fft_hip (the
    FFT path) and torch.stft + power + matmul with the same bank + log10 on the same device over the same tensor, the three
    alternating in one process, medians of 5.  The float32 MFMA
    rate the kernel is compared with is 155 TFLOP/s; the record carries the fraction reached.
(b) call leg: generated MP3 files (44.1 kHz stereo) to [files, 1, 80, 3000] through afgpu.batch_decode_mel with either
    algorithm, against afgpu.batch_decode_tensor_resampled followed by the same torch expression.  The three alternate; medians
    of 5.
No ratio is promised and nothing gates on one.

    python tools/bench_melspec.py [--rows 1024] [--call-files 256] [--distinct 32] [--out profiles/melspec_bench.json]
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
MFMA_F32_FLOPS = 155e12
SHAPES = [dict(n_fft=400, hop=160, n_mels=80, n_out=3000), dict(n_fft=1024, hop=256, n_mels=128, n_out=0)]
SAMPLES, RATE = 480000, 16000


def median(v):
    return sorted(v)[len(v) // 2]


def torch_features(x, n_fft, hop, d_bank, window, n_out):
    """x [rows, samples] -> [rows, n_mels, n_out]"""
    import torch
    st = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect", return_complex=True)
    power = st.real ** 2 + st.imag ** 2
    mel = torch.matmul(d_bank, power[:, :, :n_out])
    return torch.log10(torch.clamp(mel, min=1e-10))


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
        n_fft, hop, n_mels = s["n_fft"], s["hop"], s["n_mels"]
        prm = afgpu.mel_params(n_fft, hop, n_mels)
        n_out = s["n_out"] or afgpu.mel_frames(prm, SAMPLES)
        basis, bank = afgpu.mel_basis(n_fft), afgpu.mel_filters(RATE, n_fft, n_mels)
        d_basis, d_bank = torch.from_numpy(basis.reshape(-1).copy()).cuda(), torch.from_numpy(bank.copy()).cuda()
        window = torch.hann_window(n_fft, periodic=True, device="cuda")
        rec = np.zeros(n_rows, afgpu.MEL_ROW_DTYPE)
        rec["in_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(SAMPLES)
        rec["out_off"] = np.arange(n_rows, dtype=np.uint64) * np.uint64(n_mels * n_out)
        rec["in_frames"], rec["out_frames"] = SAMPLES, n_out
        tiles = afgpu.mel_layout(rec, prm)
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        fft_rec = rec.copy()
        fft_tiles = afgpu.mel_fft_layout(fft_rec, prm)
        d_fft_rec = torch.from_numpy(fft_rec.view(np.uint8).copy()).cuda()
        table = afgpu.mel_fft_tables(n_fft)
        d_table = torch.from_numpy(table.copy()).cuda()
        d_out = torch.empty((n_rows, n_mels, n_out), dtype=torch.float32, device="cuda")

        def run_kernel():
            afgpu.melspec(n_rows, d_rec, tiles, prm, x, x.numel(), d_basis, basis.size, d_bank, bank.size, d_out, d_out.numel())

        def run_fft():
            afgpu.melspec_fft(n_rows, d_fft_rec, fft_tiles, prm, x, x.numel(), d_table, table.size, d_bank, bank.size, d_out, d_out.numel())

        def run_torch():
            return torch_features(x, n_fft, hop, d_bank, window, n_out)

        run_fft()
        worst_fft = float((run_torch() - d_out).abs().max().item())
        run_kernel()
        worst = float((run_torch() - d_out).abs().max().item())
        tk, tf, tt = [], [], []
        for _ in range(PASSES):                                   # alternating, so that clocks and neighbours hit all alike
            tk.append(timed(run_kernel))
            tf.append(timed(run_fft))
            tt.append(timed(run_torch))
        sk, sf, st_ = median(tk), median(tf), median(tt)
        n_bins = n_fft // 2 + 1
        flops = n_rows * n_out * (2.0 * n_fft * 2 * n_bins + 2.0 * n_bins * n_mels)      # the two products as the definition has them
        out.append({"n_fft": n_fft, "hop": hop, "n_mels": n_mels, "rows": n_rows, "samples": SAMPLES, "frames": n_out, "tiles": tiles,
                    "max_abs_difference_log10": worst, "melspec_seconds": sk, "torch_seconds": st_, "torch_over_melspec": st_ / sk,
                    "fft_tiles": fft_tiles, "fft_max_abs_difference_log10": worst_fft, "fft_seconds": sf, "melspec_over_fft": sk / sf,
                    "torch_over_fft": st_ / sf,
                    "flops": flops, "melspec_TFLOPs": flops / sk / 1e12, "fraction_of_f32_mfma_rate": flops / sk / MFMA_F32_FLOPS,
                    "bytes_read_and_written": n_rows * (SAMPLES + n_mels * n_out) * 4})
        print(json.dumps(out[-1]), flush=True)
        del d_out
        torch.cuda.empty_cache()
    return out


def call_leg(blobs, threads):
    import torch
    import afgpu
    s = SHAPES[0]
    d_bank = torch.from_numpy(afgpu.mel_filters(RATE, s["n_fft"], s["n_mels"]).copy()).cuda()
    window = torch.hann_window(s["n_fft"], periodic=True, device="cuda")
    out = torch.empty((len(blobs), 1, s["n_mels"], s["n_out"]), dtype=torch.float32, device="cuda")

    def old():
        t, _ = afgpu.batch_decode_tensor_resampled(blobs, SAMPLES, 1, RATE, mono=True, n_threads=threads)
        y = torch_features(t[:, 0], s["n_fft"], s["hop"], d_bank, window, s["n_out"])
        torch.cuda.synchronize()
        return y

    def new():
        t, _ = afgpu.batch_decode_mel(blobs, SAMPLES, RATE, n_out=s["n_out"], out=out, n_threads=threads)
        torch.cuda.synchronize()
        return t[:, 0]

    def fft():
        t, _ = afgpu.batch_decode_mel(blobs, SAMPLES, RATE, n_out=s["n_out"], out=out, n_threads=threads, algorithm="fft")
        torch.cuda.synchronize()
        return t[:, 0]

    a = old()                                                     # warm-up; the three agree to float32 rounding, not bit for bit
    worst_fft = float((a - fft()).abs().max().item())
    worst = float((a - new()).abs().max().item())
    wall = {"old": [], "new": [], "fft": []}
    for _ in range(PASSES):
        for name, fn in (("old", old), ("new", new), ("fft", fft)):
            t0 = time.perf_counter()
            fn()
            wall[name].append(time.perf_counter() - t0)
    rec = {"files": len(blobs), "samples": SAMPLES, "frames": s["n_out"], "max_abs_difference_log10": worst}
    rec["fft_max_abs_difference_log10"] = worst_fft
    for name in ("old", "new", "fft"):
        rec[name + "_seconds"] = median(wall[name])
    rec["speedup"] = rec["old_seconds"] / rec["new_seconds"]
    rec["fft_speedup"] = rec["old_seconds"] / rec["fft_seconds"]
    rec["new_over_fft"] = rec["new_seconds"] / rec["fft_seconds"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--call-files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melspec_bench.json"))
    args = ap.parse_args()
    res = {"what": "tools/bench_melspec.py", "passes": PASSES,
           "note": "kernel leg: timed through the public afg_melspec_hip, which fetches the rows and waits for its stream before every "
                   "launch (the batch path checks its host copy and does not); afg_melspec_fft_hip likewise.  old: resampled tensor + torch; "
                   "new: batch_decode_mel, direct; fft: batch_decode_mel, algorithm fft"}
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
