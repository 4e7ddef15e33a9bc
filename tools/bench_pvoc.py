#!/usr/bin/env python3
"""tools/bench_pvoc.py -- what the phase-vocoder stage costs, written to profiles/pvoc_bench.json.

Slabs of device-resident complex64 spectra, [201, 3000] with Whisper's framing (n_fft 400, hop 160) and [513, 1876] with
n_fft 1024, hop 256, stretched at rates 0.8, 1.0 and 1.25.  afgpu.phase_vocoder_tensor -- the public entry, which lays the
records out, uploads them and lets afg_pvoc_hip fetch and check them before the launch -- beside the torch expression of the
same definition in float32 as torchaudio has it (torch_phase_vocoder below: angle, abs, index_select twice, round, cumsum,
polar) on the same tensor, and afg_copy_probe_hip over the bytes the stage must move (slab in once, slab out once), all
alternating in one process, medians of 5.  Then afgpu.time_stretch_tensor on rows of 30 s at 16 kHz beside the three-stage
torch chain (torch.stft, that expression, torch.istft).  No ratio is promised and nothing gates on one.

    python tools/bench_pvoc.py [--rows 1024] [--out profiles/pvoc_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "audio-formats_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PASSES = 5
SHAPES = [dict(n_fft=400, hop=160, frames=3000), dict(n_fft=1024, hop=256, frames=1876)]
RATES = [0.8, 1.0, 1.25]


def median(v):
    return sorted(v)[len(v) // 2]


def torch_phase_vocoder(spec, rate, phase_advance):
    """torchaudio.functional.phase_vocoder's lines (float32 for a complex64 tensor)"""
    import torch
    time_steps = torch.arange(0, spec.size(-1), rate, device=spec.device, dtype=torch.float32)
    alphas = time_steps % 1.0
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    s0 = spec.index_select(-1, time_steps.long())
    s1 = spec.index_select(-1, (time_steps + 1).long())
    angle_0, angle_1, norm_0, norm_1 = s0.angle(), s1.angle(), s0.abs(), s1.abs()
    phase = angle_1 - angle_0 - phase_advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = phase + phase_advance
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return torch.polar(mag, phase_acc)


def run(n_rows):
    import torch
    import afgpu
    kernel, chain = [], []
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

    for s in SHAPES:
        n_fft, hop, frames, n_bins = s["n_fft"], s["hop"], s["frames"], s["n_fft"] // 2 + 1
        spec = torch.view_as_complex(torch.empty((n_rows, n_bins, frames, 2), dtype=torch.float32, device="cuda").normal_())
        adv = torch.linspace(0, math.pi * hop, n_bins, device="cuda")[..., None]
        for rate in RATES:
            f_out = afgpu.pvoc_out_frames(frames, rate)
            out = torch.empty((n_rows, n_bins, f_out), dtype=torch.complex64, device="cuda")

            def ours():
                afgpu.phase_vocoder_tensor(spec, rate, n_fft, hop, out=out)

            def theirs():
                return torch_phase_vocoder(spec, rate, adv)

            ours()
            few = min(n_rows, 4)
            ref = theirs()[:few]
            worst = float((out[:few, :, :min(f_out, ref.shape[-1])] - ref[..., :min(f_out, ref.shape[-1])]).abs().max().item())
            del ref
            moved = int(spec.numel() * 8 + out.numel() * 8)
            probe_bytes = moved // 2 // 16 * 16                    # the probe reads and writes what it is given
            src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
            to, tt, tc = [], [], []
            for _ in range(PASSES):                               # alternating, so that clocks and neighbours hit all alike
                to.append(timed(ours))
                tt.append(timed(theirs))
                tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
            so, st, sc = median(to), median(tt), median(tc)
            kernel.append({"n_fft": n_fft, "hop": hop, "slabs": n_rows, "frames": frames, "rate": rate, "out_frames": f_out, "bytes_moved": moved,
                           "pvoc_seconds": so, "torch_seconds": st, "copy_probe_seconds": sc, "pvoc_GBps_moved": moved / so / 1e9,
                           "copy_GBps_moved": 2 * probe_bytes / sc / 1e9, "of_the_probe": sc / so, "torch_over_pvoc": st / so,
                           "steps_per_second": n_rows * n_bins * f_out / so, "max_abs_difference_to_torch_float32": worst})
            print(json.dumps(kernel[-1]), flush=True)
            del out, src, dst
            torch.cuda.empty_cache()
        del spec
        torch.cuda.empty_cache()

    # the whole stretch: rows of 30 s at 16 kHz
    n, n_fft, hop = 480000, 400, 160
    wave = torch.empty((n_rows, n), dtype=torch.float32, device="cuda").normal_().mul_(0.1)
    window = torch.hann_window(n_fft, periodic=True, device="cuda")
    adv = torch.linspace(0, math.pi * hop, n_fft // 2 + 1, device="cuda")[..., None]
    for rate in RATES:
        def ours():
            return afgpu.time_stretch_tensor(wave, rate, n_fft, hop)

        def theirs():
            sp = torch.stft(wave, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect", return_complex=True)
            st = torch_phase_vocoder(sp, rate, adv)
            return torch.istft(st, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, length=int(round(n / rate)))

        y, lengths = ours()
        to, tt = [], []
        for _ in range(PASSES):
            to.append(timed(ours, 1))
            tt.append(timed(theirs, 1))
        so, st = median(to), median(tt)
        chain.append({"n_fft": n_fft, "hop": hop, "rows": n_rows, "samples": n, "rate": rate, "out_samples": int(lengths.max()),
                      "time_stretch_seconds": so, "torch_chain_seconds": st, "torch_over_ours": st / so,
                      "audio_seconds_per_second": n_rows * n / 16000 / so})
        print(json.dumps(chain[-1]), flush=True)
        del y
        torch.cuda.empty_cache()
    return kernel, chain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_pvoc.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through afgpu.phase_vocoder_tensor / time_stretch_tensor: record layout, upload, the entries' fetch and checks, one launch "
                   "per stage; unit-variance complex noise; the torch side is torchaudio's expression in float32"}
    res["kernel"], res["time_stretch"] = run(args.rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
