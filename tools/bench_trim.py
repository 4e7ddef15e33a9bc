#!/usr/bin/env python3
"""tools/bench_trim.py -- what the silence trim costs, written to profiles/trim_bench.json.

(a) kernel leg: 1024 groups of 480 000 device-resident floats a row (30 s at 16 kHz), 1 and 2 rows, three seconds of digital
    silence in front of the signal and `begin` at each residue mod 4 (through `lead`), into T = 10 s and T = 30 s:
    afg_trim_hip beside afg_copy_probe_hip over the bytes the stage must move (the rows read once for the powers, the region
    read once more, the slab written once) and beside the torch expression on the same tensor (unfold, square, sum, compare,
    argmax, gather).
(b) call leg: 1024 generated WAV files per call, batch_decode_tensor_trimmed against batch_decode_tensor_resampled at
    scan_frames followed by that torch expression.
The sides alternate in one process; medians of 5.  No ratio is promised and nothing gates on one.

    python tools/bench_trim.py [--groups 1024] [--files 1024] [--out profiles/trim_bench.json]
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
RATE, SAMPLES, ONSET = 16000, 480000, 48000
FRAME, HOP, TOP_DB = 2048, 512, 60.0


def median(v):
    return sorted(v)[len(v) // 2]


def torch_trim(x, T, lead):
    """[n, rows, S] -> [n, rows, T] from the first frame above the threshold on, zeros behind the signal's end"""
    import torch
    p = torch.nn.functional.pad(x, (FRAME // 2, FRAME // 2)).unfold(2, FRAME, HOP).pow(2).sum(dim=(1, 3))      # frame f centred on f * HOP
    loud = p > (10.0 ** (-TOP_DB / 10.0)) * p.amax(1, keepdim=True)
    first = (loud.int().argmax(1) * HOP - lead).clamp_(min=0)
    idx = first[:, None] + torch.arange(T, device=x.device)[None, :]
    inside = idx < x.shape[2]
    got = x.gather(2, idx.clamp_(max=x.shape[2] - 1)[:, None, :].expand(-1, x.shape[1], -1))
    return got * inside[:, None, :]


def timer():
    import torch
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
    return timed


def kernel_leg(n_groups):
    import torch
    import afgpu
    timed = timer()
    out = []
    for rows in (1, 2):
        x = torch.empty((n_groups, rows, SAMPLES), dtype=torch.float32, device="cuda").normal_() * 0.1
        x[:, :, :ONSET] = 0
        for T in (10 * RATE, 30 * RATE):
            y = torch.empty((n_groups, rows, T), dtype=torch.float32, device="cuda")
            groups = np.zeros(n_groups, afgpu.TRIM_GROUP_DTYPE)
            groups["in_off"] = np.arange(n_groups, dtype=np.uint64) * np.uint64(rows * SAMPLES)
            groups["out_off"] = np.arange(n_groups, dtype=np.uint64) * np.uint64(rows * T)
            groups["in_stride"], groups["out_stride"], groups["rows"], groups["out_rows"] = SAMPLES, T, rows, rows
            groups["valid"], groups["out_frames"] = SAMPLES, T
            for residue in range(4):
                lead = (4 - residue) % 4
                prm = afgpu.trim_params(TOP_DB, FRAME, HOP, lead=lead)
                blocks, tiles = afgpu.trim_layout(groups, prm)
                d_groups = torch.from_numpy(groups.view(np.uint8).copy()).cuda()
                d_blocks = torch.empty(blocks * 8, dtype=torch.uint8, device="cuda")
                d_regions = torch.empty(n_groups * 16, dtype=torch.uint8, device="cuda")

                def run_kernel():
                    afgpu.trim(n_groups, d_groups, blocks, tiles, prm, x, x.numel(), y, y.numel(), d_blocks, d_regions)

                run_kernel()
                torch.cuda.synchronize()
                regions = d_regions.cpu().numpy().view(afgpu.TRIM_REGION_DTYPE)
                begin = int(regions["begin"][0])
                assert begin % 4 == residue and (regions["begin"] == begin).all(), (begin, residue)
                copied = np.minimum(regions["end"].astype(np.int64) - regions["begin"], T).sum() * rows * 4
                moved = int(x.numel() * 4 + copied + y.numel() * 4)
                same = bool((torch_trim(x, T, lead) == y).all().item())
                probe_bytes = moved // 2 // 16 * 16                # the probe reads and writes what it is given
                src = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
                dst = torch.empty(probe_bytes, dtype=torch.uint8, device="cuda")
                tk, tc, tt = [], [], []
                for _ in range(PASSES):                           # alternating, so that clocks and neighbours hit all alike
                    tk.append(timed(run_kernel))
                    tc.append(timed(lambda: afgpu.copy_probe(dst, src, probe_bytes)))
                    tt.append(timed(lambda: torch_trim(x, T, lead)))
                sk, sc, st = median(tk), median(tc), median(tt)
                out.append({"rows": rows, "T": T, "begin": begin, "begin_mod_4": residue, "groups": n_groups, "blocks": blocks, "tiles": tiles,
                            "bytes_moved": moved, "equals_torch": same, "trim_seconds": sk, "copy_probe_seconds": sc, "torch_seconds": st,
                            "trim_GBps_moved": moved / sk / 1e9, "copy_GBps_moved": 2 * probe_bytes / sc / 1e9, "of_the_probe": sc / sk,
                            "torch_over_trim": st / sk})
                print(json.dumps(out[-1]), flush=True)
                del src, dst
            del y
        del x
        torch.cuda.empty_cache()
    return out


def call_leg(n_files):
    import time
    import torch
    import afgpu
    import f64_model as fm
    import wav_bitstream as wb
    rng = np.random.default_rng(17)
    kinds = []
    for k in range(8):                                           # 1 to 2.5 s of silence, 8 s of signal, a second of silence
        lead = np.zeros(RATE + 3000 * k, np.int16)
        body = (6000 * rng.standard_normal(8 * RATE)).astype(np.int16)
        kinds.append(wb.wav_file(fm.KIND_S16, 1, RATE, np.concatenate([lead, body, np.zeros(RATE, np.int16)]).astype("<i2").tobytes()))
    files = [kinds[i % 8] for i in range(n_files)]
    T, scan = 5 * RATE, 12 * RATE

    def ours():
        return afgpu.batch_decode_tensor_trimmed(files, T, 1, RATE, scan_frames=scan, mono=True)[0]

    def theirs():
        return torch_trim(afgpu.batch_decode_tensor_resampled(files, scan, 1, RATE, mono=True)[0], T, 0)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    same = bool((ours() == theirs()).all().item())
    to, tt = [], []
    for _ in range(PASSES):
        to.append(wall(ours))
        tt.append(wall(theirs))
    so, st = median(to), median(tt)
    res = {"files": n_files, "frames": T, "scan_frames": scan, "equals_torch": same, "trimmed_seconds": so, "resampled_plus_torch_seconds": st,
           "ratio": st / so, "tensor_samples_per_second": n_files * T / so}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_bench.json"))
    args = ap.parse_args()
    import afgpu
    res = {"what": "tools/bench_trim.py", "passes": PASSES, "device": afgpu.device_name(0),
           "note": "timed through the public afg_trim_hip, which fetches the groups and waits for its stream before every launch "
                   "(the batch path checks its host copy and does not)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():                                                    # after every leg: a later one that fails loses nothing
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    res["kernel"] = kernel_leg(args.groups)
    save()
    res["call"] = call_leg(args.files)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
