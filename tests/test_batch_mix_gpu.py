"""afgpu.batch_decode_tensor_noisy (afg_batch_decode_mixed) on one short generated file of every format, files at 8 and
44.1 kHz, a damaged file and one that is no audio: bit for bit afgpu.add_noise_tensor over batch_decode_tensor_resampled's tensor
with the files' valid lengths and rows, records included, whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

T = 9000
IN_CHANNELS = 3                                                  # two of the generated files have three channels
LAYOUTS = {"mono": (1, True), "one-channel": (1, False), "two-channels": (2, False)}
RATES = (8000, 16000)
CLIP = 5000                                                      # shorter than the tensor's rows: it loops


@pytest.fixture(scope="module")
def files(gpu):
    out = build_files()                                          # one file per format
    rng = np.random.default_rng(79)
    for rate, ch, frames in ((8000, 1, 1501), (44100, 2, 30000)):
        out.append(wb.wav_file(f64.KIND_S16, ch, rate, wb.random_samples(rng, f64.KIND_S16, ch * frames)))
    out.append(out[2][:-100])                                    # a file cut short
    out.append(b"RIFF" + b"\x00" * 40)
    return out


@pytest.fixture(scope="module")
def banks(gpu):
    """a bank shared by the channels and one with a row per channel; lengths, clips, starts and levels per file"""
    rng = np.random.default_rng(80)
    return {1: torch.from_numpy((0.05 * rng.standard_normal((3, CLIP))).astype(np.float32)).cuda(),
            2: torch.from_numpy((0.05 * rng.standard_normal((3, 2, CLIP))).astype(np.float32)).cuda()}


def noise_args(n):
    return dict(noise_lengths=[CLIP, 4097, 63], noise_index=[i % 3 for i in range(n)], noise_start=[0, 1, CLIP + 5, 4096, 62][:n] + [7 * i for i in range(5, n)],
                snr_db=[(-5.0, 0.0, 20.0)[i % 3] for i in range(n)])


def bank_of(banks, name, per_channel):
    return banks[2] if per_channel and LAYOUTS[name][0] == 2 else banks[1]


@pytest.fixture(scope="module")
def reference(files, banks):
    """per (layout, rate, bank): the resampled tensor, add_noise_tensor over it with the definition's valid lengths and rows, its
    records and the call's meta"""
    ref = {}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for name, (C, mono) in LAYOUTS.items():
            for rate in RATES:
                tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, C, rate, mono=mono, in_channels=IN_CHANNELS, n_threads=4)
                valid, rows = np.zeros(len(files), np.int64), np.ones(len(files), np.int64)
                for i, m in enumerate(meta):
                    if m["status"] == 0:
                        valid[i] = nm.valid_length(m["frames"], 0, round(m["samplerate"]), rate, T)
                        rows[i] = 1 if mono else min(C, m["channels"])
                for per_channel in (False, True):
                    bank = bank_of(banks, name, per_channel)
                    want = tensor.clone()
                    stats = np.zeros(len(files), afgpu.MIX_STATS_DTYPE)
                    for k in sorted(set(rows.tolist())):         # add_noise_tensor takes every channel row: one call per row count
                        sel = np.flatnonzero(rows == k)
                        idx = torch.from_numpy(sel).cuda()
                        part = want[idx][:, :k].contiguous()
                        kw = {key: [v[i] for i in sel] if key != "noise_lengths" else v for key, v in noise_args(len(files)).items()}
                        got, st = afgpu.add_noise_tensor(part, bank if bank.dim() == 2 else bank[:, :k].contiguous(), valid=valid[sel], out=part, **kw)
                        want[idx, :k] = got
                        stats[sel] = st
                    torch.cuda.synchronize()
                    ref[name, rate, per_channel] = (tensor.cpu().numpy(), want.cpu().numpy(), stats, meta, valid, rows)
    return ref


def decode(files, banks, name, rate, per_channel):
    C, mono = LAYOUTS[name]
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")       # an element nobody wrote shows
    got, meta, stats = afgpu.batch_decode_tensor_noisy(files, T, C, rate, bank_of(banks, name, per_channel), mono=mono, in_channels=IN_CHANNELS, out=out,
                                                       n_threads=4, **noise_args(len(files)))
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta, stats


@pytest.mark.parametrize("per_channel", (False, True))
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_tensor_is_the_resampled_one_through_add_noise_tensor(files, banks, reference, name, rate, per_channel):
    plain, want, want_stats, want_meta, valid, rows = reference[name, rate, per_channel]
    got, meta, stats = decode(files, banks, name, rate, per_channel)
    assert meta == want_meta
    assert nm.same_bits(got, want).size == 0
    assert stats.tobytes() == want_stats.tobytes()
    damaged, junk = len(files) - 2, len(files) - 1
    for bad in (damaged, junk):                                  # a zero slab and a zero record, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
        assert stats[bad].tobytes() == bytes(24)
    mixed = 0
    for i in range(len(files)):
        k, n = int(rows[i]), int(valid[i])
        st = stats[i]
        assert (got[i, k:].view(np.uint32) == plain[i, k:].view(np.uint32)).all() and (got[i, :, n:].view(np.uint32) == plain[i, :, n:].view(np.uint32)).all()
        if n and st["flags"] == 0:                               # the level is reached over the file's own samples
            snr = 10 * np.log10(st["signal_energy"] / (float(st["gain"]) ** 2 * st["noise_energy"]))
            assert abs(snr - noise_args(len(files))["snr_db"][i]) < 1e-5
            assert abs(st["signal_energy"] - float((plain[i, :k, :n].astype(np.float64) ** 2).sum())) <= 1e-12 * st["signal_energy"]
            assert (got[i, :k, :n] != plain[i, :k, :n]).any()
            mixed += 1
    assert mixed >= 4 and any(0 < int(v) < T for v in valid) and any(int(v) > CLIP for v in valid)


def test_the_entry_does_not_depend_on_the_sublists(files, banks, reference):
    L = afgpu.lib()
    _, want, want_stats, want_meta, _, _ = reference["two-channels", 16000, True]
    slab = IN_CHANNELS * (T * 48000 // 16000 + 2 * 19 + 1) * 4   # the resampler's scratch: R_s * T_s floats, H = W(48000 -> 16000) = 19
    try:
        for value in (1, 3 * slab + slab // 2):                  # every file its own sublist; three files
            assert L.afg_dev_option(b"resample_scratch_bytes", value) == 0
            got, meta, stats = decode(files, banks, "two-channels", 16000, True)
            assert nm.same_bits(got, want).size == 0 and meta == want_meta and stats.tobytes() == want_stats.tobytes()
    finally:
        assert L.afg_dev_option(b"resample_scratch_bytes", -1) == 0


def test_empty_lists_and_refusals(files, banks):
    got, meta, stats = afgpu.batch_decode_tensor_noisy([], T, 2, 16000, banks[1], 0.0)
    assert tuple(got.shape) == (0, 2, T) and meta == [] and len(stats) == 0
    for kw in (dict(snr_db=float("inf")), dict(noise_index=3), dict(noise_lengths=CLIP + 1), dict(snr_db=[0.0, 1.0])):
        args = dict(snr_db=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_noisy(files[:1], T, 2, 16000, banks[1], **args)
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor_noisy(files[:1], T, 1, 16000, banks[2], 0.0)      # a bank of two channels against a tensor of one
    out = torch.zeros((1, 2, T), dtype=torch.float32, device="cuda")
    with pytest.raises(afgpu.AfgError, match="overlaps the tensor"):
        afgpu.batch_decode_tensor_noisy(files[:1], T, 2, 16000, out.reshape(2, T), 0.0, out=out)      # the tensor as its own bank
