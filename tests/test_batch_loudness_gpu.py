"""afgpu.batch_decode_tensor_loudnorm (afg_batch_decode_loudnorm) on one short generated file of every format, files at 8 and
44.1 kHz, a damaged file and one that is no audio: bit for bit afg_loudness_hip over batch_decode_tensor_resampled's tensor with
the groups and valid lengths of the normalisation definition, records included, whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64
import loudness_model as lm
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

T = 9000                                                         # more than 400 ms at both rates
IN_CHANNELS = 3                                                  # two of the generated files have three channels
LAYOUTS = {"mono": (1, True), "one-channel": (1, False), "two-channels": (2, False)}
RATES = (16000, 22050)
KW = dict(target_lufs=-20.0, max_peak=0.9)


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
def reference(files):
    """per (layout, rate): the resampled tensor, afg_loudness_hip run in place over the groups of the definition, its records and
    the call's meta"""
    ref = {}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for name, (C, mono) in LAYOUTS.items():
            for rate in RATES:
                tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, C, rate, mono=mono, in_channels=IN_CHANNELS, n_threads=4)
                prm = afgpu.loudness_params(rate, **KW)
                groups = np.zeros(len(files), afgpu.LOUDNESS_GROUP_DTYPE)
                groups["in_off"] = groups["out_off"] = np.arange(len(files), dtype=np.uint64) * np.uint64(C * T)
                groups["stride"], groups["rows"] = T, 1
                for i, m in enumerate(meta):
                    if m["status"] == 0:
                        groups[i]["valid"] = nm.valid_length(m["frames"], 0, round(m["samplerate"]), rate, T)
                        groups[i]["rows"] = 1 if mono else min(C, m["channels"])
                counts = afgpu.loudness_layout(groups, prm)
                want = tensor.clone()
                d_stats = torch.zeros(len(files) * afgpu.LOUDNESS_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                afgpu.loudness(len(files), torch.from_numpy(groups.view(np.uint8)).cuda(), counts, prm, want, want.numel(), want, want.numel(),
                               torch.empty(max(counts.n_sub, 1), dtype=torch.float64, device="cuda"),
                               torch.empty(max(counts.n_blocks, 1), dtype=torch.float64, device="cuda"), d_stats)
                torch.cuda.synchronize()
                ref[name, rate] = (tensor.cpu().numpy(), want.cpu().numpy(), d_stats.cpu().numpy().view(afgpu.LOUDNESS_STATS_DTYPE).copy(), meta, groups)
    return ref


def decode(files, name, rate, **kw):
    C, mono = LAYOUTS[name]
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")       # an element nobody wrote shows
    args = dict(KW)
    args.update(kw)
    got, meta, stats = afgpu.batch_decode_tensor_loudnorm(files, T, C, rate, mono=mono, in_channels=IN_CHANNELS, out=out, n_threads=4, **args)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta, stats


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_tensor_is_the_resampled_one_through_the_kernels(files, reference, name, rate):
    plain, want, want_stats, want_meta, groups = reference[name, rate]
    got, meta, stats = decode(files, name, rate)
    assert meta == want_meta
    assert nm.same_bits(got, want).size == 0
    assert stats.tobytes() == want_stats.tobytes()
    damaged, junk = len(files) - 2, len(files) - 1
    for bad in (damaged, junk):                                  # a zero slab and a zero record with gain 1, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
        assert stats[bad]["energy"] == 0 and stats[bad]["n_blocks"] == 0 and stats[bad]["peak"] == 0 and stats[bad]["gain"] == 1.0
        assert stats[bad]["flags"] == afgpu.LOUDNESS_UNGATED
    levelled = 0
    for i, g in enumerate(groups):
        k, n = int(g["rows"]), int(g["valid"])
        st = stats[i]
        assert (got[i, :k, :n].view(np.uint32) == (plain[i, :k, :n] * st["gain"]).view(np.uint32)).all()
        assert (got[i, k:].view(np.uint32) == plain[i, k:].view(np.uint32)).all() and (got[i, :, n:].view(np.uint32) == plain[i, :, n:].view(np.uint32)).all()
        if st["n_gated"] and np.isfinite(plain[i, :k, :n]).all():    # the measurement is the model's, and the gain leads to the target
            m = lm.measure(plain[i, :k], n, rate)
            assert (st["n_blocks"], st["n_abs"], st["n_gated"]) == (m["n_blocks"], m["n_abs"], int(m["gated"].sum()))
            assert abs(afgpu.loudness_lufs(st["energy"]) - lm.lufs(float(m["energy"]))) < 1e-9
            if not st["flags"]:
                assert abs(afgpu.loudness_lufs(st["energy"] * float(st["gain"]) ** 2) + 20.0) < 1e-5
                levelled += 1
        if st["flags"] & afgpu.LOUDNESS_PEAK_CLAMPED:
            assert np.abs(got[i, :k, :n]).max() <= np.float32(0.9) * (1 + 2.0 ** -22)
    assert levelled >= 2 and any(0 < int(g["valid"]) < T for g in groups) and any(s["n_blocks"] == 0 and s["peak"] > 0 for s in stats)
    # measuring only leaves the resampled tensor as it is and gives the same records
    same, _, measured = decode(files, name, rate, apply=False)
    assert nm.same_bits(same, plain).size == 0 and stats.tobytes() == measured.tobytes()


def test_the_entry_does_not_depend_on_the_sublists(files, reference):
    L = afgpu.lib()
    _, want, want_stats, want_meta, _ = reference["two-channels", 16000]
    slab = IN_CHANNELS * (T * 48000 // 16000 + 2 * 19 + 1) * 4   # the resampler's scratch: R_s * T_s floats, H = W(48000 -> 16000) = 19
    try:
        for value in (1, 3 * slab + slab // 2):                  # every file its own sublist; three files
            assert L.afg_dev_option(b"resample_scratch_bytes", value) == 0
            got, meta, stats = decode(files, "two-channels", 16000)
            assert nm.same_bits(got, want).size == 0 and meta == want_meta and stats.tobytes() == want_stats.tobytes()
    finally:
        assert L.afg_dev_option(b"resample_scratch_bytes", -1) == 0


def test_empty_lists(files):
    got, meta, stats = afgpu.batch_decode_tensor_loudnorm([], T, 2, 16000)
    assert tuple(got.shape) == (0, 2, T) and meta == [] and len(stats) == 0
