"""afgpu.batch_decode_tensor_filtered (afg_batch_decode_filtered) on one short generated file of every format, files at 8 and
44.1 kHz, a damaged file and one that is no audio: bit for bit afg_filter_hip over batch_decode_tensor_resampled's tensor with
the rows and valid lengths of the normalisation definition, +0.0 behind them, whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64
import filter_model as fm
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

T = 4000
IN_CHANNELS = 3                                                  # two of the generated files have three channels
SOS = [fm.design("highpass", 16000.0, 80.0), fm.design("peaking", 16000.0, 1000.0, 2.0, 6.0)]
LAYOUTS = {"mono": (1, True), "one-channel": (1, False), "two-channels": (2, False)}
RATES = (16000, 22050)


@pytest.fixture(scope="module")
def files(gpu):
    out = build_files()                                          # one file per format
    rng = np.random.default_rng(73)
    for rate, ch, frames in ((8000, 1, 1501), (44100, 2, 9000)):
        out.append(wb.wav_file(f64.KIND_S16, ch, rate, wb.random_samples(rng, f64.KIND_S16, ch * frames)))
    out.append(out[2][:-100])                                    # a file cut short
    out.append(b"RIFF" + b"\x00" * 40)
    return out


@pytest.fixture(scope="module")
def reference(files):
    """per (layout, rate): the resampled tensor with afg_filter_hip run over the rows of the definition, and the call's meta"""
    ref = {}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for name, (C, mono) in LAYOUTS.items():
            for rate in RATES:
                tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, C, rate, mono=mono, in_channels=IN_CHANNELS, n_threads=4)
                rows, valid = [], []
                for i, m in enumerate(meta):
                    n = nm.valid_length(m["frames"], 0, round(m["samplerate"]), rate, T) if m["status"] == 0 else 0
                    k = (1 if mono else min(C, m["channels"])) if m["status"] == 0 else 0
                    valid.append((k, n))
                    rows += [((i * C + r) * T, n) for r in range(k) if n]
                rec = np.zeros(len(rows), afgpu.FILTER_ROW_DTYPE)
                rec["in_off"] = rec["out_off"] = [o for o, _ in rows]
                rec["frames"] = [n for _, n in rows]
                want = tensor.clone()
                afgpu.filter_rows(len(rec), torch.from_numpy(rec.view(np.uint8)).cuda(), SOS, want, want.numel(), want, want.numel())
                torch.cuda.synchronize()
                want = want.cpu().numpy()
                for i, (k, n) in enumerate(valid):               # nothing lies behind valid: the resampler's own tail goes
                    want[i, :, n:] = 0.0
                ref[name, rate] = (tensor.cpu().numpy(), want, meta, valid)
    return ref


def decode(files, name, rate):
    C, mono = LAYOUTS[name]
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")       # an element nobody wrote shows
    got, meta = afgpu.batch_decode_tensor_filtered(files, T, C, rate, SOS, mono=mono, in_channels=IN_CHANNELS, out=out, n_threads=4)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_tensor_is_the_resampled_one_through_the_kernel(files, reference, name, rate):
    plain, want, want_meta, valid = reference[name, rate]
    got, meta = decode(files, name, rate)
    assert meta == want_meta
    assert nm.same_bits(got, want).size == 0
    damaged, junk = len(files) - 2, len(files) - 1
    for bad in (damaged, junk):                                  # a zero slab, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
    assert np.abs(got[damaged - 1]).max() > 0
    moved = 0
    for i, (k, n) in enumerate(valid):                           # +0.0 behind a file's samples and in the rows it has no channel for
        assert (got[i, k:].view(np.uint32) == 0).all() and (got[i, :, n:].view(np.uint32) == 0).all()
        moved += bool(k and n and (got[i].view(np.uint32) != plain[i].view(np.uint32)).any())
    assert moved >= 10 and any(0 < n < T for _, n in valid)     # the filter did something; some file ends inside the tensor
    # ... and what it did is the cascade: a mono row against the model, inside the header's interval
    if name == "mono":
        i = next(i for i, (k, n) in enumerate(valid) if n == T)
        sig = fm.run(SOS, plain[i, 0])
        KE = afgpu.FILTER_K * fm.bound(SOS) * float(np.abs(plain[i, 0]).max())
        assert (np.abs(got[i, 0].astype(fm.WIDE) - sig[-1][0]).astype(np.float64) <= fm.allowance(sig[-1][0], KE)).all()


def test_the_entry_does_not_depend_on_the_sublists(files, reference):
    L = afgpu.lib()
    _, want, want_meta, _ = reference["mono", 16000]
    slab = IN_CHANNELS * (T * 48000 // 16000 + 2 * 19 + 1) * 4   # the resampler's scratch: R_s * T_s floats, H = W(48000 -> 16000) = 19
    try:
        for value in (1, 3 * slab + slab // 2):                  # every file its own sublist; three files
            assert L.afg_dev_option(b"resample_scratch_bytes", value) == 0
            got, meta = decode(files, "mono", 16000)
            assert nm.same_bits(got, want).size == 0 and meta == want_meta
    finally:
        assert L.afg_dev_option(b"resample_scratch_bytes", -1) == 0


def test_python_refusals_and_empty_lists(files):
    part = files[:2]
    for kw in (dict(frames=0), dict(channels=0), dict(samplerate=0), dict(channels=2, mono=True), dict(sos=[(1.0, 0.0, 0.0, -2.0, 1.0)]),
               dict(sos=[SOS[0]] * 9), dict(sos=[(1.0, 0.0, float("nan"), 0.0, 0.0)])):
        args = dict(frames=T, channels=1, samplerate=16000, sos=SOS)
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_filtered(part, **args)
    got, meta = afgpu.batch_decode_tensor_filtered([], T, 1, 16000, SOS)
    assert tuple(got.shape) == (0, 1, T) and meta == []
