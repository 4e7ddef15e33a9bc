"""afgpu.batch_decode_mel (afg_batch_decode_mel) on one short generated file of every format, files at 8 and 44.1 kHz among
them, a damaged file and one that is no audio, to 16 kHz mono: the features are afgpu.batch_decode_tensor_resampled of the
same list put through tests/melspec_model.py with the library's tables, bit for bit -- whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as fm
import melspec_model as mm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T, N_FFT, HOP, N_MELS = 16000, 4000, 400, 160, 80
IN_CHANNELS = 3                                                  # two of the generated files have three channels


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()                                        # one file per format
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 3001), (44100, 2, 9000)):
        files.append(wb.wav_file(fm.KIND_S16, ch, rate, wb.random_samples(rng, fm.KIND_S16, ch * frames)))
    files.append(files[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    at = {"r8000": base, "r44100": base + 1, "damaged": base + 2, "junk": base + 3}
    with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, 1, RATE, mono=True, in_channels=IN_CHANNELS, n_threads=4)
        torch.cuda.synchronize()
    assert [i for i, m in enumerate(meta) if m["status"] != 0] == [at["damaged"], at["junk"]]
    assert sorted({m["format"] for m in meta if m["status"] == 0}) == list(range(8))
    assert {8000, 44100} <= {int(m["samplerate"]) for m in meta if m["status"] == 0}
    Cf, Sf = mm.split_basis(afgpu.mel_basis(N_FFT), N_FFT)
    bank = afgpu.mel_filters(RATE, N_FFT, N_MELS)
    rows = tensor.cpu().numpy()[:, 0]
    nf = mm.max_frames(T, N_FFT, HOP, True)
    assert nf == 26
    power = np.stack([mm.melspec32(x, Cf, Sf, bank, N_FFT, N_FFT, HOP, True, mm.PAD_REFLECT, nf)[1] for x in rows])      # made once, never changed
    power.setflags(write=False)
    return {"files": files, "meta": meta, "at": at, "rows": rows, "power": power}


def decode(files, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    n_out = kw.get("n_out", 0) or mm.max_frames(kw.get("frames", T), N_FFT, HOP, True)
    out = torch.full((len(files), 1, N_MELS, n_out), float("nan"), dtype=torch.float32, device="cuda")
    kw.setdefault("frames", T)
    kw.setdefault("in_channels", IN_CHANNELS)
    got, meta = afgpu.batch_decode_mel(files, out=out, n_threads=4, **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()[:, 0], meta


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def test_the_features_are_the_models_of_the_resampled_tensor(corpus):
    got, meta = decode(corpus["files"], out_kind=afgpu.MEL_POWER)
    same(got, corpus["power"])
    assert meta == corpus["meta"]
    at = corpus["at"]
    for bad in (at["damaged"], at["junk"]):                      # what an all-zero row gives, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
    assert got[at["r8000"]].max() > 1.0 and got[at["r44100"]].max() > 1.0 and got[at["damaged"] - 1].max() > 1.0


def test_log_mel_is_the_default_and_a_failed_file_is_the_floor(corpus):
    got, meta = decode(corpus["files"])
    ref = mm.log10_64(corpus["power"])
    ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= 3 * ulp).all()             # log10f: 3 ulp (tests/test_melspec_gpu.py)
    for bad in (corpus["at"]["damaged"], corpus["at"]["junk"]):
        assert (got[bad].view(np.uint32) == got[bad].view(np.uint32)[0, 0]).all() and abs(float(got[bad][0, 0]) + 10.0) < 1e-5


def test_the_features_do_not_depend_on_the_sublists(corpus):
    files = corpus["files"]
    L = afgpu.lib()
    assert L.afg_dev_option(b"mel_scratch_bytes", 1) == 0        # every file its own sublist
    try:
        got, meta = decode(files, out_kind=afgpu.MEL_POWER)
        assert L.afg_dev_option(b"mel_scratch_bytes", 3 * T * 4 + 8) == 0
        three, meta3 = decode(files, out_kind=afgpu.MEL_POWER)
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0
    same(got, corpus["power"])
    same(three, corpus["power"])
    assert meta == meta3 == corpus["meta"]


def test_n_out_crops_the_frames(corpus):
    got, meta = decode(corpus["files"][:4], out_kind=afgpu.MEL_POWER, n_out=25)           # 25 of 26, as Whisper takes 3000 of 3001
    assert got.shape == (4, N_MELS, 25)
    same(got, corpus["power"][:4, :, :25])


def test_other_parameters_and_two_channels(corpus):
    """a zero-padded window, zero padding, HTK bank; without the mono mix, two channel rows per file"""
    files = corpus["files"][:3] + [corpus["files"][corpus["at"]["r44100"]]]
    tensor, meta0 = afgpu.batch_decode_tensor_resampled(files, 3000, 2, RATE, n_threads=4)
    torch.cuda.synchronize()
    out = torch.full((len(files), 2, 23, mm.max_frames(3000, 512, 128, True)), float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_mel(files, 3000, RATE, n_fft=512, hop=128, n_mels=23, win_length=400, pad_mode=afgpu.MEL_PAD_ZERO,
                                       out_kind=afgpu.MEL_POWER, mono=False, channels=2, out=out, scale=afgpu.MEL_SCALE_HTK,
                                       norm=afgpu.MEL_NORM_NONE, f_min=64.0, f_max=7600.0, n_threads=4)
    torch.cuda.synchronize()
    assert meta == meta0
    Cf, Sf = mm.split_basis(afgpu.mel_basis(512, 400), 512)
    bank = afgpu.mel_filters(RATE, 512, 23, 64.0, 7600.0, afgpu.MEL_SCALE_HTK, afgpu.MEL_NORM_NONE)
    rows = tensor.cpu().numpy()
    for i in range(len(files)):
        for k in range(2):
            want = mm.melspec32(rows[i, k], Cf, Sf, bank, 512, 400, 128, True, mm.PAD_ZERO, out.shape[3])[1]
            same(got[i, k].cpu().numpy(), want)


def test_refusals_inherited_from_the_resampled_entry(corpus):
    files, at = corpus["files"], corpus["at"]
    part = [files[at["r8000"]], files[at["r44100"]], files[0]]
    got, meta = decode(part, out_kind=afgpu.MEL_POWER, max_in_rate=16000)                 # the 44.1 kHz file is above max_in_rate
    assert meta[1]["status"] == -5 and "44100" in meta[1]["message"] and "16000" in meta[1]["message"]
    assert (got[1].view(np.uint32) == 0).all()
    same(got[0], corpus["power"][at["r8000"]])
    got, meta = decode(part, out_kind=afgpu.MEL_POWER, in_channels=1)                     # ... and has more channels than in_channels
    assert meta[1]["status"] == -5 and (got[1].view(np.uint32) == 0).all() and meta[0]["status"] == 0
    same(got[0], corpus["power"][at["r8000"]])
    empty, meta = afgpu.batch_decode_mel([], T)
    assert tuple(empty.shape) == (0, 1, N_MELS, 26) and empty.is_cuda and meta == []
    for out in (torch.empty((3, 1, N_MELS, 26), dtype=torch.float64, device="cuda"), torch.empty((3, 1, N_MELS, 27), device="cuda"),
                torch.empty((3, 1, N_MELS, 26))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mel(part, T, out=out)
