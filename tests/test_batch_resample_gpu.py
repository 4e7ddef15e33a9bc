"""afgpu.batch_decode_tensor_resampled (afg_batch_decode_resampled) on one file of every format at four and more sample
rates, a damaged file and one that is no audio: the tensor is what afgpu.batch_decode returns for the same list, mixed and
resampled by tests/resample_model.py with the library's tables, bit for bit (NaN for NaN where the model's value is NaN) --
whatever the sublists, the stages' chunks or the file's place in the batch."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as fm
import resample_model as rm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

WIDE_CHANNELS, WIDE_FRAMES = 70, 201
SHAPES = [(1, 1), (2, 4000), (1, 100000)]


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()
    base = len(files)
    rng = np.random.default_rng(71)
    for rate, ch, frames in ((8000, 1, 3001), (22050, 2, 2500), (96000, 2, 9000)):
        files.append(wb.wav_file(fm.KIND_S16, ch, rate, wb.random_samples(rng, fm.KIND_S16, ch * frames)))
    nans = np.frombuffer(wb.random_samples(rng, fm.KIND_F32, 2 * 1800), "<f4").copy()
    nans[5::97] = np.nan
    files.append(wb.wav_file(fm.KIND_F32, 2, 44100, nans.astype("<f4").tobytes()))
    files.append(wb.wav_file(fm.KIND_S16, WIDE_CHANNELS, 48000, wb.random_samples(rng, fm.KIND_S16, WIDE_CHANNELS * WIDE_FRAMES)))
    files.append(files[2][:-100])                                                # a WAV file whose data chunk is cut short
    files.append(b"RIFF" + b"\x00" * 40)
    at = {"r8000": base, "r22050": base + 1, "r96000": base + 2, "nans": base + 3, "wide": base + 4, "damaged": base + 5, "junk": base + 6}
    with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        floats = afgpu.batch_decode(files, n_threads=4)
    assert [i for i, f in enumerate(floats) if f["status"] != 0] == [at["damaged"], at["junk"]]
    assert sorted({f["format"] for f in floats if f["status"] == 0}) == list(range(8))        # WAV, MP3, FLAC, OGG, OPUS, QOA, MOD, XM
    assert len({int(f["samplerate"]) for f in floats if f["status"] == 0}) >= 4
    assert np.isnan(floats[at["nans"]]["pcm"]).any() and floats[at["wide"]]["channels"] == WIDE_CHANNELS
    return {"files": files, "floats": floats, "at": at, "tables": {}}


def taps_for(corpus, samplerate):
    """the library's own table per file rate, made once"""
    def get(rate):
        key = (rate, samplerate)
        if key not in corpus["tables"]:
            corpus["tables"][key] = afgpu.resample_taps(rate, samplerate)[0]
        return corpus["tables"][key]
    return get


def first_frames(floats, varied):
    if not varied:
        return None
    ff = [(37 * (i + 1)) % max(f["frames"], 1) for i, f in enumerate(floats)]
    ff[0] = floats[0]["frames"] - 1                                              # the last frame
    ff[1] = floats[1]["frames"] + 5                                              # past the end
    ff[4] = floats[4]["frames"]                                                  # exactly the end
    return ff


def decode(files, C, T, samplerate, ff=None, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_tensor_resampled(files, T, C, samplerate, first_frame=ff, out=out, n_threads=4, **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


def same(got, want):
    bad = rm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def check_meta(meta, floats, mono=False, in_channels=2, max_in_rate=48000):
    for m, f in zip(meta, floats):
        why = rm.refusal(f, mono, in_channels, max_in_rate) if f["status"] == 0 else None
        if why is None:
            assert m == {k: v for k, v in f.items() if k != "pcm"}
            continue
        assert m["status"] == -5 and {k: m[k] for k in ("format", "channels", "samplerate", "frames")} == {k: f[k] for k in ("format", "channels", "samplerate", "frames")}
        numbers = (str(int(f["samplerate"])), str(max_in_rate)) if why == "rate" else (str(f["channels"]), str(in_channels))
        assert all(n in m["message"] for n in numbers), m["message"]


@pytest.mark.parametrize("varied", [False, True], ids=["from-0", "varied-first-frame"])
@pytest.mark.parametrize("mono", [False, True], ids=["plain", "mono"])
@pytest.mark.parametrize("C,T", SHAPES)
@pytest.mark.parametrize("samplerate", [16000, 48000])
def test_the_tensor_is_the_resampled_float_batch(corpus, samplerate, C, T, mono, varied):
    files, floats, at = corpus["files"], corpus["floats"], corpus["at"]
    C = 1 if mono else C                                                         # (a mono tensor has one channel)
    ff = first_frames(floats, varied)
    got, meta = decode(files, C, T, samplerate, ff, mono=mono)
    want = rm.tensor(floats, C, T, samplerate, ff, mono=mono, taps_of=taps_for(corpus, samplerate))
    same(got, want)
    check_meta(meta, floats, mono)
    for bad in (at["damaged"], at["junk"], at["r96000"]):
        assert meta[bad]["status"] != 0 and (got[bad].view(np.uint32) == 0).all()
    if varied:
        # file 1 starts 5 frames past its end: only the filter's leading taps still reach it, W - 1 frames back
        M, L, W, _ = rm.shape(int(floats[1]["samplerate"]), samplerate)
        assert floats[1]["status"] == 0 and (got[1][:, -(-max(W - 6, 0) * L // M):] == 0).all()
    if T > 1:
        assert np.abs(want[at["r8000"]]).max() > 0.01 and np.isnan(want[at["nans"]]).any()


def test_the_tensor_does_not_depend_on_the_sublists(corpus):
    files, floats = corpus["files"], corpus["floats"]
    C, T, rate = 2, 4000, 16000
    ff = first_frames(floats, True)
    plain, meta0 = decode(files, C, T, rate, ff)
    slab = C * (T * 48000 // rate + 2 * 19 + 1) * 4                              # R_s * T_s floats: H = W(48000 -> 16000) = 19
    per_list = 5
    assert -(-len(files) // per_list) >= 3
    L = afgpu.lib()
    assert L.afg_dev_option(b"resample_scratch_bytes", per_list * slab + slab // 2) == 0
    try:
        got, meta = decode(files, C, T, rate, ff)
        assert L.afg_dev_option(b"resample_scratch_bytes", 1) == 0                # a sublist holds one file at the least
        one_each, meta1 = decode(files, C, T, rate, ff)
    finally:
        assert L.afg_dev_option(b"resample_scratch_bytes", -1) == 0
    same(got, rm.tensor(floats, C, T, rate, ff, taps_of=taps_for(corpus, rate)))
    assert (got.view(np.uint32) == plain.view(np.uint32)).all() and (one_each.view(np.uint32) == plain.view(np.uint32)).all()
    assert meta == meta0 == meta1


def test_the_tensor_does_not_depend_on_the_chunks(corpus):
    files, floats = corpus["files"], corpus["floats"]
    C, T, rate = 2, 12000, 16000
    ff = [(11 * i) % 500 for i in range(len(files))]
    plain, _ = decode(files, C, T, rate, ff)
    L = afgpu.lib()
    assert L.afg_dev_option(b"stage_chunk_samples", 1000) == 0
    try:
        got, meta = decode(files, C, T, rate, ff)
    finally:
        assert L.afg_dev_option(b"stage_chunk_samples", -1) == 0
    assert (got.view(np.uint32) == plain.view(np.uint32)).all()
    same(got, rm.tensor(floats, C, T, rate, ff, taps_of=taps_for(corpus, rate)))
    assert max(f["frames"] * f["channels"] for f in floats if f["status"] == 0) > 4 * 4096       # files did span chunks


def test_max_in_rate_refuses_and_admits_the_96_khz_file(corpus):
    files, floats, at = corpus["files"], corpus["floats"], corpus["at"]
    k = at["r96000"]
    C, T, rate = 2, 3000, 16000
    part = [files[k - 1], files[k], files[k + 1]]
    got, meta = decode(part, C, T, rate)
    assert meta[1]["status"] == -5 and "96000" in meta[1]["message"] and "48000" in meta[1]["message"]
    assert (got[1].view(np.uint32) == 0).all() and meta[0]["status"] == meta[2]["status"] == 0
    want = rm.tensor(floats[k - 1:k + 2], C, T, rate, taps_of=taps_for(corpus, rate))
    same(got, want)
    assert np.abs(got[0]).max() > 0.01 and np.nanmax(np.abs(got[2])) > 0.01
    admitted, meta = decode(part, C, T, rate, max_in_rate=96000)
    assert [m["status"] for m in meta] == [0, 0, 0]
    same(admitted, rm.tensor(floats[k - 1:k + 2], C, T, rate, max_in_rate=96000, taps_of=taps_for(corpus, rate)))
    assert np.abs(admitted[1]).max() > 0.01 and (admitted[0].view(np.uint32) == got[0].view(np.uint32)).all()


def test_in_channels_refuses_and_admits_the_70_channel_file(corpus):
    files, floats, at = corpus["files"], corpus["floats"], corpus["at"]
    k = at["wide"]
    T, rate = 300, 48000
    part = [files[0], files[k], files[k - 1]]
    fl = [floats[0], floats[k], floats[k - 1]]
    got, meta = decode(part, 1, T, rate, mono=True)
    assert meta[1]["status"] == -5 and "70" in meta[1]["message"] and "2" in meta[1]["message"]
    assert (got[1].view(np.uint32) == 0).all() and meta[0]["status"] == meta[2]["status"] == 0
    same(got, rm.tensor(fl, 1, T, rate, mono=True, taps_of=taps_for(corpus, rate)))
    got, meta = decode(part, 1, T, rate, mono=True, in_channels=WIDE_CHANNELS)
    assert [m["status"] for m in meta] == [0, 0, 0]
    same(got, rm.tensor(fl, 1, T, rate, mono=True, in_channels=WIDE_CHANNELS, taps_of=taps_for(corpus, rate)))
    mean = rm.mix(np.ascontiguousarray(floats[k]["pcm"].T))                     # 48 kHz to 48 kHz: the mean of the 70 rows as it is
    assert (got[1, 0, :WIDE_FRAMES].view(np.uint32) == mean.view(np.uint32)).all() and (got[1, 0, WIDE_FRAMES:] == 0).all()


def test_a_new_tensor_is_made_on_the_current_device(corpus):
    files, floats = corpus["files"], corpus["floats"]
    got, meta = afgpu.batch_decode_tensor_resampled(files[:3], 700, 2, 16000)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3, 2, 700) and got.is_contiguous()
    torch.cuda.synchronize()
    same(got.cpu().numpy(), rm.tensor(floats[:3], 2, 700, 16000, taps_of=taps_for(corpus, 16000)))
    empty, meta = afgpu.batch_decode_tensor_resampled([], 700, 2, 16000)
    assert tuple(empty.shape) == (0, 2, 700) and empty.is_cuda and meta == []
    for out in (torch.empty((3, 2, 700), dtype=torch.float64, device="cuda"), torch.empty((3, 2, 701), device="cuda"), torch.empty((3, 2, 700))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_resampled(files[:3], 700, 2, 16000, out=out)
