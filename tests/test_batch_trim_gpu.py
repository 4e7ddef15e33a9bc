"""afgpu.batch_decode_tensor_trimmed (afg_batch_decode_trimmed) against afgpu.batch_decode_tensor_resampled at
frames = scan_frames put through tests/trim_model.py, bit for bit on the tensor, `begin` and `end`: one generated file of every
format, WAV and FLAC files at 8, 16 and 44.1 kHz with a second of digital silence at each end, a QOA file that is quiet, then
loud, a damaged file and one that is no audio, to 16 kHz, mono and two channels, whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as fm
import flac_bitstream as fb
import oraclelib
import trim_model as tm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T = 16000, 12000
IN_CHANNELS = 3                                                  # two of the generated files have three channels
TRIMS = {"60 dB": dict(top_db=60.0), "20 dB, margins": dict(top_db=20.0, frame_length=400, hop=200, lead=33, trail=70),
         "absolute": dict(top_db=45.0, reference="abs", abs_power=1.0, frame_length=64, hop=64)}


def padded(rate, channels, seconds, seed, quiet=0.0):
    """int16 [frames, channels]: a second of digital silence (or of a tone at `quiet` of full scale), `seconds` of a loud tone
    with noise, a second of silence"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n)
    body = np.stack([12000 * np.sin(0.05 * (c + 1) * t + c) + 500 * rng.standard_normal(n) for c in range(channels)], 1)
    lead = np.stack([quiet * 32767 * np.sin(0.05 * (c + 1) * np.arange(rate)) for c in range(channels)], 1)
    return np.concatenate([lead, body, np.zeros((rate, channels))]).round().astype(np.int16)


def silent_files():
    """(files, the indices of the WAV and FLAC ones)"""
    files = []
    for k, (rate, ch) in enumerate(((8000, 1), (16000, 2), (44100, 2), (44100, 1))):
        files.append(wb.wav_file(fm.KIND_S16, ch, rate, padded(rate, ch, 0.4, 80 + k).astype("<i2").tobytes()))
    for k, (rate, ch) in enumerate(((8000, 2), (16000, 1), (44100, 1))):
        files.append(fb.encode_file(padded(rate, ch, 0.3, 90 + k).astype(np.int64), 16, 1152, sample_rate=rate)[0])
    lossless = list(range(len(files)))
    files.append(oraclelib.qoa_encode(padded(16000, 2, 0.5, 99, quiet=0.01), 16000)[0].tobytes())      # quiet, then loud
    return files, lossless


def groups_of(meta, C, mono, scan, frames, first_frame):
    """one group per file, as include/afg.h describes them, with valid computed here from what the call reported"""
    g = np.zeros(len(meta), tm.GROUP_DTYPE)
    for i, m in enumerate(meta):
        g[i]["in_off"], g[i]["out_off"] = i * C * scan, i * C * frames
        g[i]["in_stride"], g[i]["out_stride"], g[i]["rows"], g[i]["out_rows"], g[i]["out_frames"] = scan, frames, 1, C, frames
        if m["status"] == 0:
            g[i]["rows"] = 1 if mono else min(C, m["channels"])
            g[i]["valid"] = tm_valid(m["frames"], first_frame[i] if first_frame else 0, round(m["samplerate"]), RATE, scan)
    return g


def tm_valid(frames, first_frame, in_rate, out_rate, T_):
    from math import gcd
    g = gcd(int(in_rate), int(out_rate))
    M, L = int(in_rate) // g, int(out_rate) // g
    d = int(frames) - int(first_frame)
    return 0 if d <= 0 else min(int(T_), -(-d * L // M))


@pytest.fixture(scope="module")
def corpus(gpu):
    files, lossless = silent_files()
    every = build_files()                                        # one file per format: all eight
    at = {"lossless": lossless, "qoa": len(files) - 1, "formats": len(files)}
    files += every
    at["damaged"], at["junk"] = len(files), len(files) + 1
    files.append(every[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    first = [0] * len(files)
    first[lossless[2]] = 4410                                    # a tenth of a second into the file
    return {"files": files, "at": at, "first": first, "ref": {}}


def reference(corpus, mono, scan):
    """the library's own tensor at frames = scan, made once"""
    key = (mono, scan)
    if key not in corpus["ref"]:
        C = 1 if mono else 2
        with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
            mp.setenv("AFG_NUMERIC", "exact")
            tensor, meta = afgpu.batch_decode_tensor_resampled(corpus["files"], scan, C, RATE, first_frame=corpus["first"], mono=mono,
                                                               in_channels=IN_CHANNELS, n_threads=4)
            torch.cuda.synchronize()
        plane = tensor.cpu().numpy().reshape(-1)
        plane.setflags(write=False)
        corpus["ref"][key] = (plane, meta, C)
    return corpus["ref"][key]


def model(corpus, mono, scan, name):
    key = (mono, scan, name)
    if key not in corpus["ref"]:
        plane, meta, C = reference(corpus, mono, scan)
        kw = dict(TRIMS[name])
        kw["reference"] = tm.REF_ABS if kw.get("reference") == "abs" else tm.REF_MAX
        g = groups_of(meta, C, mono, scan, T, corpus["first"])
        out, regions, _ = tm.trim(plane, np.full(len(meta) * C * T, np.nan, np.float32), g, tm.params(**kw))
        corpus["ref"][key] = (out, regions, g)
    return corpus["ref"][key]


def decode(corpus, mono, scan, name, scan_arg="given", **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    C = 1 if mono else 2
    out = torch.full((len(corpus["files"]), C, T), float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_tensor_trimmed(corpus["files"], T, C, RATE, scan_frames=None if scan_arg is None else scan, first_frame=corpus["first"],
                                                  mono=mono, in_channels=IN_CHANNELS, out=out, n_threads=4, **TRIMS[name], **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


def same(corpus, mono, scan, name, got, meta):
    want, regions, g = model(corpus, mono, scan, name)
    bad = tm.same_bits(got.reshape(-1), want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    assert [m["begin"] for m in meta] == regions["begin"].tolist() and [m["end"] for m in meta] == regions["end"].tolist()
    plain = [{k: v for k, v in m.items() if k not in ("begin", "end")} for m in meta]
    assert plain == reference(corpus, mono, scan)[1]
    return regions, g


@pytest.mark.parametrize("mono", [True, False], ids=["mono", "two-channels"])
@pytest.mark.parametrize("scan", [T, 4 * T], ids=["scan=frames", "scan=4 frames"])
@pytest.mark.parametrize("name", list(TRIMS))
def test_the_tensor_is_the_resampled_one_through_the_model(corpus, mono, scan, name):
    got, meta = decode(corpus, mono, scan, name, scan_arg=None if scan == T else "given")
    regions, g = same(corpus, mono, scan, name, got, meta)
    at = corpus["at"]
    assert sorted({m["format"] for m in meta[at["formats"]:at["damaged"]]}) == list(range(8))      # WAV, MP3, FLAC, OGG, OPUS, QOA, MOD, XM
    assert {8000, 16000, 44100} <= {int(m["samplerate"]) for m in meta if m["status"] == 0}
    for bad in (at["damaged"], at["junk"]):                      # a zero slab, region (0, 0), the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
        assert (meta[bad]["begin"], meta[bad]["end"]) == (0, 0)
    if name == "60 dB" and scan == 4 * T:
        for i in at["lossless"]:                                 # the test cannot pass on untrimmed files
            assert 0 < meta[i]["begin"] < meta[i]["end"] < g[i]["valid"], (i, meta[i], g[i]["valid"])
            assert np.abs(got[i, 0, :2048]).max() > 0.01       # the frame that finds the onset reaches half its length ahead of it
    if name == "20 dB, margins" and scan == 4 * T:
        i = at["qoa"]                                            # the quiet second is cut, the margin kept
        assert RATE - 600 < meta[i]["begin"] < RATE and meta[i]["end"] < g[i]["valid"]
    if scan == 4 * T:
        assert len([i for i, m in enumerate(meta) if m["begin"] > 0]) >= 8


def test_the_result_does_not_depend_on_the_sublists(corpus):
    L = afgpu.lib()
    scan, name = 4 * T, "60 dB"
    try:
        for value in (1, 3 * 2 * scan * 4 + 8):                  # every file its own sublist; three files
            assert L.afg_dev_option(b"trim_scratch_bytes", value) == 0
            got, meta = decode(corpus, False, scan, name)
            same(corpus, False, scan, name, got, meta)
    finally:
        assert L.afg_dev_option(b"trim_scratch_bytes", -1) == 0


def test_regions_may_be_null_and_out_is_reused(corpus):
    import ctypes as C
    files = corpus["files"][:3]
    n, scan = len(files), 4 * T
    out = torch.full((n, 1, T), float("nan"), dtype=torch.float32, device="cuda")
    ptrs = (C.c_char_p * n)(*files)
    lens = (C.c_size_t * n)(*[len(f) for f in files])
    opts = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 4, 1, T, None, RATE, 1, IN_CHANNELS, 0, 0)
    prm = afgpu.trim_params()
    res = afgpu.BatchResult()
    afgpu.check(afgpu.lib().afg_batch_decode_trimmed(ptrs, lens, n, C.byref(opts), C.byref(prm), scan, out.data_ptr(), None, C.byref(res)))
    try:
        assert res.n_files == n and all(res.items[i].status == 0 for i in range(n))
        slab = C.cast(res.items[1].pcm, C.c_void_p).value
        assert slab == out.data_ptr() + 1 * T * 4                # items[i].pcm is the file's slab of the caller's tensor
    finally:
        afgpu.lib().afg_batch_free(C.byref(res))
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    again, meta = afgpu.batch_decode_tensor_trimmed(files, T, 1, RATE, scan_frames=scan, mono=True, in_channels=IN_CHANNELS, out=out, n_threads=4)
    assert again is out
    torch.cuda.synchronize()
    assert tm.same_bits(again.cpu().numpy(), first).size == 0 and not np.isnan(first).any() and all(m["begin"] > 0 for m in meta)


def test_python_refusals_and_empty_lists(corpus):
    part = corpus["files"][:3]
    for out in (torch.empty((3, 1, T), dtype=torch.float64, device="cuda"), torch.empty((3, 1, T + 1), device="cuda"), torch.empty((3, 1, T))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_trimmed(part, T, 1, RATE, mono=True, out=out)
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor_trimmed(part, T, 1, RATE, scan_frames=T - 1)
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor_trimmed(part, T, 1, RATE, first_frame=[0])
    empty, meta = afgpu.batch_decode_tensor_trimmed([], T, 2, RATE, scan_frames=2 * T)
    assert tuple(empty.shape) == (0, 2, T) and empty.is_cuda and meta == []
