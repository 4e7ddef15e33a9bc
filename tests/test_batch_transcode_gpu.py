"""Batch decode to packed PCM (afg_batch_opts.sample_type AFG_SAMPLE_PCM_*) and afg_batch_transcode on one file of every
format: the bytes are the host writer's (afgpu.wav_encode, with the 31-bit generator as its callback for dither) over the
floats the float call returns for the same file -- clamped to [-1, 1], NaN to 0, by the test itself -- and they depend on
nothing but the file: not on its neighbours, the devices, or how the stages cut their work into chunks."""
import os

import numpy as np
import pytest

import afgpu
import f64_model as fm
import flac_bitstream as fb
import flac_ref_encoder as enc
import mod_bitstream as mb
import mp3_bitstream as m3
import opus_bitstream as ob
import oraclelib
import vorbis_bitstream as vb
import wav_bitstream as wb
import xm_bitstream as xb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
A, INC, M = 1103515245, 12345, 1 << 31
SEED = 0x1234567
PCM = [(afgpu.SAMPLE_PCM_S8, afgpu.WAV_S8), (afgpu.SAMPLE_PCM_S16, afgpu.WAV_S16LE), (afgpu.SAMPLE_PCM_S24, afgpu.WAV_S24LE)]
CASES = [(st, wf, d) for st, wf in PCM for d in (afgpu.DITHER_OFF, afgpu.DITHER_LCG31)]
IDS = [f"{'s8 s16 s24'.split()[wf]}-{'off' if d == afgpu.DITHER_OFF else 'lcg31'}" for _, wf, d in CASES]


def lcg(seed):
    state = [seed % M]

    def rng():
        state[0] = (state[0] * A + INC) % M
        return state[0]
    return rng


def make_pcm(n, channels, bps, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    amp = (1 << (bps - 1)) * 0.4
    cols = []
    for c in range(channels):
        x = amp * np.sin(0.01 * (c + 1) * t + c) + amp * 0.05 * rng.standard_normal(n)
        cols.append(np.clip(np.round(x), -(1 << (bps - 1)), (1 << (bps - 1)) - 1))
    return np.stack(cols, 1).astype(np.int64)


def flac_file(channels, bps, n, block=576, seed=7):
    data, _ = fb.encode_file(make_pcm(n, channels, bps, seed), bps, block, sample_rate=48000,
                             assignments=(enc.INDEPENDENT, enc.LEFT_SIDE, enc.MID_SIDE) if channels == 2 else (enc.INDEPENDENT,))
    return data


def float_wav(samples, channels=2, rate=22050):
    """a float32 WAV file holding `samples` as they are"""
    return afgpu.wav_encode(np.asarray(samples, np.float32).reshape(-1, channels), rate, afgpu.WAV_FP32LE)


def build_files():
    """one file of every format (the set of the float64 batch test), and a float WAV whose samples leave [-1, 1]"""
    rng = np.random.default_rng(67)
    r62 = np.random.default_rng(62)
    pcm = np.stack([9000 * np.sin(0.02 * (c + 1) * np.arange(6000)) + 300 * r62.standard_normal(6000) for c in range(2)], 1)
    qoa, _ = oraclelib.qoa_encode(pcm.round().astype(np.int16), 32000)
    wav = wb.wav_file(fm.KIND_S24, 3, 44100, wb.random_samples(rng, fm.KIND_S24, 3 * 2501))
    wav64 = wb.wav_file(fm.KIND_F64, 1, 8000, wb.random_samples(rng, fm.KIND_F64, 777))
    loud = float_wav(np.resize(np.array([2, -2, 0.25, 1.5, -1.0000001, 1, -0.75, np.nan], np.float32), 2 * 1501))
    return [open(os.path.join(GOLDEN, "mathjax_invalid_keypress.mp3"), "rb").read(), flac_file(2, 24, 576 * 20 + 100), wav, qoa.tobytes(),
            vb.make_file(931, channels=2, bs=(256, 2048), n_packets=16),
            ob.random_celt_file(np.random.default_rng(63), 2, 80, preskip=100, comments=(b"R128_TRACK_GAIN=-19000",))[0],
            mb.random_song(np.random.default_rng(64), channels=4, n_patterns=2, max_sample=2000),
            xb.random_song(np.random.default_rng(65), channels=4, rows=16, n_patterns=2), wav64, m3.make_file(4242, n_frames=12)[0],
            flac_file(3, 16, 4000), loud]


LOUD = 11           # index of the file built to leave the range
GENERATED_FLOAT_CODECS = (4, 5, 9)      # the generated Vorbis, Opus and MP3 files


@pytest.fixture(scope="module")
def corpus(gpu):
    """the files, what the float call returns for them, and (filled in as the tests ask) the expected WAV files"""
    files = build_files()
    with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        floats = afgpu.batch_decode(files, n_threads=4)
    assert all(f["status"] == 0 for f in floats), [f["message"] for f in floats]
    assert sorted({f["format"] for f in floats}) == list(range(8))               # WAV, MP3, FLAC, OGG, OPUS, QOA, MOD, XM
    return {"files": files, "floats": floats, "want": {}}


def clamp(x):
    return np.clip(np.where(np.isnan(x), np.float32(0), x), -1, 1).astype(np.float32)


def want_wav(corpus, k, wav_format, dither):
    """the host writer's file over the float call's output for file k (computed once per case)"""
    key = (k, wav_format, dither)
    if key not in corpus["want"]:
        f = corpus["floats"][k]
        x, rate = f["pcm"], int(np.float32(f["samplerate"]) + np.float32(0.5))
        if wav_format <= afgpu.WAV_S24LE:
            x = clamp(x)
        if dither == afgpu.DITHER_LCG31 and wav_format <= afgpu.WAV_S24LE:
            corpus["want"][key] = afgpu.wav_encode(x, rate, wav_format, dither=lcg(SEED), rng_max=0x7fffffff)
        else:
            corpus["want"][key] = afgpu.wav_encode(x, rate, wav_format)
    return corpus["want"][key]


def body_of(item):
    return item["pcm"].reshape(-1).view(np.uint8).tobytes()


def check_bodies(corpus, out, wav_format, dither, order=None):
    order = range(len(out)) if order is None else order
    for item, k in zip(out, order):
        f = corpus["floats"][k]
        assert item["status"] == 0 and item["frames"] == f["frames"] and item["channels"] == f["channels"], (k, item["message"])
        assert body_of(item) == want_wav(corpus, k, wav_format, dither)[44:], (k, afgpu.FORMAT_NAMES[f["format"]])


def test_the_generated_float_codec_files_stay_in_range(corpus):
    """only the file built to do so exercises the clamp (a decoder's overshoot would be covered by the clamp all the same)"""
    for k, f in enumerate(corpus["floats"]):
        x = f["pcm"]
        if k == LOUD:
            assert np.isnan(x).any() and (np.abs(x[~np.isnan(x)]) > 1).any()
        elif k in GENERATED_FLOAT_CODECS:
            print(k, afgpu.FORMAT_NAMES[f["format"]], "peak", float(np.abs(x).max()))
            assert np.isfinite(x).all() and np.abs(x).max() <= 1


@pytest.mark.parametrize("sample_type,wav_format,dither", CASES, ids=IDS)
def test_bodies_and_transcodes_are_the_host_writers_bytes(corpus, sample_type, wav_format, dither):
    files = corpus["files"]
    out = afgpu.batch_decode(files, n_threads=4, sample_type=sample_type, dither=dither, dither_seed=SEED)
    dt, shape = {afgpu.WAV_S8: (np.uint8, ()), afgpu.WAV_S16LE: (np.int16, ()), afgpu.WAV_S24LE: (np.uint8, (3,))}[wav_format]
    for item in out:
        assert item["pcm"].dtype == dt and item["pcm"].shape == (item["frames"], item["channels"]) + shape
    check_bodies(corpus, out, wav_format, dither)
    got = afgpu.batch_transcode(files, afgpu.encoding_options(wav_format, dither, SEED), n_threads=4)
    for k, item in enumerate(got):
        assert item["status"] == 0 and item["bytes"] == want_wav(corpus, k, wav_format, dither), k
    if dither == afgpu.DITHER_LCG31:                                             # (dither does something)
        assert any(want_wav(corpus, k, wav_format, dither) != want_wav(corpus, k, wav_format, afgpu.DITHER_OFF) for k in range(len(files)))


@pytest.mark.parametrize("wav_format", [afgpu.WAV_FP32LE, afgpu.WAV_FP64LE], ids=["fp32", "fp64"])
def test_float_transcodes(corpus, wav_format):
    files = corpus["files"]
    got = afgpu.batch_transcode(files, afgpu.encoding_options(wav_format, afgpu.DITHER_LCG31, SEED), n_threads=4)
    if wav_format == afgpu.WAV_FP64LE:                                           # the doubles of the double call, as they are
        wide = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    for k, item in enumerate(got):
        f = corpus["floats"][k]
        assert item["status"] == 0
        if wav_format == afgpu.WAV_FP32LE:
            assert item["bytes"] == want_wav(corpus, k, wav_format, afgpu.DITHER_OFF), k
        else:
            head = want_wav(corpus, k, wav_format, afgpu.DITHER_OFF)[:44]
            assert item["bytes"] == head + wide[k]["pcm"].tobytes(), k
        assert len(item["bytes"]) == 44 + f["frames"] * f["channels"] * (4 if wav_format == afgpu.WAV_FP32LE else 8)
    # no options: fp32
    assert [g["bytes"] for g in afgpu.batch_transcode(files[:3])] == [want_wav(corpus, k, afgpu.WAV_FP32LE, 0) for k in range(3)]


def test_transcoded_files_reopen(corpus):
    got = afgpu.batch_transcode(corpus["files"], afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF), n_threads=4)
    for k, item in enumerate(got):
        f = corpus["floats"][k]
        s = afgpu.AudioStream()
        s.openFromMemory(item["bytes"])
        assert not s.isError(), s.errorMessage()
        assert s.getFormat() == afgpu.FORMAT_WAV and s.getNumChannels() == f["channels"] and s.getLengthInFrames() == f["frames"]
        assert s.getSamplerate() == float(int(np.float32(f["samplerate"]) + np.float32(0.5)))
        s.cleanUp()


S16 = (afgpu.SAMPLE_PCM_S16, afgpu.WAV_S16LE, afgpu.DITHER_LCG31)


def decode_s16(files, **kw):
    return afgpu.batch_decode(files, n_threads=4, sample_type=S16[0], dither=S16[2], dither_seed=SEED, **kw)


def test_a_files_bytes_do_not_depend_on_its_neighbours(corpus):
    files = corpus["files"]
    n = len(files)
    back = list(range(n))[::-1]
    check_bodies(corpus, decode_s16([files[k] for k in back]), S16[1], S16[2], back)
    twice = list(range(n)) + [0, 4, 2, 9]                                         # second copies of an MP3, a Vorbis, a WAV file
    check_bodies(corpus, decode_s16([files[k] for k in twice]), S16[1], S16[2], twice)


def test_a_files_bytes_do_not_depend_on_the_devices(corpus):
    check_bodies(corpus, decode_s16(corpus["files"], devices=[0, 0]), S16[1], S16[2])
    got = afgpu.batch_transcode(corpus["files"], afgpu.encoding_options(afgpu.WAV_S24LE, afgpu.DITHER_LCG31, SEED), n_threads=4, devices=[0, 0])
    for k, item in enumerate(got):
        assert item["bytes"] == want_wav(corpus, k, afgpu.WAV_S24LE, afgpu.DITHER_LCG31), k


@pytest.mark.parametrize("option,value", [("batch_groups", 3), ("mp3_chunks", 5), ("stage_chunk_samples", 4096), ("stage_chunk_samples", 1500)])
def test_a_files_bytes_do_not_depend_on_the_chunks(corpus, option, value):
    """every dev option that makes a stage cut its work into several chunks; each file twice, so that every stage has
    several files to cut between"""
    files = corpus["files"]
    order = list(range(len(files))) * 2
    L = afgpu.lib()
    assert L.afg_dev_option(option.encode(), value) == 0
    try:
        out = decode_s16([files[k] for k in order])
        plain = afgpu.batch_decode([files[k] for k in order], n_threads=4)
    finally:
        assert L.afg_dev_option(option.encode(), -1) == 0
    check_bodies(corpus, out, S16[1], S16[2], order)
    for item, k in zip(plain, order):                                           # (the option leaves the float call as it was)
        assert (item["pcm"].view(np.uint32) == corpus["floats"][k]["pcm"].view(np.uint32)).all(), k
    for fmt, dither in ((afgpu.SAMPLE_PCM_S24, afgpu.DITHER_OFF),):
        assert L.afg_dev_option(option.encode(), value) == 0
        try:
            out = afgpu.batch_decode([files[k] for k in order], n_threads=4, sample_type=fmt, dither=dither)
        finally:
            assert L.afg_dev_option(option.encode(), -1) == 0
        check_bodies(corpus, out, afgpu.WAV_S24LE, dither, order)


def test_a_damaged_file_is_an_error_item(corpus):
    files = corpus["files"]
    damaged = files[2][:-100]                                                    # a WAV file whose data chunk is cut short
    junk = b"RIFF" + b"\x00" * 40
    batch = [files[0], damaged, files[1], junk, files[3], files[LOUD]]
    order = [0, None, 1, None, 3, LOUD]
    floats = afgpu.batch_decode(batch, n_threads=4)
    assert [i for i, f in enumerate(floats) if f["status"] != 0] == [1, 3], [(f["status"], f["message"]) for f in floats]
    got = afgpu.batch_transcode(batch, afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LCG31, SEED), n_threads=4)
    out = decode_s16(batch)
    for i, (item, body, k) in enumerate(zip(got, out, order)):
        if k is None:
            assert item["status"] == floats[i]["status"] != 0 and item["message"] == floats[i]["message"] and item["bytes"] is None
            assert body["status"] == floats[i]["status"] and body["pcm"] is None
        else:
            assert item["status"] == 0 and item["bytes"] == want_wav(corpus, k, afgpu.WAV_S16LE, afgpu.DITHER_LCG31), k
            assert body_of(body) == item["bytes"][44:]


def test_out_of_range_floats_are_clamped(corpus):
    f = corpus["floats"][LOUD]
    x = f["pcm"].reshape(-1)
    assert x[0] == 2 and x[1] == -2 and np.isnan(x[7])
    out = afgpu.batch_decode([corpus["files"][LOUD]], sample_type=afgpu.SAMPLE_PCM_S16)[0]
    got = out["pcm"].reshape(-1)
    assert list(got[:8]) == [32767, -32767, 8192, 32767, -32767, 32767, -24575, 0]
