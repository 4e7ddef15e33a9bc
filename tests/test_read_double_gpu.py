"""AudioStream.readSamplesDouble (afg_read_samples_double) for every format, compared as uint64.

WAV against tests/f64_model.py (the double quotient itself, all 32 bits of s32, f64 as stored); FLAC against the
oracle's int32 decode times 1.0 / 2147483647; QOA, MP3, Ogg Vorbis, Ogg Opus, MOD and XM against the FLOAT read of a
second handle on the same bytes, widened with astype(float64) -- the reference's own definition for those formats
(stream.d:732-739), with the float read being what the existing suites pin; it is not a comparison with the double path.

The batch path (afg_batch_opts.sample_type = AFG_SAMPLE_F64) against the stream result, file by file.

On the commit before float64 reads every test here fails: the library has no afg_read_samples_double."""
import ctypes as C
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
import wav_model as M
import xm_bitstream as xb
from test_flac_frontend import make_pcm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAN64 = np.uint64(0x7FF8ABCDEF012345)                                # what an output double the read did not write holds


def open_stream(data):
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    assert not s.isError(), s.errorMessage()
    return s


def u64(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def read_double(s, frames):
    """one double read: the samples it returned; whatever lies behind them in the buffer must be untouched"""
    ch = s.getNumChannels()
    buf = np.full(frames * ch, NAN64, np.uint64).view(np.float64)
    n = s.readSamplesDouble(buf)
    assert 0 <= n <= frames
    assert (buf.view(np.uint64)[n * ch:] == NAN64).all(), "the read wrote behind the frames it returned"
    return buf[:n * ch].copy()


def read_float(s, frames):
    ch = s.getNumChannels()
    buf = np.full(frames * ch, np.nan, np.float32)
    n = s.readSamplesFloat(buf)
    return buf[:n * ch].copy()


def read_all(s, chunk, read):
    parts = []
    while True:
        part = read(s, chunk)
        if part.size == 0:
            break
        parts.append(part)
    return np.concatenate(parts) if parts else np.zeros(0)


# ---- WAV ----------------------------------------------------------------------------------------------------------

def wav_cases():
    rng = np.random.default_rng(60)
    for kind in range(6):
        for ch in (1, 3):
            frames = 2300 + 17 * kind + ch
            raw = wb.random_samples(rng, kind, frames * ch)
            yield kind, ch, frames, raw, wb.wav_file(kind, ch, 44100, raw, before=[wb.chunk(b"LIST", b"abc")] if kind % 2 else ())


@pytest.mark.parametrize("read", [10 ** 6, 1, 7, 1000])
def test_wav_reads(gpu, read):
    for kind, ch, frames, raw, data in wav_cases():
        want = fm.convert(raw, kind)
        s = open_stream(data)
        assert s.getFormat() == afgpu.FORMAT_WAV and s.getLengthInFrames() == frames
        at = 0
        while True:
            got = read_double(s, read)
            n = got.size // ch
            assert n == min(read, frames - at) and s.tellPosition() == at + n and not s.isError()
            if n == 0:
                break
            assert (u64(got) == u64(want[at * ch:(at + n) * ch])).all(), (fm.KIND_NAMES[kind], ch, at)
            at += n
        assert at == frames


def test_wav_seek_and_read(gpu):
    for kind, ch, frames, raw, data in wav_cases():
        want = fm.convert(raw, kind)
        s = open_stream(data)
        for frame in (frames // 2, 0, frames - 1, frames, 17, frames // 3):
            assert s.seekPosition(frame) and s.tellPosition() == frame
            got = read_double(s, 100)
            n = min(100, frames - frame)
            assert got.size == n * ch and s.tellPosition() == frame + n
            assert (u64(got) == u64(want[frame * ch:(frame + n) * ch])).all(), (fm.KIND_NAMES[kind], ch, frame)
        assert not s.seekPosition(frames + 1) and not s.isError()


def test_wav_data_chunk_cut_short(gpu):
    """wav.d:253: the failing read returns 0, the stream is in error state, and the position has moved all the same."""
    rng = np.random.default_rng(61)
    for kind in range(6):
        ch, frames = 2, 1500
        raw = wb.random_samples(rng, kind, frames * ch)
        whole = wb.wav_file(kind, ch, 44100, raw)
        data = whole[:len(whole) - (len(raw) // 2 + 1)]
        model = M.WavDecoder(data)
        s = open_stream(data)
        assert s.getLengthInFrames() == frames
        want = fm.convert(raw, kind)
        while True:
            at = model.tell()
            got = read_double(s, 300)
            wn, _, failed = model.read(300)
            assert got.size == wn * ch and s.isError() == failed and s.tellPosition() == model.tell()
            if failed:
                assert wn == 0 and model.tell() == at + 300 and s.errorMessage() == M.DECODING_ERROR
                assert read_double(s, 4).size == 0 and s.tellPosition() == model.tell()
                break
            assert (u64(got) == u64(want[at * ch:(at + wn) * ch])).all()


# ---- FLAC ---------------------------------------------------------------------------------------------------------

def flac_file(channels, bps, n=3000, block=576, seed=7):
    pcm = make_pcm(n, channels, bps, seed)
    data, _ = fb.encode_file(pcm, bps, block, sample_rate=48000,
                             assignments=(enc.INDEPENDENT, enc.LEFT_SIDE, enc.MID_SIDE) if channels == 2 else (enc.INDEPENDENT,))
    info, frames, subframes, res = afgpu.flac_parse(data)
    i32 = oraclelib.flac_transform(frames, subframes, res, info["out_samples"])
    assert i32.dtype == np.int32 and i32.size == n * channels
    return data, fm.flac_doubles(i32)


@pytest.mark.parametrize("channels,bps", [(2, 16), (2, 24), (3, 16), (3, 24)])
def test_flac_reads(gpu, channels, bps):
    n = 576 * 20 + 100                                       # more than one decode chunk of 16 frames
    data, want = flac_file(channels, bps, n=n)
    s = open_stream(data)
    assert s.getFormat() == afgpu.FORMAT_FLAC and s.getLengthInFrames() == n
    got = read_all(s, 1000, read_double)
    assert got.size == want.size and (u64(got) == u64(want)).all()
    if bps == 24:                                            # float32 cannot hold these: the double read is not the float read widened
        assert (got.astype(np.float32).astype(np.float64) != got).any()
    assert read_double(s, 4).size == 0 and not s.isError()   # stream.d:705
    assert s.seekPosition(777) and (u64(read_double(s, 50)) == u64(want[777 * channels:827 * channels])).all()


def test_flac_declared_length_zero_reads_nothing(gpu):
    pcm = make_pcm(512, 2, 16, 4)
    frames, subframes, res, _ = enc.encode(pcm, 16, 256)
    data = fb.write_file(frames, subframes, res, 44100, 16, total_samples=0)
    s = open_stream(data)
    assert s.getLengthInFrames() == 0
    assert read_double(s, 32).size == 0 and not s.isError()


# ---- the float decoders: the double read is the float read, widened -----------------------------------------------------

def float_codec_files():
    rng = np.random.default_rng(62)
    pcm = np.stack([9000 * np.sin(0.02 * (c + 1) * np.arange(6000)) + 300 * rng.standard_normal(6000) for c in range(2)], 1)
    qoa, _ = oraclelib.qoa_encode(pcm.round().astype(np.int16), 32000)
    return {
        "qoa": qoa.tobytes(),
        "mp3": m3.make_file(4242, n_frames=12)[0],
        "mp3_file": open(os.path.join(GOLDEN, "mathjax_invalid_keypress.mp3"), "rb").read(),
        "ogg": vb.make_file(931, channels=2, bs=(256, 2048), n_packets=16),
        "opus": ob.random_celt_file(np.random.default_rng(63), 2, 80, preskip=100, comments=(b"R128_TRACK_GAIN=-19000",))[0],
        "mod": mb.random_song(np.random.default_rng(64), channels=4, n_patterns=2, max_sample=2000),
        "xm": xb.random_song(np.random.default_rng(65), channels=4, rows=16, n_patterns=2),
    }


def check_against_the_float_read(data, chunk, cap=40):
    """the same reads on two handles: the counts agree and the doubles are the floats widened (modules stop reads early at
    pattern ends, and never end: `cap` reads)"""
    sd, sf = open_stream(data), open_stream(data)
    total = 0
    for _ in range(cap):
        got, ref = read_double(sd, chunk), read_float(sf, chunk)
        assert got.size == ref.size and sd.tellPosition() == sf.tellPosition() and sd.isError() == sf.isError()
        assert (u64(got) == u64(fm.widen(ref))).all()
        total += got.size
        if got.size == 0:
            break
    assert total > 0
    return total


@pytest.mark.parametrize("name", ["qoa", "mp3", "mp3_file", "ogg", "opus", "mod", "xm"])
def test_float_codecs(gpu, name):
    check_against_the_float_read(float_codec_files()[name], 1531)


@pytest.mark.numeric_tolerance
@pytest.mark.parametrize("name", ["mp3_file", "opus"])
def test_float_codecs_in_the_default_numeric_mode(gpu, name):
    """AFG_NUMERIC_TOLERANCE changes the floats, not their widening"""
    assert afgpu.get_numeric_mode() == afgpu.NUMERIC_TOLERANCE
    check_against_the_float_read(float_codec_files()[name], 1531)


# ---- float and double reads mixed on one handle ----------------------------------------------------------------------

def mixed_case(name):
    if name == "wav_s24":
        raw = wb.random_samples(np.random.default_rng(66), fm.KIND_S24, 2 * 1000)
        return wb.wav_file(fm.KIND_S24, 2, 44100, raw)
    if name == "flac":
        return flac_file(2, 24, n=576 * 20)[0]                # the reads below cross a decode chunk's end (16 frames)
    return float_codec_files()["mp3_file"]


@pytest.mark.parametrize("name", ["wav_s24", "flac", "mp3"])
@pytest.mark.parametrize("start", [0, 9150])
def test_mixed_reads_on_one_handle(gpu, name, start):
    """float 100 frames, double 100, float 100: each piece is what a handle that only ever used that type returns there"""
    data = mixed_case(name)
    if name == "wav_s24":
        start = start and 650
    ch = open_stream(data).getNumChannels()
    only_f, only_d, mixed = open_stream(data), open_stream(data), open_stream(data)
    if start:                                                 # decode ahead first: the change of type then has a FIFO to drop
        for s, rd in ((only_f, read_float), (only_d, read_double), (mixed, read_float)):
            assert rd(s, start).size == start * ch
    want_f = [read_float(only_f, 100) for _ in range(3)]
    want_d = [read_double(only_d, 100) for _ in range(3)]
    assert all(w.size == 100 * ch for w in want_f + want_d)
    a, b, c = read_float(mixed, 100), read_double(mixed, 100), read_float(mixed, 100)
    assert mixed.tellPosition() == start + 300 and not mixed.isError()
    assert (a.view(np.uint32) == want_f[0].view(np.uint32)).all()
    assert (u64(b) == u64(want_d[1])).all()
    assert (c.view(np.uint32) == want_f[2].view(np.uint32)).all()


# ---- handles that do not read ------------------------------------------------------------------------------------------

def test_a_writing_handle_reads_nothing(gpu):
    s = afgpu.AudioStream()
    s.openToBuffer(afgpu.FORMAT_WAV, 44100.0, 2)
    assert s.isOpenForWriting() and not s.isError()
    buf = np.full(16, NAN64, np.uint64).view(np.float64)
    assert afgpu.lib().afg_read_samples_double(s._h, buf.ctypes.data, 8) == 0
    assert (buf.view(np.uint64) == NAN64).all()
    s.cleanUp()


def test_null_out_skips_frames_and_bad_counts_read_nothing(gpu):
    kind, ch, frames, raw, data = next(wav_cases())
    want = fm.convert(raw, kind)
    L = afgpu.lib()
    for blob, w in ((data, want), (flac_file(2, 16, n=2000)[0], None)):
        s = open_stream(blob)
        c = s.getNumChannels()
        assert L.afg_read_samples_double(s._h, None, 0) == 0 and L.afg_read_samples_double(s._h, None, -5) == 0
        assert L.afg_read_samples_double(s._h, None, 123) == 123 and s.tellPosition() == 123
        got = read_double(s, 10)
        ref = open_stream(blob)
        assert ref.seekPosition(123)
        assert (u64(got) == u64(read_double(ref, 10))).all() and got.size == 10 * c
        if w is not None:
            assert (u64(got) == u64(w[123 * c:133 * c])).all()


# ---- the batch path: afg_batch_opts.sample_type --------------------------------------------------------------------------

def batch_files():
    """one file of every format"""
    rng = np.random.default_rng(67)
    f = float_codec_files()
    wav = wb.wav_file(fm.KIND_S24, 3, 44100, wb.random_samples(rng, fm.KIND_S24, 3 * 2501))
    wav64 = wb.wav_file(fm.KIND_F64, 1, 8000, wb.random_samples(rng, fm.KIND_F64, 777))
    return [f["mp3_file"], flac_file(2, 24, n=576 * 20 + 100)[0], wav, f["qoa"], f["ogg"], f["opus"], f["mod"], f["xm"], wav64, f["mp3"],
            flac_file(3, 16, n=4000)[0]]


def stream_doubles(data, frames):
    """the stream's double reads of the first `frames` frames (modules: reads stop at pattern ends, so read until there)"""
    s = open_stream(data)
    parts, got = [], 0
    while got < frames:
        part = read_double(s, min(frames - got, 1 << 16))
        if part.size == 0:
            break
        parts.append(part)
        got += part.size // s.getNumChannels()
    return np.concatenate(parts) if parts else np.zeros(0)


def check_batch_against_streams(files, out):
    assert len(out) == len(files)
    for k, (data, item) in enumerate(zip(files, out)):
        assert item["status"] == 0, (k, item["message"])
        assert item["pcm"].dtype == np.float64 and item["pcm"].shape == (item["frames"], item["channels"])
        want = stream_doubles(data, item["frames"])
        assert want.size == item["pcm"].size and (u64(item["pcm"]) == u64(want)).all(), (k, afgpu.FORMAT_NAMES[item["format"]])


def test_batch_of_every_format(gpu):
    files = batch_files()
    out = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    assert sorted({o["format"] for o in out}) == list(range(8))                  # WAV, MP3, FLAC, OGG, OPUS, QOA, MOD, XM
    check_batch_against_streams(files, out)
    # the float call on the same files is the double call narrowed, except where float32 cannot hold the doubles
    flt = afgpu.batch_decode(files, n_threads=4)
    for d, f in zip(out, flt):
        assert f["pcm"].dtype == np.float32 and f["frames"] == d["frames"]
        if d["format"] not in (afgpu.FORMAT_WAV, afgpu.FORMAT_FLAC):
            assert (u64(fm.widen(f["pcm"])) == u64(d["pcm"])).all()


def test_batch_on_two_devices_gives_the_same_doubles(gpu):
    if afgpu.device_count() < 2:
        pytest.skip("one device visible")
    files = batch_files()
    one = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    two = afgpu.batch_decode(files, n_threads=4, devices=[0, 1], dtype=np.float64)
    for a, b in zip(one, two):
        assert a["status"] == b["status"] == 0 and (u64(a["pcm"]) == u64(b["pcm"])).all()


def test_batch_split_over_a_device_named_twice_gives_the_same_doubles(gpu):
    """the multi-device split (files sharded over per-device host threads) on whatever is there: device 0 twice"""
    files = batch_files()
    one = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    two = afgpu.batch_decode(files, n_threads=4, devices=[0, 0], dtype=np.float64)
    for a, b in zip(one, two):
        assert a["status"] == b["status"] == 0 and (u64(a["pcm"]) == u64(b["pcm"])).all()


def test_grouped_flac_batch_gives_the_same_doubles(gpu):
    files = [flac_file(1 + k % 3, (16, 24)[k % 2], n=3000 + 100 * k, seed=70 + k)[0] for k in range(8)]
    plain = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    check_batch_against_streams(files, plain)
    L = afgpu.lib()
    assert L.afg_dev_option(b"batch_groups", 3) == 0
    try:
        grouped = afgpu.batch_decode(files, n_threads=4, dtype=np.float64)
    finally:
        assert L.afg_dev_option(b"batch_groups", -1) == 0
    for a, b in zip(plain, grouped):
        assert a["status"] == b["status"] == 0 and a["frames"] == b["frames"] and (u64(a["pcm"]) == u64(b["pcm"])).all()


def raw_batch(files, opts):
    L = afgpu.lib()
    ptrs = (C.c_char_p * len(files))(*files)
    lens = (C.c_size_t * len(files))(*[len(f) for f in files])
    res = afgpu.BatchResult()
    rc = L.afg_batch_decode_ex(ptrs, lens, len(files), C.byref(opts), C.byref(res))
    return rc, res


def test_an_unknown_sample_type_is_refused(gpu):
    files = [flac_file(2, 16, n=1000)[0]]
    rc, res = raw_batch(files, afgpu.BatchOpts(C.sizeof(afgpu.BatchOpts), 0, 0, None, 7))
    assert rc == -1 and res.n_files == 0 and not res.items                       # AFG_ERR_INVALID, nothing decoded
    assert b"sample_type" in afgpu.lib().afg_last_error()


def test_a_struct_size_without_the_field_gets_floats(gpu):
    """a caller built before the field existed: whatever lies behind its struct is not read"""
    files = [flac_file(2, 24, n=2000)[0], float_codec_files()["qoa"]]
    want = afgpu.batch_decode(files)
    opts = afgpu.BatchOpts(afgpu.BATCH_OPTS_SIZE_V1, 0, 0, None, afgpu.SAMPLE_F64)
    assert afgpu.BATCH_OPTS_SIZE_V1 == 24 < C.sizeof(afgpu.BatchOpts)
    rc, res = raw_batch(files, opts)
    try:
        assert rc == 0 and res.n_files == 2
        for k in range(2):
            it = res.items[k]
            n = it.frames * it.channels
            got = np.ctypeslib.as_array(it.pcm, shape=(n,))
            assert (got.view(np.uint32) == want[k]["pcm"].reshape(-1).view(np.uint32)).all()
    finally:
        afgpu.lib().afg_batch_free(C.byref(res))
