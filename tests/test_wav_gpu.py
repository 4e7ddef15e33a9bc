"""WAV on the device: the sample conversion (afg_wav_convert_hip), the stream's reads / seek / tell, the writer's round trip,
the batch path and transcode.py, compared as uint32 with tests/wav_model.py (for f64 input a NaN only has to stay a NaN).

On the commit before WAV decoding every test here fails: afg_wav_convert_hip does not exist, and a WAV opens as
"Cannot decode stream: unrecognized encoding." (test_stream_*, test_round_trip_*, test_batch_*, test_transcode_*)."""
import os

import numpy as np
import pytest

import afgpu
import flac_bitstream as fb
import mod_bitstream as mb
import pocketmod_model as pm
import wav_bitstream as wb
import wav_model as M
from record_cases import RECORD_CASES, record_lengths
from test_flac_frontend import make_pcm
from test_stream_gpu import MP3_FIXTURE, flac_expected, qoa_file

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7FC0BEEF)                                    # what an output float nobody wrote holds


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def convert(gpu, spans):
    """spans: (kind, sample bytes, byte offset of the span in the input plane modulo 16, float offset modulo 4).  One launch;
    checks every span against the model and that no float outside the spans was written."""
    import torch
    recs = np.zeros(len(spans), afgpu.WAV_SPAN_DTYPE)
    in_at, out_at = 0, 0
    for k, (kind, raw, in_mis, out_mis) in enumerate(spans):
        assert len(raw) % afgpu.WAV_KIND_BYTES[kind] == 0
        in_at = (in_at + 15) // 16 * 16 + in_mis
        out_at = (out_at + 3) // 4 * 4 + out_mis
        recs[k] = (in_at, out_at, len(raw) // afgpu.WAV_KIND_BYTES[kind], 0, kind, 0)
        in_at += len(raw)
        out_at += int(recs[k]["count"])
    in_bytes, out_floats = (in_at + 15) // 16 * 16 + 16, (out_at + 3) // 4 * 4 + 4
    plane = np.zeros(in_bytes, np.uint8)
    for r, (_, raw, _, _) in zip(recs, spans):
        plane[int(r["in_off"]):int(r["in_off"]) + len(raw)] = np.frombuffer(raw, np.uint8)
    tiles = afgpu.wav_layout(recs)
    assert tiles == sum(-(-int(r["count"]) // afgpu.WAV_TILE_SAMPLES) for r in recs)
    d_in = torch.from_numpy(plane).to(gpu)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(gpu)
    d_out = torch.from_numpy(np.full(out_floats, SENTINEL, np.uint32).view(np.float32).copy()).to(gpu)
    afgpu.wav_convert(len(recs), d_recs, tiles, d_in, in_bytes, d_out, out_floats)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    untouched = np.ones(out_floats, bool)
    for k, (r, (kind, raw, _, _)) in enumerate(zip(recs, spans)):
        o, n = int(r["out_off"]), int(r["count"])
        want = M.convert(raw, kind)
        ok = M.same_floats(got[o:o + n], want, kind)
        if not ok:
            bad = np.flatnonzero(bits(got[o:o + n]) != bits(want))
            print(f"span {k} kind {kind}: {bad.size} of {n} differ, first at {bad[0]}: got {bits(got[o:o + n])[bad[0]]:#x} want {bits(want)[bad[0]]:#x}")
        assert ok, (k, kind)
        untouched[o:o + n] = False
    assert (got.view(np.uint32)[untouched] == SENTINEL).all(), "a float outside every span was written"
    return got


def test_convert_u8_s16_s24_exhaustively(gpu):
    u8 = np.arange(256, dtype=np.uint8).tobytes()
    s16 = np.arange(65536, dtype="<u2").tobytes()
    v = np.arange(1 << 24, dtype=np.uint32)
    s24 = np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8).tobytes()
    convert(gpu, [(M.KIND_U8, u8, 0, 0), (M.KIND_S16, s16, 0, 0), (M.KIND_S24, s24, 0, 0)])
    # and through the per-sample path (a base that is not aligned for the wide loads)
    convert(gpu, [(M.KIND_U8, u8, 1, 1), (M.KIND_S16, s16, 2, 3), (M.KIND_S24, s24[:3 << 16], 3, 2)])


def edge_s32():
    return np.array([0, 1, -1, 2**31 - 1, -2**31, 2**24, 2**24 + 1, 2**24 + 3, -2**24 - 1, 2**30 + 64, 2**30 + 65, 0x7FFFFFBF, 0x7FFFFFC0,
                     -0x7FFFFFC1, 3, 5, 12345678, -87654321], "<i4")


def test_convert_s32_f32_f64_edges_and_random_bits(gpu):
    rng = np.random.default_rng(21)
    n = 1 << 20
    s32 = np.concatenate([edge_s32(), rng.integers(-2**31, 2**31, n, dtype=np.int64).astype("<i4")]).tobytes()
    f32_edges = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF, 0xFFA00000, 1, 0x807FFFFF,
                          0x00800000, 0x3F800000, 0x7F7FFFFF], "<u4")
    f32 = np.concatenate([f32_edges, rng.integers(0, 2**32, n, dtype=np.uint64).astype("<u4")]).tobytes()
    tiny = np.float64(np.finfo(np.float32).tiny)
    f64_edges = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e300, -1e300, 5e-324, 3.4028234663852886e38, 3.4028235677973366e38,
                          3.4028235677973362e38, tiny, tiny * (1 - 2**-25), tiny * (1 - 2**-24), 1.401298464324817e-45, 0.7e-45, 0.700649232162409e-45,
                          2.1e-45, 1 + 2**-24, 1 + 2**-24 + 2**-50, 1 + 3 * 2**-24, 1 - 2**-25], "<f8")
    near = rng.integers(0, 2**32, n, dtype=np.uint64).astype("<u4").view("<f4").astype("<f8")     # every float exponent, denormals too
    with np.errstate(all="ignore"):
        near = near * (1.0 + rng.integers(-3, 4, n) * 2.0**-24 + rng.integers(-1, 2, n) * 2.0**-52)
    f64 = np.concatenate([f64_edges, near, rng.integers(0, 2**63, n // 4, dtype=np.uint64).astype("<u8").view("<f8"),
                          np.array([0x7FF0000000000001, 0xFFF8000000000000, 0x7FF4000000000000], "<u8").view("<f8")]).tobytes()
    got = convert(gpu, [(M.KIND_S32, s32, 0, 0), (M.KIND_F32, f32, 0, 0), (M.KIND_F64, f64, 0, 0)])
    assert got is not None
    convert(gpu, [(M.KIND_S32, s32[:4 * 5000], 4, 1), (M.KIND_F32, f32[:4 * 5000], 1, 3), (M.KIND_F64, f64[:8 * 5000], 8, 2)])


def test_convert_bases_lengths_and_a_mix_of_all_kinds(gpu):
    rng = np.random.default_rng(22)
    spans = []
    lengths = [0, 1, 2, 3, 4, 5, 7, 8, 63, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 12289, 40000]
    for i, n in enumerate(lengths):
        for kind in range(6):
            in_mis = [0, 0, 0, 16 - afgpu.WAV_KIND_BYTES[kind], 4, 8, 1][(i + kind) % 7]
            out_mis = [0, 0, 0, 1, 2, 3][(i + 2 * kind) % 6]
            spans.append((kind, wb.random_samples(rng, kind, n), in_mis, out_mis))
    order = rng.permutation(len(spans))
    convert(gpu, [spans[k] for k in order])


def open_stream(data):
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    return s


def stream_files(rng):
    out = []
    for kind in range(6):
        ch = [1, 2, 3, 8, 2, 5][kind]
        frames = [5000, 3001, 777, 1200, 200001, 999][kind]
        out.append((kind, ch, [44100, 48000, 8000, 12345, 96000, 22050][kind], wb.random_samples(rng, kind, frames * ch)))
    return out


@pytest.mark.parametrize("read", [1, 7, 1024, 10 ** 6])
def test_stream_reads(gpu, read):
    rng = np.random.default_rng(30)
    for kind, ch, rate, raw in stream_files(rng):
        if read == 1 and len(raw) > 40000:
            raw = raw[:afgpu.WAV_KIND_BYTES[kind] * ch * 1500]
        data = wb.wav_file(kind, ch, rate, raw, fmt_size=[16, 18, 40][kind % 3], before=[wb.chunk(b"LIST", b"abc")] if kind % 2 else ())
        model = M.WavDecoder(data)
        s = open_stream(data)
        assert not s.isError(), s.errorMessage()
        assert s.getFormat() == afgpu.FORMAT_WAV and s.getNumChannels() == ch == model.channels and s.getSamplerate() == float(rate)
        assert s.getLengthInFrames() == model.frames == len(raw) // (afgpu.WAV_KIND_BYTES[kind] * ch)
        assert s.canSeek() and not s.isModule()
        parts = []
        while True:
            buf = np.full(read * ch, np.nan, np.float32)
            n = s.readSamplesFloat(buf)
            wn, want, failed = model.read(read)
            assert n == wn and not failed and not s.isError()
            assert s.tellPosition() == model.tell()
            if n == 0:
                break
            assert M.same_floats(buf[:n * ch], want, kind), (kind, len(parts))
            parts.append(n)
        assert sum(parts) == model.frames
        assert s.readSamplesFloat(np.zeros(ch * 4, np.float32)) == 0 and not s.isError()


def test_stream_seek_and_tell(gpu):
    rng = np.random.default_rng(31)
    for kind, ch, rate, raw in stream_files(rng):
        data = wb.wav_file(kind, ch, rate, raw)
        model = M.WavDecoder(data)
        s = open_stream(data)
        length = model.frames
        for frame in (length // 2, 0, length, length + 1, -1, length // 3, 2**31 - 1, length - 1, 17):
            assert s.seekPosition(frame) == model.seek(frame), frame
            assert s.tellPosition() == model.tell()
            buf = np.full(100 * ch, np.nan, np.float32)
            n = s.readSamplesFloat(buf)
            wn, want, failed = model.read(100)
            assert n == wn and not failed and M.same_floats(buf[:n * ch], want, kind)
            assert s.tellPosition() == model.tell() and not s.isError()


def test_stream_cut_short_file(gpu):
    """A 'data' chunk cut short opens with the declared length; reads that end before the missing byte succeed, the first one
    that needs it returns 0 and leaves the stream in error state, with the position moved by the clamped request."""
    rng = np.random.default_rng(32)
    for kind in range(6):
        ch, frames = 2, 4000
        raw = wb.random_samples(rng, kind, frames * ch)
        whole = wb.wav_file(kind, ch, 44100, raw)
        for cut in (len(raw) // 2 + 1, 1, afgpu.WAV_KIND_BYTES[kind] * ch * 1000):
            data = whole[:len(whole) - cut]
            model = M.WavDecoder(data)
            s = open_stream(data)
            assert not s.isError() and s.getLengthInFrames() == frames == model.frames
            while True:
                buf = np.full(300 * ch, np.nan, np.float32)
                n = s.readSamplesFloat(buf)
                wn, want, failed = model.read(300)
                assert n == wn and s.isError() == failed
                assert s.tellPosition() == model.tell()
                if failed:
                    assert n == 0 and s.errorMessage() == M.DECODING_ERROR
                    assert s.getFormat() == afgpu.FORMAT_UNKNOWN and not s.seekPosition(0)
                    assert s.readSamplesFloat(buf) == 0 and s.tellPosition() == model.tell()
                    break
                assert n == 300 and M.same_floats(buf, want, kind)
        # a seek past what is there, then a read
        data = whole[:len(whole) - len(raw) // 2]
        model, s = M.WavDecoder(data), open_stream(data)
        assert s.seekPosition(frames - 10) and model.seek(frames - 10)
        n = s.readSamplesFloat(np.zeros(50 * ch, np.float32))
        assert (n, True) == model.read(50)[::2] and s.isError() and s.tellPosition() == model.tell() == frames


def test_stream_formats_that_open_and_fail_at_the_first_read(gpu):
    for tag, nbits in ((1, 64), (3, 8), (3, 16), (3, 24)):
        data = wb.riff([wb.fmt_chunk(tag, 2, 8000, nbits), wb.chunk(b"data", bytes(nbits // 8 * 2 * 40))])
        model, s = M.WavDecoder(data), open_stream(data)
        assert not s.isError() and s.getFormat() == afgpu.FORMAT_WAV and s.getLengthInFrames() == 40 and s.getNumChannels() == 2
        n = s.readSamplesFloat(np.zeros(2 * 16, np.float32))
        assert (n, True) == model.read(16)[::2]
        assert s.isError() and s.errorMessage() == M.DECODING_ERROR and s.tellPosition() == model.tell() == 16


@pytest.mark.parametrize("fmt", ["WAV_S8", "WAV_S16LE", "WAV_S24LE", "WAV_FP32LE", "WAV_FP64LE"])
def test_round_trip_through_the_writer(gpu, fmt):
    rng = np.random.default_rng(33)
    pcm = (rng.standard_normal((5000, 2)) * 0.4).astype(np.float32)
    pcm = np.clip(pcm, -1.0, 1.0)
    pcm[:6, 0] = [1.0, -1.0, 0.0, 1.5, -1.5, 1e-40]
    data = afgpu.wav_encode(pcm, 48000, getattr(afgpu, fmt), dither=None)
    verdict = M.whole_file(data)
    assert verdict[0] == "ok"
    want = verdict[2]
    s = open_stream(data)
    assert not s.isError() and s.getNumChannels() == 2 and s.getSamplerate() == 48000.0 and s.getLengthInFrames() == 5000
    got = np.full(5000 * 2, np.nan, np.float32)
    assert s.readSamplesFloat(got) == 5000
    assert np.array_equal(bits(got), bits(want).ravel())
    if fmt in ("WAV_FP32LE", "WAV_FP64LE"):
        assert np.array_equal(bits(got), bits(pcm).ravel())          # the floats come back as they went in
    else:
        peak = {"WAV_S8": 127.0, "WAV_S16LE": 32767.0, "WAV_S24LE": 8388607.0}[fmt]
        assert np.abs(got.reshape(-1, 2)[6:] - pcm[6:]).max() <= 1.0 / peak


def mixed_files():
    rng = np.random.default_rng(34)
    files, wants = [], []
    for i in range(2):
        pcm = make_pcm(3000 + 517 * i, 1 + i % 2, 16, 30 + i)
        d, _ = fb.encode_file(pcm, 16, 1024, sample_rate=44100)
        files.append(d)
        wants.append(("flac", flac_expected(d)[1]))
    d, w = qoa_file(7000, 2, 44100, 44)
    files.append(d)
    wants.append(("qoa", w))
    files.append(open(MP3_FIXTURE, "rb").read())
    wants.append(("mp3", None))
    files.append(mb.random_song(rng, channels=4, n_patterns=1, max_sample=1500))
    wants.append(("mod", pm.decode_batch(files[-1])[0]))
    files.append(b"\x00" * 100)
    wants.append(("junk", None))
    files.append(b"RIFF" + bytes(rng.integers(0, 256, 3000, dtype=np.uint8)))
    wants.append(("junk", None))
    wavs = []
    for kind in range(6):
        for ch, frames in ((1, 4097), (2, 30011), (6, 555)):
            wavs.append(wb.wav_file(kind, ch, 32000 + kind, wb.random_samples(rng, kind, frames * ch), fmt_size=[16, 18, 40][ch % 3]))
    wavs.append(wb.wav_file(M.KIND_F32, 2, 48000, wb.random_samples(rng, M.KIND_F32, 2 * 999), extensible=True))
    wavs.append(wb.wav_file(M.KIND_S16, 2, 48000, b""))                                   # no frames
    wavs.append(wb.wav_file(M.KIND_S16, 2, 48000, wb.random_samples(rng, M.KIND_S16, 2 * 999))[:-5])          # cut short
    wavs.append(wb.riff([wb.fmt_chunk(3, 1, 8000, 16), wb.chunk(b"data", bytes(64))]))    # fails at the first read
    wavs.append(wb.stdlib_wave(2, 44100, 3, rng.integers(0, 256, 6 * 1234, dtype=np.uint8).tobytes()))
    for k, w in enumerate(wavs):
        at = (3 * k + 1) % (len(files) + 1)
        files.insert(at, w)
        wants.insert(at, ("wav", M.whole_file(w)))
    return files, wants


def check_mixed(out, alone, wants):
    others = iter(alone)
    seen = {"ok": 0, "error": 0}
    for item, (what, want) in zip(out, wants):
        if what == "wav":
            assert want[0] != "refused"
            dec = want[1]
            seen[want[0]] += 1
            assert item["format"] == afgpu.FORMAT_WAV and item["channels"] == dec.channels and item["samplerate"] == float(dec.sample_rate)
            if want[0] == "error":
                assert item["status"] != 0 and item["message"] == M.DECODING_ERROR and item["pcm"] is None and item["frames"] == 0
                continue
            assert item["status"] == 0 and item["message"] is None and item["frames"] == dec.frames == len(want[2])
            if dec.frames:
                assert M.same_floats(item["pcm"], want[2], dec.kind)
            else:
                assert item["pcm"] is None
            continue
        ref = next(others)
        if what == "junk":
            assert item["status"] != 0 and item["pcm"] is None and ref["status"] == item["status"]
            assert item["message"] == ref["message"] == M.UNKNOWN_FORMAT
            continue
        assert item["status"] == 0 == ref["status"] and item["frames"] == ref["frames"] and item["format"] == ref["format"]
        assert np.array_equal(bits(item["pcm"]), bits(ref["pcm"]))
        if want is not None:
            assert np.array_equal(bits(item["pcm"]), bits(want))
    assert seen["ok"] >= 20 and seen["error"] == 2


def test_batch_mixes_wav_with_other_formats(gpu):
    files, wants = mixed_files()
    out = afgpu.batch_decode(files, n_threads=3)
    alone = afgpu.batch_decode([f for f, (k, _) in zip(files, wants) if k != "wav"], n_threads=3)
    check_mixed(out, alone, wants)


def test_batch_sharded_over_devices_gives_the_same_items(gpu):
    files, wants = mixed_files()
    one = afgpu.batch_decode(files)
    many = afgpu.batch_decode(files, devices=[0, 0] if afgpu.device_count() < 2 else [0, 1])
    alone = afgpu.batch_decode([f for f, (k, _) in zip(files, wants) if k != "wav"])
    check_mixed(many, alone, wants)
    for a, b in zip(one, many):
        assert (a["status"], a["message"], a["format"], a["channels"], a["frames"]) == (b["status"], b["message"], b["format"], b["channels"], b["frames"])
        assert (a["pcm"] is None) == (b["pcm"] is None)
        if a["pcm"] is not None:
            eq = bits(a["pcm"]) == bits(b["pcm"])
            assert (eq | (np.isnan(a["pcm"]) & np.isnan(b["pcm"]))).all()


def test_batch_file_longer_than_a_chunk(gpu):
    """A file of more samples than one chunk of the batch pipeline (8 Mi samples) is cut at tile boundaries; its neighbours
    share the chunks."""
    rng = np.random.default_rng(35)
    n = (8 << 20) + 12345
    long_raw = rng.integers(0, 256, n * 2, dtype=np.uint8).tobytes()
    files = [wb.wav_file(M.KIND_S24, 1, 8000, wb.random_samples(rng, M.KIND_S24, 5001)), wb.wav_file(M.KIND_S16, 1, 48000, long_raw),
             wb.wav_file(M.KIND_U8, 2, 8000, wb.random_samples(rng, M.KIND_U8, 2 * 7001))]
    for item, f in zip(afgpu.batch_decode(files), files):
        _, dec, want = M.whole_file(f)
        assert item["status"] == 0 and item["frames"] == dec.frames
        assert M.same_floats(item["pcm"], want, dec.kind)


def test_transcode_writes_the_models_samples(gpu, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(36)
    data = wb.wav_file(M.KIND_S24, 2, 44100, wb.random_samples(rng, M.KIND_S24, 2 * 5000), before=[wb.chunk(b"LIST", b"abcd")])
    src, dst = tmp_path / "song.wav", tmp_path / "out.wav"
    src.write_bytes(data)
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "transcode.py"), "--format", "f32", str(src), str(dst)])
    wav = dst.read_bytes()
    want = M.whole_file(data)[2]
    back = M.whole_file(wav)
    assert back[0] == "ok" and back[1].kind == M.KIND_F32 and back[1].channels == 2 and back[1].sample_rate == 44100
    assert np.array_equal(bits(back[2]), bits(want))


SWEEP_SEED, SWEEP_FILES = 2026, 3000


def test_damaged_file_sweep_streams(gpu):
    """The damaged-file recipe through the stream: verdict, header fields, and for the files that open every read up to and
    including the first one that fails.  At most 5 % of the files may end in one of the two rules that are this library's own."""
    rng = np.random.default_rng(SWEEP_SEED + 1)
    own = opened = failed_reads = 0
    files = wb.sweep_files(SWEEP_SEED, SWEEP_FILES)
    for n, (label, data) in enumerate(files):
        model, why = M.open_wav(data)
        s = open_stream(data)
        own += why in M.OWN_RULES
        if model is None:
            assert s.isError() and s.errorMessage() == M.UNKNOWN_FORMAT, (n, label, why)
            continue
        opened += 1
        assert not s.isError(), (n, label, s.errorMessage())
        assert (s.getFormat(), s.getNumChannels(), s.getSamplerate(), s.getLengthInFrames()) == \
               (afgpu.FORMAT_WAV, model.channels, float(np.float32(model.sample_rate)), model.frames), (n, label)
        step = int(rng.choice([64, 500, 4096, 1 << 20]))
        step = max(1, min(step, (1 << 22) // model.channels))        # (a damaged channel count can be 65535)
        while True:
            buf = np.full(step * model.channels, np.nan, np.float32)
            got = s.readSamplesFloat(buf)
            wn, want, failed = model.read(step)
            assert got == wn and s.isError() == failed and s.tellPosition() == model.tell(), (n, label)
            if failed:
                assert s.errorMessage() == M.DECODING_ERROR
                failed_reads += 1
                break
            if got == 0:
                break
            assert M.same_floats(buf[:got * model.channels], want, model.kind), (n, label)
    print(f"sweep: {len(files)} files, {opened} open, {failed_reads} ended in a failing read, {own} in the two own rules")
    assert own <= 0.05 * len(files) and opened >= 0.5 * len(files) and failed_reads >= 0.05 * len(files)


@pytest.mark.parametrize("case", RECORD_CASES)
def test_convert_record_counts_and_spans_without_tiles(gpu, case):
    """1, 2 and 5 spans, with spans of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(13)
    convert(gpu, [(M.KIND_S16, rng.integers(0, 65536, n, dtype=np.uint64).astype("<u2").tobytes(), 2 * (k % 2), k % 4)
                  for k, n in enumerate(record_lengths(afgpu.WAV_TILE_SAMPLES)[case])])
