"""The WAV host front-end (afg_wav_parse: WAVDecoder.scan, no device needed) against tests/wav_model.py: well-formed
files of every layout, every refusal of wav.d:61-210, hostile chunk sizes, the RIFF-prefixed non-WAV files of the older
tests, and a damaged-file sweep."""
import struct
import threading

import numpy as np
import pytest

import afgpu
import wav_bitstream as wb
import wav_model as M


def product(data):
    """(fields, None) or (None, reason)."""
    try:
        return afgpu.wav_parse(data), None
    except afgpu.AfgError as e:
        text = str(e)
        assert "afg_wav_parse: " in text, text
        return None, text.split("afg_wav_parse: ", 1)[1].strip()


def agree(data, label=""):
    """Product and model give the same verdict and fields; returns the model's reason (None: opens)."""
    dec, why = M.open_wav(data)
    got, got_why = product(data)
    assert got_why == why, (label, got_why, why)
    if dec is not None:
        want = {"tag": dec.tag, "channels": dec.channels, "bits": dec.bits, "sample_rate": dec.sample_rate, "frames": dec.frames,
                "kind": dec.kind, "samples_offset": dec.samples_off, "present_samples": dec.present_samples}
        assert got == want, (label, got, want)
    return why


def test_well_formed_files_parse_as_the_model():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(4):
        for label, data in wb.base_files(rng, max_channels=8):
            assert agree(data, label) is None, label
            seen.add(label)
    assert {"kind0", "kind5", "fmt18", "fmt40pcm", "ext_f32", "list_cue", "odd_chunk", "trailing0", "stdlib"} <= seen
    # mono to 8 channels and more, odd rates
    for ch in (1, 2, 3, 5, 8, 255, 65535 // 2):
        data = wb.wav_file(M.KIND_S16, ch, 7919, wb.random_samples(rng, M.KIND_S16, ch * 5))
        assert agree(data) is None
        assert afgpu.wav_parse(data)["channels"] == ch


def test_stdlib_wave_files_open():
    rng = np.random.default_rng(12)
    for sw, kind in ((1, M.KIND_U8), (2, M.KIND_S16), (3, M.KIND_S24), (4, M.KIND_S32)):
        raw = rng.integers(0, 256, 100 * 2 * sw, dtype=np.uint8).tobytes()
        data = wb.stdlib_wave(2, 22050, sw, raw)
        assert agree(data) is None
        p = afgpu.wav_parse(data)
        assert (p["kind"], p["channels"], p["sample_rate"], p["frames"], p["present_samples"]) == (kind, 2, 22050, 100, 200)
        assert data[p["samples_offset"]:] == raw


def refusals():
    s16 = wb.random_samples(np.random.default_rng(3), M.KIND_S16, 64)
    fmt = wb.fmt_chunk(1, 2, 44100, 16)
    data = wb.chunk(b"data", s16)
    ext = lambda **kw: wb.fmt_chunk(0xFFFE, 2, 44100, 32, 40, **kw)
    head = lambda n: wb.riff([fmt])[:12] + wb.fmt_chunk(1, 2, 44100, 16)[:n]
    return {
        "Cannot read RIFF header": b"RIFF\x10\0",
        "Expected RIFF chunk.": b"RIFX" + wb.riff([fmt, data])[4:],
        "RIFF chunk is too small to contain a format.": b"RIFF\x03\0\0\0WAVE",
        "Expected WAVE format.": b"RIFF\x10\0\0\0AVI " + fmt,
        "Found several 'fmt ' chunks in RIFF file.": wb.riff([fmt, fmt, data]),
        "Expected at least 16 bytes in 'fmt ' chunk.": wb.riff([wb.chunk(b"fmt ", b"\1\0\2\0" * 3), data]),
        "Cannot read WAV format": head(8 + 1),
        "Unsupported audio format, only PCM and IEEE float and WAVE_FORMAT_EXTENSIBLE are supported.": wb.riff([wb.fmt_chunk(6, 2, 8000, 8), data]),
        "Cannot read number of channels": head(8 + 3),
        "Unsupported sample-rate.": wb.riff([wb.fmt_chunk(1, 2, 0x80000000, 16), data]),
        "Cannot read bytesPerSec": head(8 + 10),
        "Cannot read bytesPerFrame": head(8 + 13),
        "Cannot read bitsPerSample": head(8 + 15),
        "Unsupported bitdepth": wb.riff([wb.fmt_chunk(1, 2, 44100, 12, block_align=2), data]),
        "Invalid bytes-per-second, data might be corrupted.": wb.riff([wb.fmt_chunk(1, 2, 44100, 16, block_align=2), data]),
        "Cannot read cbSize": wb.riff([fmt])[:12] + wb.fmt_chunk(1, 2, 44100, 16, 18)[:8 + 17],
        "Unsupported WAVE_FORMAT_EXTENSIBLE.": wb.riff([ext(cb=20), data]),
        "Cannot read wReserved": wb.riff([fmt])[:12] + ext()[:8 + 19],
        "Cannot read dwChannelMask": wb.riff([fmt])[:12] + ext()[:8 + 22],
        "Cannot read SubFormat": wb.riff([fmt])[:12] + ext()[:8 + 30],
        "Unsupported GUID in WAVE_FORMAT_EXTENSIBLE.": wb.riff([ext(guid=wb.PCM_GUID), wb.chunk(b"data", s16 + s16)]),
        "Found several 'data' chunks in RIFF file.": wb.riff([fmt, data, data]),
        "'fmt ' chunk expected before the 'data' chunk.": wb.riff([data, fmt]),
        "Remaining bytes in 'data' chunk, inconsistent with audio data type.": wb.riff([fmt, wb.chunk(b"data", s16[:-1])]),
        "'fmt ' chunk not found.": wb.riff([wb.chunk(b"LIST", b"abcd")]),
        "'data' chunk not found.": wb.riff([fmt]),
        # a byte that is not 0 left over at the end
        "Cannot read RIFF header#2": wb.riff([fmt, data], trailer=b"\x01"),
    }


def test_every_refusal_of_the_scan():
    for reason, data in refusals().items():
        want = reason.split("#")[0]
        assert agree(data, reason) == want, reason


def within(seconds, fn, *args):
    """fn(*args) on a helper thread; fails when it has not returned in time (a C call releases the interpreter lock)."""
    box = {}

    def run():
        try:
            box["value"] = fn(*args)
        except BaseException as e:      # noqa: BLE001 - handed to the caller's thread
            box["error"] = e
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(seconds)
    assert not th.is_alive(), f"no verdict within {seconds} s: {args[1:]}"
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_hostile_sizes_terminate_with_the_models_verdict():
    s16 = bytes(64)
    fmt = wb.fmt_chunk(1, 2, 44100, 16)
    cases = {
        # an unknown chunk at offset 12 whose size runs (almost) round the 32-bit clock: the reference's skip(int) goes back 8 bytes
        "0xFFFFFFF8": wb.riff([wb.chunk(b"JUNK", b"", 0xFFFFFFF8), fmt, wb.chunk(b"data", s16)]),
        "0x80000000": wb.riff([fmt, wb.chunk(b"JUNK", b"", 0x80000000), wb.chunk(b"data", s16)]),
        "data 0x80000000": wb.riff([wb.fmt_chunk(1, 1, 8000, 8), wb.chunk(b"data", s16, 0x80000000)]),
        # extensible, an 18-byte chunk, cbSize 22: the skip is 18 - 40
        "ext18": wb.riff([wb.fmt_chunk(0xFFFE, 2, 44100, 32, 40, declared=18), wb.chunk(b"data", s16)]),
        "fmt17": wb.riff([wb.fmt_chunk(1, 2, 44100, 16, 18, declared=0xFFFFFFFF), wb.chunk(b"data", s16)]),
        "channels0": wb.riff([wb.fmt_chunk(1, 0, 44100, 16), wb.chunk(b"data", s16)]),
        "channels0 no data": wb.riff([wb.fmt_chunk(1, 0, 44100, 16)]),
        # just under the line: the chunk runs past the end of the file, which the scan allows
        "0x7FFFFFFF": wb.riff([fmt, wb.chunk(b"data", s16), wb.chunk(b"JUNK", b"", 0x7FFFFFFF)]),
        "data 0x7FFFFFFE": wb.riff([wb.fmt_chunk(1, 1, 8000, 16), wb.chunk(b"data", s16, 0x7FFFFFFE)]),
    }
    want = {"0xFFFFFFF8": M.REASON_SKIP, "0x80000000": M.REASON_SKIP, "data 0x80000000": M.REASON_SKIP, "ext18": M.REASON_SKIP,
            "fmt17": M.REASON_SKIP, "channels0": M.REASON_CHANNELS, "channels0 no data": "'data' chunk not found.",
            "0x7FFFFFFF": None, "data 0x7FFFFFFE": None}
    for label, data in cases.items():
        assert within(10.0, agree, data, label) == want[label], label
    p = afgpu.wav_parse(cases["data 0x7FFFFFFE"])
    assert p["frames"] == 0x7FFFFFFE // 2 and p["present_samples"] == 32


def test_open_but_unreadable_formats_and_short_data():
    """What the scan lets through and readSamples refuses has kind -1; a 'data' chunk cut short keeps its declared length."""
    for tag, bits in ((1, 64), (3, 8), (3, 16), (3, 24)):
        data = wb.riff([wb.fmt_chunk(tag, 1, 8000, bits), wb.chunk(b"data", bytes(bits // 8 * 24))])
        assert agree(data) is None
        assert afgpu.wav_parse(data)["kind"] == -1
    whole = wb.wav_file(M.KIND_S24, 2, 48000, bytes(6 * 100))
    cut = whole[:-301]
    assert agree(cut) is None
    p = afgpu.wav_parse(cut)
    assert p["frames"] == 100 and p["present_samples"] == (600 - 301) // 3


def test_riff_prefixed_non_wav_files_stay_unrecognized():
    """The RIFF-prefixed files of the MP3 and MOD front-end tests: the scan refuses them by the reference's own checks, so they
    come out as they did before WAV was decoded -- and that needs no device."""
    import mod_bitstream as mb
    from test_mp3_frontend import real
    rng = np.random.default_rng(5)
    good = mb.random_song(rng, channels=4, n_patterns=1, max_sample=500)
    for data in (b"RIFF" + real(), b"RIFF" + bytes(4) + b"WAVE" + good[12:], b"RF64" + bytes(600),
                 b"RIFF" + struct.pack("<I", 4096) + b"AVI " + bytes(4096)):
        dec, why = M.open_wav(data)
        assert dec is None and why not in M.OWN_RULES
        assert product(data)[1] == why
        s = afgpu.AudioStream()
        s.openFromMemory(data)
        assert s.isError() and s.errorMessage() == M.UNKNOWN_FORMAT
        assert s.getFormat() == afgpu.FORMAT_UNKNOWN and s.tellPosition() == -1


SWEEP_SEED, SWEEP_FILES = 2026, 20000


def test_damaged_file_sweep_parser():
    """Every file of the sweep, nothing left out: verdict and header fields, product against model; at most 5 % of the files may
    end in one of the two rules that are this library's own."""
    own = opened = short = 0
    files = wb.sweep_files(SWEEP_SEED, SWEEP_FILES)
    for n, (label, data) in enumerate(files):
        why = agree(data, (n, label))
        own += why in M.OWN_RULES
        if why is None:
            opened += 1
            dec, _ = M.open_wav(data)
            short += dec.present_samples < dec.frames * dec.channels
    print(f"sweep: {len(files)} files, {opened} open ({short} with 'data' cut short), {len(files) - opened - own} refused by the "
          f"reference's checks, {own} by the two own rules ({100.0 * own / len(files):.2f} %)")
    assert own <= 0.05 * len(files), own
    assert opened >= 0.5 * len(files) and short >= 0.05 * len(files)
