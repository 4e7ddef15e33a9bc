"""Builds WAV files for the tests: every sample kind, any channel count, 16- / 18- / 40-byte 'fmt ' chunks, extensible
headers, extra chunks before and after 'data', odd-sized chunks without a pad byte, a trailing single byte -- and the
damaged-file recipe of the sweep.  Python's `wave` module serves as a writer none of us wrote (stdlib_wave)."""
import io
import struct
import wave

import numpy as np

import wav_model as M

KIND_FORMAT = {M.KIND_U8: (1, 8), M.KIND_S16: (1, 16), M.KIND_S24: (1, 24), M.KIND_S32: (1, 32), M.KIND_F32: (3, 32),
               M.KIND_F64: (3, 64)}
PCM_GUID = bytes([1, 0, 0, 0, 0, 0, 16, 0, 128, 0, 0, 170, 0, 56, 155, 113])


def chunk(cid, payload, size=None):
    """A RIFF chunk as the reference reads it: no pad byte after an odd size."""
    return cid + struct.pack("<I", len(payload) if size is None else size) + payload


def fmt_chunk(tag, channels, rate, bits, size=16, cb=None, guid=M.IEEE_FLOAT_GUID, block_align=None, declared=None):
    align = (bits // 8) * channels if block_align is None else block_align
    body = struct.pack("<HHIIHH", tag, channels, rate & 0xFFFFFFFF, (rate * align) & 0xFFFFFFFF, align & 0xFFFF, bits)
    if size >= 18:
        body += struct.pack("<H", (22 if size >= 40 else 0) if cb is None else cb)
    if size >= 40:
        body += struct.pack("<HI", bits, (1 << channels) - 1 & 0xFFFFFFFF) + guid
    body += b"\0" * (size - len(body)) if size > len(body) else b""
    return chunk(b"fmt ", body, declared)


def riff(chunks, trailer=b""):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body + trailer


def random_samples(rng, kind, n):
    """n samples of the kind as little-endian bytes; floats include specials."""
    if kind == M.KIND_F32:
        x = (rng.standard_normal(n) * 0.5).astype("<f4")
        if n >= 8:
            x[:8] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-45, 1.0, -1.0], "<f4")
        return x.tobytes()
    if kind == M.KIND_F64:
        x = (rng.standard_normal(n) * 0.5).astype("<f8")
        if n >= 8:
            x[:8] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-46, 1e300, 5e-324], "<f8")
        return x.tobytes()
    return rng.integers(0, 256, n * KIND_FORMAT[kind][1] // 8, dtype=np.uint8).tobytes()


def wav_file(kind, channels, rate, sample_bytes, fmt_size=16, before=(), after=(), trailer=b"", extensible=False, **fmt_args):
    tag, bits = KIND_FORMAT[kind]
    if extensible:
        tag, fmt_size = 0xFFFE, max(fmt_size, 40)
    return riff(list(before) + [fmt_chunk(tag, channels, rate, bits, fmt_size, **fmt_args)] + [chunk(b"data", sample_bytes)] + list(after),
                trailer)


def stdlib_wave(channels, rate, sampwidth, sample_bytes):
    """The file Python's wave module writes for the sample bytes (8-bit unsigned, 16 / 24 / 32-bit signed little-endian)."""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(sampwidth)
        w.setframerate(rate)
        w.writeframes(sample_bytes)
    return buf.getvalue()


def base_files(rng, frames=(200, 3000), max_channels=3):
    """One well-formed file per layout the tests name; list of (label, bytes)."""
    out = []

    def body(kind, ch):
        n = int(rng.integers(frames[0], frames[1] + 1))
        return random_samples(rng, kind, n * ch)

    rates = (8000, 11025, 22050, 44100, 48000, 96000, 12345, 1)
    for kind in range(6):
        ch = int(rng.integers(1, max_channels + 1))
        out.append((f"kind{kind}", wav_file(kind, ch, int(rng.choice(rates)), body(kind, ch))))
    ch = int(rng.integers(1, max_channels + 1))
    out.append(("fmt18", wav_file(M.KIND_S16, ch, 44100, body(M.KIND_S16, ch), fmt_size=18)))
    out.append(("fmt40pcm", wav_file(M.KIND_S24, ch, 48000, body(M.KIND_S24, ch), fmt_size=40)))
    out.append(("ext_f32", wav_file(M.KIND_F32, ch, 48000, body(M.KIND_F32, ch), extensible=True)))
    out.append(("ext_f64", wav_file(M.KIND_F64, ch, 22050, body(M.KIND_F64, ch), extensible=True, fmt_size=44)))
    out.append(("list_cue", wav_file(M.KIND_S16, ch, 32000, body(M.KIND_S16, ch), before=[chunk(b"LIST", b"INFOISFT\x04\0\0\0afg\0")],
                                     after=[chunk(b"cue ", struct.pack("<I", 0))])))
    out.append(("odd_chunk", wav_file(M.KIND_U8, ch, 8000, body(M.KIND_U8, ch), before=[chunk(b"junk", b"abc")])))
    out.append(("trailing0", wav_file(M.KIND_S16, ch, 44100, body(M.KIND_S16, ch), after=[chunk(b"AFAn", b"xy")], trailer=b"\0")))
    sw = int(rng.integers(1, 5))
    n = int(rng.integers(frames[0], frames[1] + 1))
    out.append(("stdlib", stdlib_wave(ch, 44100, sw, rng.integers(0, 256, n * ch * sw, dtype=np.uint8).tobytes())))
    return out


def damage(rng, data):
    """One of: cut at a random byte; 1-4 random byte replacements anywhere; 1-4 in the first 80 bytes."""
    b = bytearray(data)
    how = int(rng.integers(0, 3))
    if how == 0:
        return bytes(b[:int(rng.integers(0, len(b)))])
    span = len(b) if how == 1 else min(80, len(b))
    for _ in range(int(rng.integers(1, 5))):
        b[int(rng.integers(0, span))] = int(rng.integers(0, 256))
    return bytes(b)


def sweep_files(seed, count, frames=(200, 3000), max_channels=3):
    """The damaged-file sweep's files: (label, bytes), deterministic in the seed."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        for label, data in base_files(rng, frames, max_channels):
            out.append((label, damage(rng, data)))
            if len(out) == count:
                break
    return out
