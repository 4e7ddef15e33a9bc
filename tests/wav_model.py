"""WAVDecoder of the reference (wav.d:21-358) over a byte string, as a release build behaves (asserts off): scan(),
readSamples!float, seekPosition, tellPosition on io.d's readers (:33-268) and stream.d's memory callbacks (:2084-2190).

Two places where the reference has no defined result carry the product's rule instead ("WAV"):
  * skip() takes an int: a skip amount that is negative as a 32-bit int moves the cursor backwards and can loop for
    ever.  The file is refused (REASON_SKIP).
  * a 'data' chunk behind a 'fmt ' chunk with 0 channels divides by zero (wav.d:188).  Refused (REASON_CHANNELS).
`OWN_RULES` names them, so that a test can count how often it leans on them.
"""
import struct

import numpy as np

REASON_SKIP = "chunk size is negative as a 32-bit int (refused by this library)"
REASON_CHANNELS = "'data' chunk of a format with 0 channels (refused by this library)"
OWN_RULES = (REASON_SKIP, REASON_CHANNELS)
DECODING_ERROR = "Decoder encountered an error"                     # internals.d: kErrorDecodingError
UNKNOWN_FORMAT = "Cannot decode stream: unrecognized encoding."     # internals.d: kErrorUnknownFormat
IEEE_FLOAT_GUID = bytes([3, 0, 0, 0, 0, 0, 16, 0, 128, 0, 0, 170, 0, 56, 155, 113])   # wav.d:43
KIND_U8, KIND_S16, KIND_S24, KIND_S32, KIND_F32, KIND_F64 = range(6)


class WavError(Exception):
    pass


class _Memory:
    """MemoryContext: the cursor may stand behind the end after a skip."""

    def __init__(self, data):
        self.buf, self.size, self.cursor = bytes(data), len(data), 0

    def remaining(self):                                             # io.d:38-44
        return self.size - self.cursor

    def read(self, n):                                               # memory_read: None = fewer than n bytes were there
        avail = max(self.size - self.cursor, 0)
        if n <= avail:
            out = self.buf[self.cursor:self.cursor + n]
            self.cursor += n
            return out
        self.cursor = max(self.cursor, self.size)
        return None

    def seek(self, offset):                                          # memory_seek, absolute
        if offset < 0:
            return False
        if offset >= self.size:
            self.cursor = self.size
            return False
        self.cursor = offset
        return True

    def skip(self, amount):                                          # skip(int) on memory_skip
        amount &= 0xFFFFFFFF
        if amount >= 0x80000000:
            raise WavError(REASON_SKIP)
        self.cursor += amount

    def u16(self):
        b = self.read(2)
        return None if b is None else struct.unpack("<H", b)[0]

    def u32le(self):
        b = self.read(4)
        return None if b is None else struct.unpack("<I", b)[0]

    def u32be(self):
        b = self.read(4)
        return None if b is None else struct.unpack(">I", b)[0]


def _id(s):
    return struct.unpack(">I", s)[0]


class WavDecoder:
    def __init__(self, data):
        self.io = _Memory(data)
        self.tag = self.channels = self.bits = self.sample_rate = 0
        self.frames = 0                     # _lengthInFrames
        self.samples_off = 0
        self.position = 0                   # _framePosition
        self.scan()

    # wav.d:53-217
    def scan(self):
        io = self.io

        def need(value, reason):
            if value is None:
                raise WavError(reason)
            return value

        cid = need(io.u32be(), "Cannot read RIFF header")
        size = need(io.u32le(), "Cannot read RIFF header")
        if cid != _id(b"RIFF"):
            raise WavError("Expected RIFF chunk.")
        if size < 4:
            raise WavError("RIFF chunk is too small to contain a format.")
        if io.u32be() != _id(b"WAVE"):
            raise WavError("Expected WAVE format.")
        found_fmt = found_data = False
        bits = 0
        while io.remaining() > 0:
            if io.remaining() == 1 and io.buf[io.cursor] == 0:
                break
            cid = need(io.u32be(), "Cannot read RIFF header")
            size = need(io.u32le(), "Cannot read RIFF header")
            if cid == _id(b"fmt "):
                if found_fmt:
                    raise WavError("Found several 'fmt ' chunks in RIFF file.")
                found_fmt = True
                if size < 16:
                    raise WavError("Expected at least 16 bytes in 'fmt ' chunk.")
                self.tag = need(io.u16(), "Cannot read WAV format")
                wfe = self.tag == 0xFFFE
                if self.tag not in (1, 3) and not wfe:
                    raise WavError("Unsupported audio format, only PCM and IEEE float and WAVE_FORMAT_EXTENSIBLE are supported.")
                self.channels = need(io.u16(), "Cannot read number of channels")
                rate = io.u32le() or 0                               # the error flag is not looked at (wav.d:121)
                rate = rate - (1 << 32) if rate >= (1 << 31) else rate
                if rate <= 0:
                    raise WavError("Unsupported sample-rate.")
                self.sample_rate = rate
                need(io.u32le(), "Cannot read bytesPerSec")
                bytes_per_frame = need(io.u16(), "Cannot read bytesPerFrame")
                bits = need(io.u16(), "Cannot read bitsPerSample")
                if bits not in (8, 16, 24, 32, 64):
                    raise WavError("Unsupported bitdepth")
                if bytes_per_frame != (bits // 8) * self.channels:
                    raise WavError("Invalid bytes-per-second, data might be corrupted.")
                if size >= 18:
                    cb = need(io.u16(), "Cannot read cbSize")
                    if wfe:
                        if cb < 22:
                            raise WavError("Unsupported WAVE_FORMAT_EXTENSIBLE.")
                        need(io.u16(), "Cannot read wReserved")
                        need(io.u32le(), "Cannot read dwChannelMask")
                        guid = need(io.read(16), "Cannot read SubFormat")
                        if guid != IEEE_FLOAT_GUID:
                            raise WavError("Unsupported GUID in WAVE_FORMAT_EXTENSIBLE.")
                        self.tag = 3
                        io.skip(size - 40)
                    else:
                        io.skip(size - 18)
                else:
                    io.skip(size - 16)
            elif cid == _id(b"data"):
                if found_data:
                    raise WavError("Found several 'data' chunks in RIFF file.")
                if not found_fmt:
                    raise WavError("'fmt ' chunk expected before the 'data' chunk.")
                frame_size = self.channels * (bits // 8)
                if frame_size == 0:
                    raise WavError(REASON_CHANNELS)
                if size % frame_size:
                    raise WavError("Remaining bytes in 'data' chunk, inconsistent with audio data type.")
                self.frames = size // frame_size
                self.samples_off = io.cursor
                io.skip(size)
                found_data = True
            else:
                io.skip(size)
        if not found_fmt:
            raise WavError("'fmt ' chunk not found.")
        if not found_data:
            raise WavError("'data' chunk not found.")
        self.bits = bits
        io.seek(self.samples_off)
        self.position = 0

    @property
    def bytes_per_sample(self):
        return self.bits // 8

    @property
    def kind(self):
        """What readSamples!float does with the format; -1: it refuses (wav.d:282-286, :332-337)."""
        if self.tag == 3:
            return {32: KIND_F32, 64: KIND_F64}.get(self.bits, -1)
        return {8: KIND_U8, 16: KIND_S16, 24: KIND_S24, 32: KIND_S32}.get(self.bits, -1)

    @property
    def present_samples(self):
        there = max(self.io.size - self.samples_off, 0) // self.bytes_per_sample
        return min(there, self.frames * self.channels)

    # wav.d:220-231
    def seek(self, frame):
        if frame < 0 or frame > self.frames:
            return False
        self.io.seek(self.samples_off + frame * self.channels * self.bytes_per_sample)
        self.position = frame
        return True

    def tell(self):
        return self.position

    # wav.d:242-344: (frames read, float32 samples, failed)
    def read(self, max_frames):
        frames = min(max_frames, self.frames - self.position)
        self.position += frames
        n = frames * self.channels
        kind = self.kind
        empty = np.zeros(0, np.float32)
        if kind < 0:
            return 0, empty, True
        raw = self.io.read(n * self.bytes_per_sample)
        if raw is None:                                              # some sample was not there: "return 0"
            return 0, empty, True
        return frames, convert(raw, kind), False


def convert(raw, kind):
    """readSamples!float's arithmetic on little-endian sample bytes: divide in double, narrow to float."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    with np.errstate(all="ignore"):
        if kind == KIND_U8:
            return ((raw.astype(np.float64) - 128.0) / 127.0).astype(np.float32)
        if kind == KIND_S16:
            return (raw.view("<i2").astype(np.float64) / 32767.0).astype(np.float32)
        if kind == KIND_S24:
            b = raw.reshape(-1, 3).astype(np.int32)
            s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            s = (s << 8) >> 8
            return (s.astype(np.float64) / 8388607.0).astype(np.float32)
        if kind == KIND_S32:
            return (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
        if kind == KIND_F32:
            return raw.view("<u4").astype(np.uint32).view(np.float32)
        if kind == KIND_F64:
            return raw.view("<f8").astype(np.float32)
    raise ValueError(kind)


def same_floats(got, want, kind):
    """Bit equality; for f64 input a NaN only has to stay a NaN."""
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    if got.shape != want.shape:
        return False
    eq = got.view(np.uint32) == want.view(np.uint32)
    if kind == KIND_F64:
        eq |= np.isnan(got) & np.isnan(want)
    return bool(eq.all())


def open_wav(data):
    """(decoder, None) or (None, reason)."""
    try:
        return WavDecoder(data), None
    except WavError as e:
        return None, str(e)


def whole_file(data):
    """What the batch path delivers: one read of the whole declared length.  ("refused", reason) | ("error", decoder) |
    ("ok", decoder, samples [frames, channels])."""
    dec, why = open_wav(data)
    if dec is None:
        return ("refused", why)
    if dec.kind < 0:
        return ("error", dec)
    if dec.frames == 0:
        return ("ok", dec, np.zeros((0, dec.channels), np.float32))
    n, pcm, failed = dec.read(dec.frames)
    if failed:
        return ("error", dec)
    return ("ok", dec, pcm.reshape(n, dec.channels))
