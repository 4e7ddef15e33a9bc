"""AudioStream.readSamplesDouble of the reference (stream.d:656-747) as NumPy float64 arithmetic: what each source's
samples become when the caller asks for doubles.  NumPy's float64 is IEEE binary64 with correctly rounded +, *, / and
exact int -> double conversion (below 2^53), so every expression here is the reference's, bit for bit.

Kinds 0-5 are the WAV kinds of wav_model.py (WAVDecoder.readSamples!double, wav.d:242-344); kind 6 is the FLAC path's
int32 sample (stream.d:707-717).  Every other decoder delivers floats, and readSamplesDouble widens them
(stream.d:732-739; QOA multiplies in float first, qoa.d:831-838): `widen`.
"""
import numpy as np

KIND_U8, KIND_S16, KIND_S24, KIND_S32, KIND_F32, KIND_F64, KIND_FLAC_S32 = range(7)
KIND_BYTES = (1, 2, 3, 4, 4, 8, 4)
KIND_NAMES = ("u8", "s16", "s24", "s32", "f32", "f64", "flac_s32")


def s24_values(raw):
    """little-endian 3-byte samples, sign-extended (wav.d:311-317)"""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 3).astype(np.int32)
    s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return (s << 8) >> 8


def convert(raw, kind):
    """Little-endian sample bytes of one kind to float64."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    with np.errstate(all="ignore"):
        if kind == KIND_U8:
            return (raw.astype(np.float64) - 128.0) / 127.0                       # wav.d:297  (b - 128) / 127.0
        if kind == KIND_S16:
            return raw.view("<i2").astype(np.float64) / 32767.0                   # wav.d:307  s / 32767.0
        if kind == KIND_S24:
            return s24_values(raw).astype(np.float64) / 8388607.0                 # wav.d:318-319  s / 8388607.0
        if kind == KIND_S32:
            return raw.view("<i4").astype(np.float64) / 2147483648.0              # wav.d:329  s / 2147483648.0 (exact)
        if kind == KIND_F32:
            return widen(raw.view("<u4").astype(np.uint32).view(np.float32))      # wav.d:266-269  the float, widened
        if kind == KIND_F64:
            return raw.view("<u8").astype(np.uint64).view(np.float64)             # wav.d:276-279  the 64 bits as read
        if kind == KIND_FLAC_S32:
            return raw.view("<i4").astype(np.float64) * (1.0 / 2147483647.0)      # stream.d:713-716  s * (1.0 / int.max)
    raise ValueError(kind)


def widen(floats):
    """stream.d:732-739: a float sample assigned to a double.  Exact; a quiet NaN keeps sign and payload (in the top
    mantissa bits); a signalling NaN comes out a NaN with its sign -- its quiet bit is not specified (`same_doubles`)."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(floats, np.float32).astype(np.float64)


def is_signalling_f32(bits):
    """float32 bit patterns that are signalling NaNs: exponent all ones, quiet bit clear, mantissa not zero"""
    bits = np.asarray(bits, np.uint32)
    return ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x00400000) == 0) & ((bits & 0x003FFFFF) != 0)


def flac_doubles(int32_samples):
    return np.asarray(int32_samples, np.int32).astype(np.float64) * (1.0 / 2147483647.0)    # stream.d:713-716


def same_doubles(got, want):
    """Bit equality of two float64 arrays."""
    got, want = np.ascontiguousarray(got, np.float64).ravel(), np.ascontiguousarray(want, np.float64).ravel()
    return got.shape == want.shape and bool((got.view(np.uint64) == want.view(np.uint64)).all())
