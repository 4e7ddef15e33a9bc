"""float64 reads without a device: f64_model's arithmetic against exact rational arithmetic, and the two new entry points'
behaviour when there is nothing to run on.

f64_model divides in NumPy float64.  Here every quotient is formed exactly (fractions.Fraction) and rounded once to
binary64 by float(): Fraction.__float__ is int / int true division, which CPython rounds correctly for any operands."""
import ctypes as C
from fractions import Fraction

import numpy as np

import f64_model as fm


def exact(values, divisor):
    return np.array([float(Fraction(int(v), divisor)) for v in values], np.float64)


def test_u8_every_input():
    raw = np.arange(256, dtype=np.uint8)
    want = exact(raw.astype(np.int64) - 128, 127)
    assert fm.same_doubles(fm.convert(raw.tobytes(), fm.KIND_U8), want)


def test_s16_every_input():
    v = np.arange(-32768, 32768, dtype=np.int64)
    assert fm.same_doubles(fm.convert(v.astype("<i2").tobytes(), fm.KIND_S16), exact(v, 32767))


def test_s24_random_inputs_and_edges():
    rng = np.random.default_rng(24)
    v = np.concatenate([np.array([1, -1, 8388607, -8388607, -8388608, 0], np.int64), rng.integers(-2**23, 2**23, 2**16)])
    raw = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    assert (fm.s24_values(raw) == v).all()
    assert fm.same_doubles(fm.convert(raw, fm.KIND_S24), exact(v, 8388607))


def test_s32_and_flac_kinds_round_once():
    rng = np.random.default_rng(32)
    v = np.concatenate([np.array([0, 1, -1, 2**31 - 1, -2**31, 2**24 + 1, -2**24 - 1], np.int64), rng.integers(-2**31, 2**31, 4096)])
    raw = v.astype("<i4").tobytes()
    assert fm.same_doubles(fm.convert(raw, fm.KIND_S32), exact(v, 2**31))                       # exact: a power of two
    k = 1.0 / 2147483647.0
    want = np.array([float(Fraction(int(x)) * Fraction(k)) for x in v], np.float64)             # one rounding of s * k
    assert fm.same_doubles(fm.convert(raw, fm.KIND_FLAC_S32), want)
    assert fm.same_doubles(fm.flac_doubles(v.astype(np.int32)), want)


def test_float_kinds_move_bits():
    rng = np.random.default_rng(64)
    b64 = rng.integers(0, 2**64, 4096, dtype=np.uint64)
    assert (fm.convert(b64.astype("<u8").tobytes(), fm.KIND_F64).view(np.uint64) == b64).all()
    b32 = rng.integers(0, 2**32, 4096, dtype=np.uint64).astype(np.uint32)
    b32 = b32[~fm.is_signalling_f32(b32)]
    got = fm.convert(b32.astype("<u4").tobytes(), fm.KIND_F32)
    back = got.astype(np.float32).view(np.uint32)
    assert (back == b32).all()                                                                  # widening loses nothing
    assert fm.is_signalling_f32(np.array([0x7F800001, 0xFFBFFFFF], np.uint32)).all()
    assert not fm.is_signalling_f32(np.array([0x7F800000, 0x7FC00001, 0x00000001, 0x7F7FFFFF], np.uint32)).any()


def test_read_samples_double_of_null_is_zero():
    import afgpu
    L = afgpu.lib()
    out = np.zeros(8, np.float64)
    assert L.afg_read_samples_double(None, out.ctypes.data, 4) == 0
    assert L.afg_read_samples_double(None, None, 4) == 0
    assert not out.any()


def test_pcm_to_f64_without_a_device_says_so():
    """The entry checks its arguments, then asks for the device: with none it fails loudly and touches nothing."""
    import torch
    import afgpu
    L = afgpu.lib()
    assert L.afg_pcm_to_f64_hip(0, None, 0, None, 0, None, 0, None) == 0                        # nothing to do
    assert L.afg_pcm_to_f64_hip(1, None, 1, None, 0, None, 0, None) == -1                       # AFG_ERR_INVALID: NULL planes
    if torch.cuda.is_available():
        return
    spans = np.zeros(1, afgpu.WAV_SPAN_DTYPE)
    fake = C.c_void_p(spans.ctypes.data)                 # never dereferenced: the device check comes first
    assert L.afg_pcm_to_f64_hip(1, fake, 1, fake, 0, fake, 0, None) == -2                       # AFG_ERR_NO_DEVICE
    assert b"gfx950" in L.afg_last_error() or b"device" in L.afg_last_error()
