"""Encode side, host-only parts of the C ABI (no GPU): afg_lcg31_jump against stepping the dither generator,
afg_wav_pack_layout against a restatement, and the argument refusals of the encode entries."""
import ctypes as C

import numpy as np

import afgpu

A, INC, M = 1103515245, 12345, 1 << 31
SEEDS = [0, 1, 12345, 0x7FFFFFFF, 0x2545F491, 0x40000000]


def step(state, n):
    for _ in range(n):
        state = (state * A + INC) % M
    return state


def closed_form(seed, n):
    """n steps of x -> (A x + INC) mod 2^31 without stepping: A^n x + INC (A^n - 1) / (A - 1); the quotient is exact, so the
    power is taken modulo (A - 1) 2^31."""
    an = pow(A, n, (A - 1) * M)
    return (an * seed + INC * ((an - 1) // (A - 1))) % M


def test_closed_form_is_the_stepped_generator():
    for seed in SEEDS:
        s = seed
        for n in range(200):
            assert closed_form(seed, n) == s
            s = (s * A + INC) % M


def test_jump_equals_stepping_for_every_small_count():
    for seed in SEEDS:
        s = seed
        for n in range(4097):
            assert afgpu.lcg31_jump(seed, n) == s, (seed, n)
            s = (s * A + INC) % M


def test_jump_at_powers_of_two_and_random_counts():
    rng = np.random.default_rng(3)
    counts = [((1 << k) + d) for k in range(1, 41) for d in (-1, 0, 1)]
    counts += [int(v) for v in rng.integers(0, 1 << 40, 200)] + [int(v) for v in rng.integers(0, 1 << 20, 50)]
    for seed in SEEDS + [int(v) for v in rng.integers(0, M, 5)]:
        for n in counts:
            assert afgpu.lcg31_jump(seed, n) == closed_form(seed, n), (seed, n)
    for n in [int(v) for v in rng.integers(5000, 200000, 6)]:                     # and against plain stepping
        assert afgpu.lcg31_jump(77, n) == step(77, n)


def test_jump_takes_the_seed_modulo_2_31():
    assert afgpu.lcg31_jump(0x80000005, 9) == afgpu.lcg31_jump(5, 9)


def test_pack_layout_counts_tiles():
    rng = np.random.default_rng(4)
    counts = [0, 1, 3, 4, 4095, 4096, 4097, 0, 1 << 24, 8191, 8192] + [int(v) for v in rng.integers(0, 100000, 40)]
    spans = np.zeros(len(counts), afgpu.WAV_PACK_SPAN_DTYPE)
    spans["count"] = counts
    spans["first_tile"] = 99
    tiles = afgpu.wav_pack_layout(spans)
    at = 0
    for c, sp in zip(counts, spans):
        assert int(sp["first_tile"]) == at
        at += (c + afgpu.WAV_TILE_SAMPLES - 1) // afgpu.WAV_TILE_SAMPLES
    assert tiles == at
    assert afgpu.lib().afg_wav_pack_layout(None, 5) == 0
    assert afgpu.wav_pack_layout(spans[:0].copy()) == 0


def test_span_record_matches_the_header():
    d = afgpu.WAV_PACK_SPAN_DTYPE
    assert d.itemsize == 48
    assert [d.fields[k][1] for k in ("in_off", "out_off", "count", "first_tile", "draw0", "seed", "format", "dither")] == \
        [0, 8, 16, 24, 32, 40, 44, 45]
    assert C.sizeof(afgpu.EncodingOptions) == 16 and C.sizeof(afgpu.EncodeInput) == 24 and C.sizeof(afgpu.EncodedItem) == 32


def test_pack_refuses_bad_arguments():
    L = afgpu.lib()
    assert L.afg_wav_pack_hip(0, None, 0, None, 0, None, 0, None) == 0           # nothing to do
    assert L.afg_wav_pack_hip(1, None, 1, None, 0, None, 0, None) == -1          # AFG_ERR_INVALID
    assert b"NULL" in L.afg_last_error()
    assert L.afg_wav_pack_hip(1, 4096, 1, 4096 + 4, 16, 8192, 16, None) == -1    # planes not 16-byte aligned
    assert L.afg_wav_pack_hip(1 << 32, 4096, 1, 4096, 16, 8192, 16, None) == -1
    assert L.afg_wav_pack_hip(1, 4096, 1 << 31, 4096, 16, 8192, 16, None) == -1


def test_batch_encode_refuses_bad_arguments():
    L = afgpu.lib()
    res = afgpu.EncodeResult()
    one = (afgpu.EncodeInput * 1)()
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, None, 0, None) == -1
    assert L.afg_batch_encode(None, 1, afgpu.FORMAT_WAV, None, 0, C.byref(res)) == -1
    assert L.afg_batch_encode(one, -1, afgpu.FORMAT_WAV, None, 0, C.byref(res)) == -1
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, None, -2, C.byref(res)) == -1
    bad = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF)
    bad.struct_size = 12
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, C.byref(bad), 0, C.byref(res)) == -1
    assert b"struct_size" in L.afg_last_error()
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, C.byref(afgpu.encoding_options(7, 0)), 0, C.byref(res)) == -1
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, C.byref(afgpu.encoding_options(afgpu.WAV_S16LE, 9)), 0, C.byref(res)) == -1
    # formats nobody writes, and the reference's own dither on an integer format: unsupported for the whole call
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_FLAC, None, 0, C.byref(res)) == -5
    assert L.afg_batch_encode(one, 1, afgpu.FORMAT_WAV, C.byref(afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LIBC)), 0,
                              C.byref(res)) == -5
    assert res.n_files == 0 and not res.items and not res.owner
    L.afg_encode_free(C.byref(res))                                              # harmless on an empty result
    L.afg_encode_free(None)


def test_write_entries_take_null_handles():
    L = afgpu.lib()
    x = np.zeros(8, np.float32)
    assert L.afg_write_samples_float(None, x.ctypes.data, 4) == 0
    assert L.afg_write_samples_double(None, x.ctypes.data, 1) == 0
    assert L.afg_finalize_encoding(None) == 0
    p, n = C.POINTER(C.c_uint8)(), C.c_size_t(5)
    assert L.afg_finalize_and_get_encoded(None, C.byref(p), C.byref(n)) == 0 and n.value == 0
    assert L.afg_is_open_for_writing(None) == 0 and L.afg_is_open_for_reading(None) == 0


def test_unsupported_formats_carry_the_reference_message():
    """No device is needed to refuse: the format is looked at first."""
    for fmt in (afgpu.FORMAT_MP3, afgpu.FORMAT_FLAC, afgpu.FORMAT_OGG, afgpu.FORMAT_OPUS, afgpu.FORMAT_MOD, afgpu.FORMAT_XM,
                afgpu.FORMAT_UNKNOWN):
        st = afgpu.AudioStream()
        st.openToBuffer(fmt, 44100, 2)
        assert st.isError() and st.isOpenForWriting() and not st.isOpenForReading()
        assert st.errorMessage() == "Unsupported encoding format, maybe check your audio-formats configuration"
        assert st.writeSamplesFloat(np.zeros((4, 2), np.float32)) == 0 and not st.finalizeEncoding()
        st.cleanUp()
    for kw in (dict(fmt=afgpu.FORMAT_QOA, samplerate=0, channels=2), dict(fmt=afgpu.FORMAT_QOA, samplerate=1 << 24, channels=2),
               dict(fmt=afgpu.FORMAT_QOA, samplerate=44100, channels=9), dict(fmt=afgpu.FORMAT_QOA, samplerate=44100, channels=0),
               dict(fmt=afgpu.FORMAT_WAV, samplerate=44100, channels=1025), dict(fmt=afgpu.FORMAT_WAV, samplerate=44100, channels=-1)):
        st = afgpu.AudioStream()
        st.openToBuffer(**kw)
        assert st.isError() and st.errorMessage() == "Encoder encountered an error", kw
    bad = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF)
    bad.struct_size = 8
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_WAV, 44100, 2, bad)
    assert st.isError() and st.errorMessage() == "Encoder encountered an error"
