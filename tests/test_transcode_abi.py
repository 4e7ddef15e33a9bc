"""Batch decode to packed PCM and batch transcode, host-only parts of the C ABI (no GPU): the new symbols, the tile layout
of afg_pcm_pack_layout, the struct sizes, and every refusal that is made before any device work."""
import ctypes as C

import numpy as np

import afgpu


def test_the_new_symbols_exist():
    L = afgpu.lib()
    for name in ("afg_pcm_pack_layout", "afg_pcm_pack_hip", "afg_batch_transcode"):
        assert hasattr(L, name) and name in afgpu.ABI_SYMBOLS, name
    assert (afgpu.SAMPLE_F32, afgpu.SAMPLE_F64, afgpu.SAMPLE_PCM_S8, afgpu.SAMPLE_PCM_S16, afgpu.SAMPLE_PCM_S24) == (0, 1, 2, 3, 4)
    assert L.afg_abi_version() == 2


def test_pcm_pack_layout_counts_tiles():
    counts = [0, 1, 4096, 4097, 0, 8192, 12289]
    spans = np.zeros(len(counts), afgpu.PCM_PACK_SPAN_DTYPE)
    spans["count"] = counts
    spans["first_tile"] = 99
    assert afgpu.pcm_pack_layout(spans) == 0 + 1 + 1 + 2 + 0 + 2 + 4
    assert [int(v) for v in spans["first_tile"]] == [0, 0, 1, 2, 4, 4, 6]
    for count, tiles in ((0, 0), (1, 1), (4096, 1), (4097, 2)):
        one = np.zeros(1, afgpu.PCM_PACK_SPAN_DTYPE)
        one["count"] = count
        one["first_tile"] = 7
        assert afgpu.pcm_pack_layout(one) == tiles and int(one["first_tile"][0]) == 0
    assert afgpu.lib().afg_pcm_pack_layout(None, 5) == 0
    assert afgpu.pcm_pack_layout(spans[:0].copy()) == 0


def test_struct_sizes():
    d = afgpu.PCM_PACK_SPAN_DTYPE
    assert d.itemsize == 48
    assert [d.fields[k][1] for k in ("in_off", "out_off", "count", "first_tile", "draw0", "seed", "format", "dither")] == \
        [0, 8, 16, 24, 32, 40, 44, 45]
    B = afgpu.BatchOpts
    assert C.sizeof(B) == 40                                     # sizeof(afg_batch_opts)
    assert afgpu.BATCH_OPTS_SIZE_V1 == 24 == B.sample_type.offset                # ... before sample_type
    assert afgpu.BATCH_OPTS_SIZE_V2 == 28 == B.dither.offset                     # ... up to sample_type
    assert B.dither_seed.offset == 32


def test_pcm_pack_refuses_bad_arguments():
    L = afgpu.lib()
    assert L.afg_pcm_pack_hip(0, None, 0, None, 0, None, 0, None) == 0           # nothing to do
    assert L.afg_pcm_pack_hip(1, None, 1, None, 0, None, 0, None) == -1          # AFG_ERR_INVALID
    assert b"NULL" in L.afg_last_error()
    assert L.afg_pcm_pack_hip(1, 4096, 1, 4096 + 2, 16, 8192, 16, None) == -1    # floats are 4-byte aligned
    assert L.afg_pcm_pack_hip(1 << 32, 4096, 1, 4096, 16, 8192, 16, None) == -1
    assert L.afg_pcm_pack_hip(1, 4096, 1 << 31, 4096, 16, 8192, 16, None) == -1


def transcode(data, lens, n, fmt, enc, opts, res):
    return afgpu.lib().afg_batch_transcode(data, lens, n, fmt, None if enc is None else C.byref(enc), None if opts is None else C.byref(opts),
                                           None if res is None else C.byref(res))


def test_batch_transcode_refuses_bad_arguments():
    L = afgpu.lib()
    res = afgpu.EncodeResult()
    files = [b"not a file"]
    ptrs = (C.c_char_p * 1)(*files)
    lens = (C.c_size_t * 1)(len(files[0]))
    s16 = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF)
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, s16, None, None) == -1
    assert transcode(None, lens, 1, afgpu.FORMAT_WAV, s16, None, res) == -1
    assert transcode(ptrs, None, 1, afgpu.FORMAT_WAV, s16, None, res) == -1
    assert transcode(ptrs, lens, -1, afgpu.FORMAT_WAV, s16, None, res) == -1
    bad = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF)
    bad.struct_size = 12
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, bad, None, res) == -1
    assert b"struct_size" in L.afg_last_error()
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, afgpu.encoding_options(7, 0), None, res) == -1
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, afgpu.encoding_options(afgpu.WAV_S16LE, 9), None, res) == -1
    short = afgpu.BatchOpts(8, 0, 0, None, 0, 0, 0)
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, s16, short, res) == -1
    # QOA output: unsupported, with its own message
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_QOA, s16, None, res) == -5
    assert b"QOA" in L.afg_last_error()
    assert transcode(ptrs, lens, 1, afgpu.FORMAT_FLAC, s16, None, res) == -5
    # the reference's own dither on an integer format has no draw order across files
    for fmt in (afgpu.WAV_S8, afgpu.WAV_S16LE, afgpu.WAV_S24LE):
        assert transcode(ptrs, lens, 1, afgpu.FORMAT_WAV, afgpu.encoding_options(fmt, afgpu.DITHER_LIBC), None, res) == -1
        assert b"dither" in L.afg_last_error()
    assert res.n_files == 0 and not res.items and not res.owner
    L.afg_encode_free(C.byref(res))


def decode(files, opts):
    ptrs = (C.c_char_p * len(files))(*files)
    lens = (C.c_size_t * len(files))(*[len(f) for f in files])
    res = afgpu.BatchResult()
    return afgpu.lib().afg_batch_decode_ex(ptrs, lens, len(files), C.byref(opts), C.byref(res)), res


def test_batch_decode_refuses_before_any_work():
    L = afgpu.lib()
    files = [b"not a file"]
    for sample_type in (5, 7, 0xffffffff):
        rc, res = decode(files, afgpu.BatchOpts(C.sizeof(afgpu.BatchOpts), 0, 0, None, sample_type, afgpu.DITHER_OFF, 0))
        assert rc == -1 and res.n_files == 0 and not res.items
        assert b"sample_type" in L.afg_last_error()
    for sample_type in (afgpu.SAMPLE_F32, afgpu.SAMPLE_PCM_S8, afgpu.SAMPLE_PCM_S16, afgpu.SAMPLE_PCM_S24):
        rc, res = decode(files, afgpu.BatchOpts(C.sizeof(afgpu.BatchOpts), 0, 0, None, sample_type, afgpu.DITHER_LIBC, 0))
        assert rc == -1 and res.n_files == 0 and not res.items
        assert b"dither" in L.afg_last_error()
    rc, res = decode(files, afgpu.BatchOpts(C.sizeof(afgpu.BatchOpts), 0, 0, None, afgpu.SAMPLE_PCM_S16, 3, 0))
    assert rc == -1 and b"dither" in L.afg_last_error()
    # a struct that ends before the two dither fields: they are not read, whatever lies there (and 7 is still refused)
    rc, res = decode(files, afgpu.BatchOpts(afgpu.BATCH_OPTS_SIZE_V2, 0, 0, None, 7, afgpu.DITHER_LIBC, 0))
    assert rc == -1 and b"sample_type" in L.afg_last_error()
