"""afg_resample_taps / afg_resample_hip / afg_batch_decode_resampled without a GPU: the symbols, the record layouts, the
filter table against tests/resample_model.py, and the argument checks that come before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import resample_model as rm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_resample_taps", "afg_resample_layout", "afg_resample_hip", "afg_batch_decode_resampled")
INVALID = -1
PAIRS = [(44100, 16000), (48000, 16000), (44100, 48000), (8000, 16000), (22050, 16000), (44101, 16000)]


def test_symbols_are_exported_and_declared():
    lib = afgpu.lib()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "audio-formats_amd", "lib", "libafg_hip.so")], text=True)
    header = open(os.path.join(ROOT, "include", "afg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    d = open(os.path.join(ROOT, "bindings", "d", "afgpu.d")).read()
    d = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", d, flags=re.S))
    for name in NEW:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", exported), name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert re.search(rf"\b{name}\s*\(", d), name
        assert name in afgpu.ABI_SYMBOLS
    # appended behind the collate entry, which other tests read by position; the ABI version is unchanged
    assert code.index("afg_batch_decode_to_device(") < min(code.index(n + "(") for n in NEW)
    assert lib.afg_abi_version() == 2
    assert "reference has no resampler" in header


def test_record_layouts_match_the_header():
    names = list(afgpu.RESAMPLE_ROW_DTYPE.names)
    size, offs = c_layout("afg_resample_row", names)
    assert size == afgpu.RESAMPLE_ROW_DTYPE.itemsize == 72
    assert offs == [afgpu.RESAMPLE_ROW_DTYPE.fields[n][1] for n in names]
    assert afgpu.RESAMPLE_ROW_DTYPE["in_frame0"] == np.int64 and afgpu.RESAMPLE_ROW_DTYPE["in_frames"] == np.uint32
    names = [f[0] for f in afgpu.ResampleOpts._fields_]
    assert names == ["struct_size", "n_threads", "channels", "frames", "first_frame", "samplerate", "mono", "in_channels", "max_in_rate",
                     "lowpass_width"]
    size, offs = c_layout("afg_resample_opts", names)
    assert size == C.sizeof(afgpu.ResampleOpts)
    assert offs == [getattr(afgpu.ResampleOpts, n).offset for n in names]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_the_table_is_the_models(pair):
    taps, M, L, W = afgpu.resample_taps(*pair)
    assert (M, L, W) == rm.shape(*pair)[:3]
    want = rm.taps64(*pair)
    assert taps.dtype == np.float32 and taps.shape == want.shape == (L, 2 * W)
    assert (np.abs(taps.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    if pair == (44101, 16000):
        assert taps.size == 544000


def test_table_sizes_widths_and_equal_rates():
    lib = afgpu.lib()
    M, L, W = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
    # the size alone; a buffer that is too small is left as it is
    assert lib.afg_resample_taps(48000, 16000, 0, None, 0, C.byref(M), C.byref(L), C.byref(W)) == 38 and (M.value, L.value, W.value) == (3, 1, 19)
    buf = np.full(40, 7, np.float32)
    assert lib.afg_resample_taps(48000, 16000, 0, buf.ctypes.data, 37, None, None, None) == 38 and (buf == 7).all()
    assert lib.afg_resample_taps(48000, 16000, 0, buf.ctypes.data, 38, None, None, None) == 38 and (buf[38:] == 7).all() and (buf[:38] != 7).all()
    # another width: W follows Z
    taps, M_, L_, W_ = afgpu.resample_taps(44100, 16000, 16)
    assert W_ == rm.shape(44100, 16000, 16)[2] == 45
    assert (np.abs(taps - rm.taps64(44100, 16000, 16)) <= 2.0 ** -24 * np.abs(rm.taps64(44100, 16000, 16)) + 1e-12).all()
    # equal rates: no filter, and no error
    taps, M_, L_, W_ = afgpu.resample_taps(16000, 16000)
    assert taps.size == 0 and (M_, L_, W_) == (1, 1, 0)


def test_the_three_refusals():
    lib = afgpu.lib()
    seen = set()
    for args in ((0, 16000, 0), (16000, 0, 0), (44100, 16000, 65), (999983, 1000003, 0)):
        M, L, W = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
        assert lib.afg_resample_taps(*args, None, 0, C.byref(M), C.byref(L), C.byref(W)) == 0
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_resample_taps:") and (M.value, L.value, W.value) == (0, 0, 0)
        seen.add(msg)
        with pytest.raises(afgpu.AfgError):
            afgpu.resample_taps(*args)
    assert len(seen) == 4
    assert lib.afg_resample_taps(44100, 16000, 64, None, 0, None, None, None) == 160 * 2 * rm.shape(44100, 16000, 64)[2]     # 64 is allowed


def test_layout_gives_every_row_its_tiles():
    """1024 output frames per tile; 512 ... 64 while floor(tile * M / L) + 2 W + 1 input frames exceed 4096"""
    rows = np.zeros(7, afgpu.RESAMPLE_ROW_DTYPE)
    rows["M"], rows["L"], rows["W"] = [1, 441, 3, 3, 12, 12, 63], [1, 160, 1, 1, 1, 1, 1], [0, 17, 19, 19, 73, 73, 382]
    rows["out_frames"] = [1025, 1024, 1025, 0, 256, 257, 65]
    #                       1024      1024  1024   -    256   256  64 (and not staged)
    assert afgpu.resample_layout(rows) == 2 + 1 + 2 + 0 + 1 + 2 + 2
    assert list(rows["first_tile"]) == [0, 2, 3, 5, 5, 6, 8]


def call(n_files, opts, d_out=0x1000, out=True, files=(b"x",)):
    """afg_batch_decode_resampled with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    bufs = [bytes(f) for f in files]
    ptrs = (C.c_char_p * max(len(bufs), 1))(*bufs)
    lens = (C.c_size_t * max(len(bufs), 1))(*[len(b) for b in bufs])
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_resampled(ptrs, lens, n_files, None if opts is None else C.byref(opts), d_out, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def good_opts(**kw):
    o = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 16, None, 16000, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_argument_errors_come_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    neg = (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call(1, None),
        "NULL d_out": call(1, good_opts(), d_out=None),
        "NULL out": call(1, good_opts(), out=False),
        "short struct": call(1, good_opts(struct_size=afgpu.ResampleOpts.lowpass_width.offset)),
        "no channels": call(1, good_opts(channels=0)),
        "no frames": call(1, good_opts(frames=0)),
        "no samplerate": call(1, good_opts(samplerate=0)),
        "samplerate too high": call(1, good_opts(samplerate=(1 << 20) + 1)),
        "mono with two channels": call(1, good_opts(mono=1, channels=2)),
        "in_channels": call(1, good_opts(in_channels=65536)),
        "max_in_rate": call(1, good_opts(max_in_rate=(1 << 20) + 1)),
        "lowpass_width": call(1, good_opts(lowpass_width=65)),
        "negative first_frame": call(1, good_opts(first_frame=neg)),
        "negative n_files": call(-1, good_opts()),
        "scratch row": call(1, good_opts(frames=0xffffffff, samplerate=8000)),
    }
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    # no file at all: ok, and nothing is touched (the address is made up)
    rc, _, res = call(0, good_opts())
    assert rc == 0 and res.n_files == 0 and not res.items


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    assert lib.afg_resample_hip(0, None, 0, None, 0, None, 0, None, 0, None) == 0                 # no rows: nothing to do
    for args in ((1, None, 1, 0x1000, 8, 0x2000, 8, 0x3000, 8, None), (1, 0x1000, 1, 0x1000, 8, 0x2000, 8, None, 8, None),
                 (1, 0x1000, 1, 0x1002, 8, 0x2000, 8, 0x3000, 8, None), (1 << 32, 0x1000, 1, 0x1000, 8, 0x2000, 8, 0x3000, 8, None)):
        assert lib.afg_resample_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_resample_hip:")


def test_python_entry_checks_its_arguments():
    for kw in (dict(frames=0, channels=1, samplerate=16000), dict(frames=16, channels=0, samplerate=16000),
               dict(frames=16, channels=1, samplerate=0), dict(frames=16, channels=2, samplerate=16000, mono=True)):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_resampled([b"x"], **kw)
    assert afgpu.lib().afg_dev_option(b"resample_scratch_bytes", 1 << 20) == 0 and afgpu.lib().afg_dev_option(b"resample_scratch_bytes", -1) == 0
