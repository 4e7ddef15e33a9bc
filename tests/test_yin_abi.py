"""The host half of the YIN pitch stage (include/afg.h: afg_yin_*, afg_batch_decode_pitch) through the C ABI: the helpers'
return values, every parameter refusal with its message, what the kernel entry checks without a device, struct_size
handling and the refusals of the batch options.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import afgpu
import yin_model as ym

INVALID = -1


def good_params(**kw):
    p = afgpu.yin_params(16000, 1024, 512, 160, 32, 320)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [(dict(frame_length=3, win_length=1, tau_min=1, tau_max=1), "frame_length"), (dict(frame_length=4097), "frame_length"),
              (dict(win_length=0), "win_length"), (dict(win_length=1023), "win_length"), (dict(hop=0), "hop"), (dict(tau_min=0), "tau_min"),
              (dict(tau_min=321), "tau_min"), (dict(tau_max=512), "tau_max"), (dict(center=2), "center"), (dict(pad_mode=2), "pad_mode"),
              (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=float("inf")), "threshold"),
              (dict(samplerate=0.0), "samplerate"), (dict(samplerate=-16000.0), "samplerate"), (dict(samplerate=float("inf")), "samplerate"),
              (dict(samplerate=float("nan")), "samplerate"), (dict(reserved=(C.c_uint32 * 2)(0, 1)), "reserved")]


def test_symbols_sizes_and_constants():
    lib = afgpu.lib()
    for name in ("afg_yin_lags", "afg_yin_frames", "afg_yin_layout", "afg_yin_hip", "afg_batch_decode_pitch"):
        assert hasattr(lib, name) and name in afgpu.ABI_SYMBOLS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "afg.h")).read()
    assert C.sizeof(afgpu.YinParams) == 48 and afgpu.YinParams.samplerate.offset == 32 and afgpu.YinParams.reserved.offset == 40
    assert C.sizeof(afgpu.PitchOpts) == 104 and afgpu.PitchOpts.n_out.offset == 44 and afgpu.PitchOpts.yin.offset == 48
    assert afgpu.PitchOpts.reserved.offset == 96
    assert (afgpu.YIN_TILE, afgpu.YIN_CHUNK) == (4, ym.CHUNK)
    assert "#define AFG_YIN_TILE  4" in header and "#define AFG_YIN_CHUNK 16" in header
    assert lib.afg_abi_version() == 2                            # additions only


def test_lags_are_librosas():
    lib = afgpu.lib()
    for args in ((22050, 65.40639132514966, 2093.004522404789, 2048, 1024), (16000, 50, 500, 1024, 512), (16000, 20, 500, 1024, 512),
                 (44100, 440, 441, 2048, 1024), (8000, 80, 400, 512, 256), (16000, 50, 500, 4096, 1)):
        assert afgpu.yin_lags(*args) == ym.lags(*args), args
    lo, hi = C.c_uint32(77), C.c_uint32(78)
    for args, word in (((16000, 50, 50000, 1024, 512), "no lag"), ((16000, 500, 600, 64, 61), "no lag"), ((16000, 500, 50, 1024, 512), "fmin"),
                       ((16000, 0, 500, 1024, 512), "fmin"), ((16000, 50, float("inf"), 1024, 512), "fmin"), ((16000, float("nan"), 500, 1024, 512), "fmin"),
                       ((0, 50, 500, 1024, 512), "samplerate"), ((float("nan"), 50, 500, 1024, 512), "samplerate"), ((16000, 50, 500, 3, 1), "frame_length"),
                       ((16000, 50, 500, 4097, 1), "frame_length"), ((16000, 50, 500, 1024, 0), "win_length"), ((16000, 50, 500, 1024, 1023), "win_length")):
        assert lib.afg_yin_lags(*map(float, args[:3]), *args[3:], C.byref(lo), C.byref(hi)) == INVALID, args
        assert lib.afg_last_error().decode().startswith("afg_yin_lags:") and word in lib.afg_last_error().decode(), args
        assert (lo.value, hi.value) == (77, 78)                  # nothing stored
        with pytest.raises(afgpu.AfgError, match=word):
            afgpu.yin_lags(*args)
    assert lib.afg_yin_lags(16000.0, 50.0, 500.0, 1024, 512, None, C.byref(hi)) == INVALID and "NULL" in lib.afg_last_error().decode()


def test_frames_and_layout():
    lib = afgpu.lib()
    p = good_params()                                            # centred: pad 512
    assert [afgpu.yin_frames(p, n) for n in (0, 1, 159, 160, 16000, 480000)] == [1, 1, 1, 2, 101, 3001]
    q = good_params(center=0)
    assert [afgpu.yin_frames(q, n) for n in (0, 1023, 1024, 1183, 1184, 16000, 2 ** 32 - 1)] == [0, 0, 1, 1, 2, 94, 1 + (2 ** 32 - 1 - 1024) // 160]
    r = good_params(hop=5000)                                    # a hop beyond the frame
    assert [afgpu.yin_frames(r, n) for n in (4999, 5000, 10000)] == [1, 2, 3]
    for n in (0, 1, 700, 16000):
        for prm, model in ((p, ym.params(16000, 1024, 512, 160)), (q, ym.params(16000, 1024, 512, 160, center=0))):
            assert afgpu.yin_frames(prm, n) == ym.n_frames(n, model)
    assert lib.afg_yin_frames(None, 16000) == 0 and "NULL params" in lib.afg_last_error().decode()
    rows = np.zeros(5, afgpu.MEL_ROW_DTYPE)
    rows["out_frames"] = [0, 4, 5, 1, 3]
    assert afgpu.yin_layout(rows, p) == 5 and list(rows["first_tile"]) == [0, 0, 1, 3, 4]
    assert lib.afg_yin_layout(None, 0, C.byref(p)) == 0
    for kw, word in BAD_PARAMS:
        bad = good_params(**kw)
        assert afgpu.yin_frames(bad, 16000) == 0 and lib.afg_last_error().decode().startswith(f"afg_yin_frames: {word}"), kw
        assert afgpu.yin_layout(rows, bad) == 0 and lib.afg_last_error().decode().startswith(f"afg_yin_layout: {word}"), kw
    for ok in (dict(frame_length=4, win_length=1, tau_min=1, tau_max=2), dict(frame_length=4096, win_length=1, tau_min=1, tau_max=4094),
               dict(win_length=1022, tau_min=1, tau_max=1), dict(threshold=0.0), dict(hop=2 ** 32 - 1)):
        assert afgpu.yin_frames(good_params(**ok), 100000) >= 1, ok


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = good_params()
    assert lib.afg_yin_hip(0, None, 0, C.byref(p), None, 0, None, 0, None) == 0           # n_rows == 0 is AFG_OK
    assert lib.afg_yin_hip(0, None, 0, None, None, 0, None, 0, None) == INVALID and "NULL params" in lib.afg_last_error().decode()
    for kw, word in BAD_PARAMS:
        assert lib.afg_yin_hip(1, 0x1000, 1, C.byref(good_params(**kw)), 0x2000, 8, 0x5000, 8, None) == INVALID
        assert lib.afg_last_error().decode().startswith(f"afg_yin_hip: {word}"), kw
        assert lib.afg_yin_hip(0, None, 0, C.byref(good_params(**kw)), None, 0, None, 0, None) == INVALID   # also without rows
    for args in ((1, None, 1, C.byref(p), 0x2000, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, None, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2002, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x5001, 8, None),
                 (1 << 32, 0x1000, 1, C.byref(p), 0x2000, 8, 0x5000, 8, None), (1, 0x1000, 1 << 31, C.byref(p), 0x2000, 8, 0x5000, 8, None)):
        assert lib.afg_yin_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_yin_hip:")


def call(n_files, opts, d_out=0x1000):
    """the batch entry with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    counts = np.full(1, 77, np.uint32)
    rc = lib.afg_batch_decode_pitch(ptrs, lens, n_files, C.byref(opts) if opts is not None else None, d_out, counts.ctypes.data, C.byref(res))
    assert counts[0] == 77
    return rc, lib.afg_last_error().decode(), res


def good_opts(yin=None, **kw):
    o = afgpu.PitchOpts(C.sizeof(afgpu.PitchOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, good_params(**(yin or {})), 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_batch_entry_refuses_before_any_device_call():
    cases = {
        "no opts": (call(1, None), "NULL opts"),
        "no d_out": (call(1, good_opts(), d_out=None), "NULL d_out"),
        "short struct": (call(1, good_opts(struct_size=C.sizeof(afgpu.PitchOpts) - 8)), "struct_size"),
        "resample's struct": (call(1, good_opts(struct_size=C.sizeof(afgpu.ResampleOpts))), "struct_size"),
        "reserved": (call(1, good_opts(reserved=1)), "afg_pitch_opts.reserved"),
        "channels": (call(1, good_opts(channels=0)), "channels"),
        "mono with two channels": (call(1, good_opts(channels=2)), "mono"),
        "another rate": (call(1, good_opts(yin=dict(samplerate=22050.0))), "yin.samplerate"),
        "no frame": (call(1, good_opts(yin=dict(center=0), frames=1023)), "no frame"),
        "reflect": (call(1, good_opts(yin=dict(pad_mode=afgpu.MEL_PAD_REFLECT), frames=512)), "reflect padding"),
        "n_out": (call(1, good_opts(n_out=102)), "n_out"),
    }
    for kw, word in BAD_PARAMS:
        if "samplerate" not in kw:
            cases[f"params {kw}"] = (call(1, good_opts(yin=kw)), f"afg_batch_decode_pitch: {word}")
    for what, ((rc, msg, res), word) in cases.items():
        assert rc == INVALID and word in msg, (what, rc, msg)
        assert res.n_files == 0 and not res.items
    for o in (good_opts(), good_opts(n_out=101), good_opts(struct_size=C.sizeof(afgpu.PitchOpts) + 64),
              good_opts(yin=dict(pad_mode=afgpu.MEL_PAD_REFLECT), frames=513)):
        rc, _, res = call(0, o)                                  # no file at all touches nothing
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entries_check_their_arguments():
    with pytest.raises(ValueError, match="no frame"):
        afgpu.batch_decode_pitch([b"x"], 1000, 16000, 50, 500, frame_length=1024, center=False)
    with pytest.raises(ValueError, match="n_out"):
        afgpu.batch_decode_pitch([b"x"], 16000, 16000, 50, 500, n_out=99)
    with pytest.raises(afgpu.AfgError, match="no lag"):
        afgpu.batch_decode_pitch([b"x"], 16000, 16000, 50, 50000)
    with pytest.raises(afgpu.AfgError, match="frame_length"):
        afgpu.batch_decode_pitch([b"x"], 16000, 16000, 50, 500, frame_length=8192)
    with pytest.raises(afgpu.AfgError, match="threshold"):
        afgpu.batch_decode_pitch([b"x"], 16000, 16000, 50, 500, threshold=-1.0)
    with pytest.raises(ValueError, match="mono"):
        afgpu.batch_decode_pitch([b"x"], 16000, 16000, 50, 500, channels=2)
    with pytest.raises(ValueError, match="tau_min and tau_max"):
        afgpu.yin_params(16000)
