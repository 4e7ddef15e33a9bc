"""afg_biquad_design / afg_filter_bound / afg_filter_check_rows / afg_filter_hip / afg_batch_decode_filtered without a GPU: the
symbols, the structures, the helper and the bound against tests/filter_model.py, and every refusal that needs no device, each
with its status and message."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import filter_model as fm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_biquad_design", "afg_filter_bound", "afg_filter_tile_frames", "afg_filter_check_rows", "afg_filter_hip", "afg_batch_decode_filtered")
INVALID = -1
HP = fm.design("highpass", 48000.0, 20.0)


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
        assert re.search(rf"\b{name}\s*\(", d), name                                         # the D prototypes
        assert name in afgpu.ABI_SYMBOLS
    assert code.index("afg_batch_decode_trimmed(") < min(code.index(n + "(") for n in NEW)    # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    consts = {"AFG_FILTER_TILE": afgpu.FILTER_TILE, "AFG_FILTER_CHUNK": afgpu.FILTER_CHUNK, "AFG_FILTER_K": afgpu.FILTER_K,
              "AFG_FILTER_MAX_SECTIONS": afgpu.FILTER_MAX_SECTIONS}
    consts.update({"AFG_BIQUAD_" + k.upper(): v for k, v in afgpu.BIQUAD_KINDS.items()})
    for const, value in consts.items():
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
    assert (afgpu.FILTER_TILE, afgpu.FILTER_CHUNK, afgpu.FILTER_K, afgpu.FILTER_MAX_SECTIONS) == (fm.TILE, fm.CHUNK, fm.K, fm.MAX_SECTIONS)
    assert lib.afg_filter_tile_frames() == fm.TILE == 256 * fm.CHUNK
    assert tuple(afgpu.BIQUAD_KINDS) == fm.KINDS
    for name in ("Biquad", "FilterParams", "FILTER_ROW_DTYPE", "biquad", "filter_params", "filter_bound", "filter_check_rows", "filter_rows",
                 "filter_tensor", "batch_decode_tensor_filtered"):
        assert hasattr(afgpu, name), name


def test_structures_match_the_header():
    for struct, cls, size in (("afg_biquad", afgpu.Biquad, 40), ("afg_filter_params", afgpu.FilterParams, 328)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
    names = list(afgpu.FILTER_ROW_DTYPE.names)
    got, offs = c_layout("afg_filter_row", names)
    assert got == afgpu.FILTER_ROW_DTYPE.itemsize == fm.ROW_DTYPE.itemsize == 24
    assert offs == [afgpu.FILTER_ROW_DTYPE.fields[n][1] for n in names] == [fm.ROW_DTYPE.fields[n][1] for n in names]
    assert C.sizeof(afgpu.ResampleOpts) == c_layout("afg_resample_opts", ["struct_size"])[0]


def test_design_helper_is_the_models():
    for fs, f0, q, db in ((48000.0, 20.0, math.sqrt(0.5), 0.0), (16000.0, 1000.0, 2.0, 6.0), (16000.0, 7000.0, 0.5, -9.0), (1.0, 0.45, 8.0, 3.0),
                          (44100.0, 22049.0, 0.3, 12.0), (96000.0, 0.5, 5.0, -3.0)):
        for kind in fm.KINDS:
            f = 0.97 if kind == "preemphasis" else f0
            got, want = afgpu.biquad(kind, fs, f, q, db), fm.design(kind, fs, f, q, db)
            for g, w in zip(got, want):
                assert abs(g - w) <= 1e-15 * abs(w), (kind, fs, f0, got, want)
            assert fm.stable(got)
    assert afgpu.biquad("preemphasis", f0=0.97) == (1.0, -0.97, 0.0, 0.0, 0.0)
    assert afgpu.biquad("dc_block", 48000.0, 30.0)[:3] == (1.0, -1.0, 0.0)
    lib = afgpu.lib()
    out = afgpu.Biquad(7.0, 7.0, 7.0, 7.0, 7.0)
    seen = set()
    for args in ((10, 48000.0, 100.0, 1.0, 0.0), (0, 48000.0, 0.0, 1.0, 0.0), (0, 48000.0, 24000.0, 1.0, 0.0), (1, 48000.0, -5.0, 1.0, 0.0),
                 (0, 48000.0, float("nan"), 1.0, 0.0), (0, 0.0, 100.0, 1.0, 0.0), (0, float("inf"), 100.0, 1.0, 0.0), (2, 48000.0, 100.0, 0.0, 0.0),
                 (2, 48000.0, 100.0, -1.0, 0.0), (3, 48000.0, 100.0, float("nan"), 0.0), (5, 48000.0, 100.0, 1.0, float("inf")),
                 (6, 48000.0, 100.0, 1.0, float("nan")), (8, 1.0, 1.5, 1.0, 0.0), (8, 1.0, float("nan"), 1.0, 0.0), (9, 48000.0, 24000.0, 1.0, 0.0)):
        assert lib.afg_biquad_design(*args, C.byref(out)) == INVALID, args
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_biquad_design:"), msg
        seen.add(msg.split(":")[1].split()[0])
        assert out.b0 == 7.0 and out.a2 == 7.0                  # untouched
    assert seen == {"kind", "f0", "samplerate", "q", "gain_db", "pre-emphasis"}
    assert lib.afg_biquad_design(0, 48000.0, 100.0, 1.0, 0.0, None) == INVALID and "NULL" in lib.afg_last_error().decode()
    assert lib.afg_biquad_design(0, 48000.0, 100.0, 1.0, float("nan"), C.byref(out)) == 0      # gain_db is not looked at by a low-pass
    with pytest.raises(ValueError):
        afgpu.biquad("brickwall", 48000.0, 100.0)
    with pytest.raises(ValueError):
        afgpu.biquad("lowpass", 48000.0, 30000.0)


CASCADES = [[fm.design("preemphasis", f0=0.97)], [HP], [fm.design("lowpass", 48000.0, 50.0, 5.0)],
            [fm.design("highpass", 16000.0, 80.0), fm.design("peaking", 16000.0, 1000.0, 2.0, 6.0), fm.design("lowpass", 16000.0, 7000.0)],
            [fm.design("lowpass", 1.0, 0.45, 8.0)], [fm.design("dc_block", 48000.0, 5.0)],
            [fm.design("lowpass", 1.0, 0.1, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / 32.0))) for k in range(8)]]


def test_bound_is_the_models():
    for sos in CASCADES:
        got, want = afgpu.filter_bound(sos), fm.bound(sos)
        assert abs(got - want) <= 1e-9 * want, (sos, got, want)
    six = [(s[0], s[1], s[2], 1.0, s[3], s[4]) for s in CASCADES[3]]                         # scipy's rows
    assert afgpu.filter_bound(six) == afgpu.filter_bound(CASCADES[3])
    with pytest.raises(ValueError):
        afgpu.filter_params([(1.0, 0.0, 0.0, 2.0, 0.0, 0.0)])


def params(sos, n=None):
    p = afgpu.filter_params(sos)
    if n is not None:
        p.n_sections = n
    return p


BAD_CASCADES = {
    "n_sections 0": params([HP], 0),
    "n_sections 9": params([HP], 9),
    "a pole on the circle": params([HP, (1.0, 0.0, 0.0, -2.0, 1.0)]),
    "a2 of 1": params([(1.0, 0.0, 0.0, 0.0, 1.0)]),
    "a2 of -1": params([(1.0, 0.0, 0.0, 0.0, -1.0)]),
    "a1 too large": params([(1.0, 0.0, 0.0, 1.6, 0.5)]),
    "a NaN": params([(1.0, float("nan"), 0.0, 0.0, 0.0)]),
    "an infinity": params([HP, HP, (float("inf"), 0.0, 0.0, 0.0, 0.0)]),
    "a NaN pole": params([(1.0, 0.0, 0.0, float("nan"), 0.0)]),
    "the bound's cap": params([(2048.0, 0.0, 0.0, 0.0, 0.0)] * 8),
}


def test_every_cascade_refusal_needs_no_device():
    lib = afgpu.lib()
    seen = {}
    for what, p in BAD_CASCADES.items():
        assert lib.afg_filter_bound(C.byref(p)) == 0.0, what
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_filter_params." if "cap" not in what else "afg_filter_bound:"), (what, msg)
        seen[what] = msg
        # the same answer from the row check, the kernel entry and the batch entry
        assert lib.afg_filter_check_rows(None, 0, C.byref(p), 0, 0, 0) == INVALID and lib.afg_last_error().decode() == msg
        assert lib.afg_filter_hip(0, None, C.byref(p), None, 0, None, 0, None, None) == INVALID and lib.afg_last_error().decode() == msg
        rc, got, _ = call_filtered(1, resample_opts(), p)
        assert rc == INVALID and got == msg
    assert "n_sections 0" in seen["n_sections 0"] and "n_sections 9" in seen["n_sections 9"]
    assert "sec[1]" in seen["a pole on the circle"] and "unit circle" in seen["a2 of 1"] and "not finite" in seen["a NaN"]
    assert "sec[2]" in seen["an infinity"] and "2^30" in seen["the bound's cap"]
    assert lib.afg_filter_bound(None) == 0.0 and "NULL" in lib.afg_last_error().decode()
    assert lib.afg_filter_check_rows(None, 0, None, 0, 0, 0) == INVALID
    sections_beyond = params([HP, (float("nan"),) * 5], 1)      # sec[n_sections ..] are not looked at
    assert lib.afg_filter_bound(C.byref(sections_beyond)) == afgpu.filter_bound([HP])
    assert afgpu.filter_bound([(2048.0, 0.0, 0.0, 0.0, 0.0)] * 7) > 0.0
    with pytest.raises(ValueError):
        afgpu.filter_bound([(2048.0, 0.0, 0.0, 0.0, 0.0)] * 8)


def rows_of(spec):
    r = np.zeros(len(spec), afgpu.FILTER_ROW_DTYPE)
    for k, (a, b, n) in enumerate(spec):
        r[k]["in_off"], r[k]["out_off"], r[k]["frames"] = a, b, n
    return r


def refused(rows, in_floats, out_floats, same_plane):
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.filter_check_rows(rows, [HP], in_floats, out_floats, same_plane)
    return str(e.value).split("): ", 1)[1]


def test_every_row_refusal_needs_no_device():
    good = rows_of([(0, 0, 100), (100, 100, 0), (150, 150, 50), (200, 300, 50), (200, 400, 50), (2 ** 64 - 1, 2 ** 64 - 1, 0)])
    afgpu.filter_check_rows(good, [HP], 500, 500, True)         # in place, empty rows anywhere, one input read twice
    afgpu.filter_check_rows(rows_of([(0, 0, 100), (50, 100, 100)]), [HP], 500, 500, False)    # two planes: only the outputs count
    afgpu.filter_check_rows(rows_of([(0, 0, 0xffffffff)]), [HP], 0xffffffff, 0xffffffff, True)
    seen = set()
    for spec, fl, same in (
            ([(401, 0, 100)], (500, 500), False),                # a row leaves the input ...
            ([(0, 401, 100)], (500, 500), False),                # ... the output
            ([(2 ** 64 - 50, 0, 100)], (500, 500), False),       # ... by an offset that would wrap
            ([(0, 2 ** 64 - 50, 100)], (500, 500), False),
            ([(0, 0, 100)], (99, 500), False),
            ([(0, 0, 100), (200, 50, 100)], (500, 500), False),  # two outputs overlap
            ([(0, 0, 100), (0, 0, 100)], (500, 500), True),      # ... the same row twice in place
            ([(0, 1, 100)], (500, 500), True),                   # a row shifted by one onto itself
            ([(0, 100, 100), (150, 300, 100)], (500, 500), True),    # an output over another row's input
            ([(100, 0, 100), (150, 150, 100)], (500, 500), True),    # an input over a row that runs in place
            ([(0, 99, 100)], (500, 500), True)):
        msg = refused(rows_of(spec), fl[0], fl[1], same)
        assert msg.startswith("afg_filter_row"), msg
        seen.add(re.sub(r"\d+", "#", msg))
    assert len(seen) == 3                                        # the input, the output, an overlap
    bad = rows_of([(0, 0, 10)])
    bad[0]["reserved"] = 1
    assert "reserved" in refused(bad, 500, 500, False)
    assert afgpu.lib().afg_filter_check_rows(None, 1, C.byref(params([HP])), 10, 10, 0) == INVALID


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = params([HP])
    assert lib.afg_filter_hip(0, None, C.byref(p), None, 0, None, 0, None, None) == 0               # no rows: nothing to do
    assert lib.afg_filter_hip(0, None, None, None, 0, None, 0, None, None) == INVALID
    good = (1, 0x1000, C.byref(p), 0x20000, 1000, 0x30000, 1000, 0x4000, None)
    seen = set()
    for at, value in ((1, None), (3, None), (5, None), (1, 0x1004), (3, 0x20002), (5, 0x30001), (7, 0x4004), (0, 1 << 31), (4, 1 << 61), (6, 1 << 61),
                      (5, 0x20000 + 3996), (5, 0x20000 - 3996)):
        args = list(good)
        args[at] = value
        assert lib.afg_filter_hip(*args) == INVALID, (at, value)
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_filter_hip:"), (at, msg)
        seen.add(msg)
    assert len(seen) == 5                                        # NULL, alignment, the launch's cap, a plane's size, overlap


def resample_opts(**kw):
    o = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def call_filtered(n_files, opts, flt, d_out=0x1000, out=True):
    """afg_batch_decode_filtered with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_filtered(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if flt is None else C.byref(flt), d_out,
                                       C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def test_batch_entry_refuses_its_arguments_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    p, neg = params([HP]), (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call_filtered(1, None, p),
        "NULL filter": call_filtered(1, resample_opts(), None),
        "NULL d_out": call_filtered(1, resample_opts(), p, d_out=None),
        "NULL out": call_filtered(1, resample_opts(), p, out=False),
        # what afg_batch_decode_resampled refuses
        "short struct": call_filtered(1, resample_opts(struct_size=C.sizeof(afgpu.ResampleOpts) - 8), p),
        "no channels": call_filtered(1, resample_opts(channels=0), p),
        "no frames": call_filtered(1, resample_opts(frames=0), p),
        "samplerate": call_filtered(1, resample_opts(samplerate=0), p),
        "mono with two channels": call_filtered(1, resample_opts(channels=2), p),
        "in_channels": call_filtered(1, resample_opts(in_channels=1 << 16), p),
        "max_in_rate": call_filtered(1, resample_opts(max_in_rate=(1 << 20) + 1), p),
        "lowpass_width": call_filtered(1, resample_opts(lowpass_width=65), p),
        "negative n_files": call_filtered(-1, resample_opts(), p),
        "negative first_frame": call_filtered(1, resample_opts(first_frame=neg), p),
        "a scratch row too long": call_filtered(1, resample_opts(samplerate=8000, frames=0xffffffff), p),
        # the cascade
        "n_sections": call_filtered(1, resample_opts(), params([HP], 0)),
        "unstable": call_filtered(1, resample_opts(), params([(1.0, 0.0, 0.0, -2.0, 1.0)])),
        "not finite": call_filtered(1, resample_opts(), params([(float("inf"), 0.0, 0.0, 0.0, 0.0)])),
        "the bound's cap": call_filtered(1, resample_opts(), BAD_CASCADES["the bound's cap"]),
    }
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    rc, _, res = call_filtered(0, resample_opts(), p)            # no file: nothing is touched
    assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entry_checks_its_arguments():
    for kw in (dict(frames=0), dict(channels=0), dict(samplerate=0), dict(channels=2, mono=True), dict(sos=[(1.0, 0.0, 0.0, -2.0, 1.0)]),
               dict(sos=[HP] * 9), dict(sos=[(2048.0, 0.0, 0.0, 0.0, 0.0)] * 8)):
        args = dict(frames=16000, channels=1, samplerate=16000, sos=[HP])
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_filtered([b"x"], **args)
