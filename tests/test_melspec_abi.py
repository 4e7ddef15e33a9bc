"""afg_mel_basis / afg_mel_filters / afg_mel_layout / afg_melspec_hip / afg_batch_decode_mel without a GPU: the symbols, the
record and option layouts, the tables against tests/melspec_model.py, and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import melspec_model as mm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_mel_basis", "afg_mel_filters", "afg_mel_frames", "afg_mel_layout", "afg_mel_check_rows", "afg_melspec_hip", "afg_batch_decode_mel")
INVALID = -1


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
    # appended behind the resampled entry; the ABI version is unchanged
    assert code.index("afg_batch_decode_resampled(") < min(code.index(n + "(") for n in NEW)
    assert lib.afg_abi_version() == 2
    assert "reference has no such stage" in header
    for const, value in (("AFG_MEL_PAD_REFLECT", afgpu.MEL_PAD_REFLECT), ("AFG_MEL_PAD_ZERO", afgpu.MEL_PAD_ZERO), ("AFG_MEL_POWER", afgpu.MEL_POWER),
                         ("AFG_MEL_LOG10", afgpu.MEL_LOG10), ("AFG_MEL_SCALE_SLANEY", afgpu.MEL_SCALE_SLANEY), ("AFG_MEL_SCALE_HTK", afgpu.MEL_SCALE_HTK),
                         ("AFG_MEL_NORM_NONE", afgpu.MEL_NORM_NONE), ("AFG_MEL_NORM_SLANEY", afgpu.MEL_NORM_SLANEY)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
        assert getattr(mm, const[8:]) == value


def test_record_and_option_layouts_match_the_header():
    names = list(afgpu.MEL_ROW_DTYPE.names)
    size, offs = c_layout("afg_mel_row", names)
    assert size == afgpu.MEL_ROW_DTYPE.itemsize == 32
    assert offs == [afgpu.MEL_ROW_DTYPE.fields[n][1] for n in names]
    names = [f[0] for f in afgpu.MelParams._fields_]
    assert names == ["n_fft", "win_length", "hop", "n_mels", "center", "pad_mode", "out_kind", "log_floor"]
    size, offs = c_layout("afg_mel_params", names)
    assert size == C.sizeof(afgpu.MelParams) == 32
    assert offs == [getattr(afgpu.MelParams, n).offset for n in names]
    names = [f[0] for f in afgpu.MelOpts._fields_]
    assert names[:10] == [f[0] for f in afgpu.ResampleOpts._fields_] and names[10:] == ["n_out", "mel", "scale", "norm", "f_min", "f_max"]
    size, offs = c_layout("afg_mel_opts", names)
    assert size == C.sizeof(afgpu.MelOpts)
    assert offs == [getattr(afgpu.MelOpts, n).offset for n in names]
    assert offs[:10] == [getattr(afgpu.ResampleOpts, n).offset for n in names[:10]]      # afg_resample_opts' fields where they are there


@pytest.mark.parametrize("n_fft,win", [(400, 400), (512, 400), (16, 16), (2048, 2048), (64, 1), (1024, 1023)])
def test_the_basis_is_the_models(n_fft, win):
    table = afgpu.mel_basis(n_fft, win)
    assert table.dtype == np.float32 and table.shape == (win, 2 * mm.nb16(n_fft))
    if (n_fft, win) == (400, 400):
        assert table.shape == (400, 416)
    Cf, Sf = mm.split_basis(table, n_fft)                        # (asserts the padding columns are +0.0f)
    C64, S64 = mm.basis64(n_fft, win)
    for got, want in ((Cf, C64), (Sf, S64)):
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    # the size alone; a buffer that is too small is left as it is
    lib = afgpu.lib()
    assert lib.afg_mel_basis(n_fft, win, None, 0) == table.size
    buf = np.full(table.size, 7, np.float32)
    assert lib.afg_mel_basis(n_fft, win, buf.ctypes.data, table.size - 1) == table.size and (buf == 7).all()


@pytest.mark.parametrize("args", [(16000, 400, 80, 0.0, 0.0, mm.SCALE_SLANEY, mm.NORM_SLANEY), (16000, 400, 80, 0.0, 0.0, mm.SCALE_HTK, mm.NORM_NONE),
                                  (22050, 1024, 128, 20.0, 8000.0, mm.SCALE_SLANEY, mm.NORM_SLANEY), (8000, 512, 23, 64.0, 3800.0, mm.SCALE_HTK, mm.NORM_SLANEY),
                                  (48000, 2048, 256, 0.0, 0.0, mm.SCALE_SLANEY, mm.NORM_NONE), (16000, 16, 1, 0.0, 0.0, mm.SCALE_HTK, mm.NORM_SLANEY)],
                         ids=lambda a: "-".join(str(int(v)) for v in a))
def test_the_bank_is_the_models(args):
    bank = afgpu.mel_filters(*args)
    want = mm.filters64(*args)
    assert bank.dtype == np.float32 and bank.shape == want.shape == (args[2], args[1] // 2 + 1)
    assert (np.abs(bank.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12).all()
    assert (bank >= 0).all()
    lib = afgpu.lib()
    buf = np.full(bank.size, 7, np.float32)
    assert lib.afg_mel_filters(*args, buf.ctypes.data, bank.size - 1) == bank.size and (buf == 7).all()


def test_table_refusals():
    lib = afgpu.lib()
    seen = set()
    for args in ((15, 15), (2049, 400), (400, 0), (400, 401)):
        assert lib.afg_mel_basis(*args, None, 0) == 0
        seen.add(lib.afg_last_error().decode())
        with pytest.raises(afgpu.AfgError):
            afgpu.mel_basis(*args)
    good = [16000, 400, 80, 0.0, 0.0, 0, 1]
    for at, value in ((0, 0), (1, 15), (1, 2049), (2, 0), (2, 257), (3, -1.0), (3, 8000.0), (4, 8000.5), (5, 2), (6, 2), (3, float("nan"))):
        args = list(good)
        args[at] = value
        assert lib.afg_mel_filters(*args, None, 0) == 0, args
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_mel_filters:")
        seen.add(msg)
        with pytest.raises(afgpu.AfgError):
            afgpu.mel_filters(*args)
    assert len(seen) >= 12


def good_params(**kw):
    p = afgpu.mel_params(400, 160, 80, None, True, afgpu.MEL_PAD_REFLECT, afgpu.MEL_LOG10, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [dict(n_fft=15), dict(n_fft=2049, win_length=400), dict(win_length=0), dict(win_length=401), dict(hop=0), dict(hop=401),
              dict(n_mels=0), dict(n_mels=257), dict(center=2), dict(pad_mode=2), dict(out_kind=2), dict(log_floor=-1.0),
              dict(log_floor=float("nan")), dict(log_floor=float("inf"))]


def test_frames_and_layout():
    p = good_params()
    assert [afgpu.mel_frames(p, n) for n in (0, 1, 159, 160, 480000)] == [1, 1, 1, 2, 3001]
    assert afgpu.mel_frames(good_params(center=0), 399) == 0 and afgpu.mel_frames(good_params(center=0), 400) == 1
    assert afgpu.mel_frames(good_params(n_fft=401, win_length=401), 0) == 0           # 2 * (401 / 2) - 401 is negative
    rows = np.zeros(5, afgpu.MEL_ROW_DTYPE)
    rows["out_frames"] = [64, 65, 0, 1, 3000]
    assert afgpu.mel_layout(rows, p) == 1 + 2 + 0 + 1 + 47                            # tiles of 64 frames
    assert list(rows["first_tile"]) == [0, 1, 3, 3, 4]
    big = good_params(n_fft=2048, win_length=2048, hop=2048, n_mels=256, center=0)
    assert afgpu.mel_layout(rows, big) == 4 + 5 + 0 + 1 + 188                          # ... of 16
    assert afgpu.mel_layout(rows, good_params(n_fft=1024, win_length=1024, hop=256, n_mels=128)) == 2 + 3 + 0 + 1 + 94      # ... of 32
    lib = afgpu.lib()
    for kw in BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_mel_layout(rows.ctypes.data, len(rows), C.byref(bad)) == 0 and lib.afg_last_error().decode().startswith("afg_mel_params.")
        assert lib.afg_mel_frames(C.byref(bad), 1000) == 0


def records(p, lengths, frames=None):
    """rows laid out back to back, with every frame they have unless `frames` says otherwise; (rows, tiles, in_floats, out_floats)"""
    rows = np.zeros(len(lengths), afgpu.MEL_ROW_DTYPE)
    i = o = 0
    for k, n in enumerate(lengths):
        f = afgpu.mel_frames(p, n) if frames is None else frames[k]
        rows[k]["in_off"], rows[k]["out_off"], rows[k]["in_frames"], rows[k]["out_frames"] = i, o, n, f
        i += n
        o += p.n_mels * f
    return rows, afgpu.mel_layout(rows, p), i, o


def test_every_record_refusal_needs_no_device():
    lib = afgpu.lib()
    p = good_params()
    basis, bank = 400 * 416, 80 * 201
    rows, tiles, nin, nout = records(p, [2000, 201, 700, 48000])
    afgpu.mel_check_rows(rows, tiles, p, nin, basis, bank, nout)                      # as it stands it passes
    afgpu.mel_check_rows(rows[:0], 0, p, 0, 0, 0, 0)                                   # no rows: the parameters alone
    seen = set()

    def refused(change=None, prm=p, **kw):
        bad = rows.copy()
        if change:
            change(bad)
        a = dict(tiles=tiles, nin=nin, basis=basis, bank=bank, nout=nout)
        a.update(kw)
        rc = lib.afg_mel_check_rows(bad.ctypes.data, len(bad), a["tiles"], C.byref(prm), a["nin"], a["basis"], a["bank"], a["nout"])
        msg = lib.afg_last_error().decode()
        assert rc == INVALID and msg, (rc, msg)
        seen.add(msg)

    for kw in BAD_PARAMS:                                                             # each parameter out of range
        refused(prm=good_params(**kw))
    n = len(seen)
    assert n == len(BAD_PARAMS)
    refused(lambda b: b["in_frames"].__setitem__(1, 200), nin=nin + 1000)             # reflect with in_frames <= pad ...
    assert "reflect" in lib.afg_last_error().decode() or "frames" in lib.afg_last_error().decode()
    one = records(p, [200], [1])
    assert lib.afg_mel_check_rows(one[0].ctypes.data, 1, one[1], C.byref(p), 200, basis, bank, 80) == INVALID
    assert "reflect" in lib.afg_last_error().decode()                                  # ... seen on its own: 200 samples do have a frame
    zero = good_params(pad_mode=afgpu.MEL_PAD_ZERO)
    assert lib.afg_mel_check_rows(one[0].ctypes.data, 1, one[1], C.byref(zero), 200, basis, bank, 80) == 0
    silent = records(p, [200], [0])
    assert lib.afg_mel_check_rows(silent[0].ctypes.data, 1, 0, C.byref(p), 200, basis, bank, 0) == 0     # no output, nothing to reflect
    refused(lambda b: b["out_frames"].__setitem__(2, 6))                               # out_frames > max_frames (700 samples: 5)
    assert "out_frames" in lib.afg_last_error().decode()
    refused(nin=nin - 1)                                                               # planes overrun
    refused(nout=nout - 1)
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(3, (1 << 64) - 8))
    refused(basis=basis - 1)
    refused(bank=bank - 1)
    refused(tiles=tiles + 1)                                                           # wrong tile count
    refused(lambda b: b["first_tile"].__setitem__(2, 0))
    assert len(seen) >= n + 9
    # fewer frames than the row has is fine (Whisper takes 3000 of 3001)
    rows2, tiles2, nin2, nout2 = records(p, [480000], [3000])
    afgpu.mel_check_rows(rows2, tiles2, p, nin2, basis, bank, nout2)


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = good_params()
    assert lib.afg_melspec_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, 0, None, 0, None) == 0           # no rows: nothing to do
    assert lib.afg_melspec_hip(0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None) == INVALID           # ... but the parameters are looked at
    for kw in BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_melspec_hip(1, 0x1000, 1, C.byref(bad), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None) == INVALID
        assert lib.afg_last_error().decode().startswith("afg_mel_params.")
    for args in ((1, None, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, None, 8, 0x4000, 8, 0x5000, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, None, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, None, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2002, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1 << 32, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None)):
        assert lib.afg_melspec_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_melspec_hip:")


def call(n_files, opts, d_out=0x1000, out=True, files=(b"x",)):
    """afg_batch_decode_mel with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    bufs = [bytes(f) for f in files]
    ptrs = (C.c_char_p * max(len(bufs), 1))(*bufs)
    lens = (C.c_size_t * max(len(bufs), 1))(*[len(b) for b in bufs])
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_mel(ptrs, lens, n_files, None if opts is None else C.byref(opts), d_out, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def good_opts(mel=None, **kw):
    o = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, good_params(**(mel or {})), 0, 1, 0.0, 0.0)
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
        "short struct": call(1, good_opts(struct_size=C.sizeof(afgpu.MelOpts) - 8)),
        # inherited from the resampled entry
        "no channels": call(1, good_opts(channels=0)),
        "no samplerate": call(1, good_opts(samplerate=0)),
        "samplerate too high": call(1, good_opts(samplerate=(1 << 20) + 1)),
        "mono with two channels": call(1, good_opts(channels=2)),
        "in_channels": call(1, good_opts(in_channels=65536)),
        "max_in_rate": call(1, good_opts(max_in_rate=(1 << 20) + 1)),
        "lowpass_width": call(1, good_opts(lowpass_width=65)),
        "negative first_frame": call(1, good_opts(first_frame=neg)),
        "negative n_files": call(-1, good_opts()),
        # the bank's
        "scale": call(1, good_opts(scale=2)),
        "norm": call(1, good_opts(norm=2)),
        "f_min": call(1, good_opts(f_min=9000.0)),
        "f_max": call(1, good_opts(f_max=8000.5)),
        # frames against the mel parameters
        "no frame": call(1, good_opts(mel=dict(center=0), frames=399)),
        "n_out": call(1, good_opts(n_out=102)),
        "reflect": call(1, good_opts(frames=200)),
    }
    for n, kw in enumerate(BAD_PARAMS):
        cases[f"mel {n}"] = call(1, good_opts(mel=kw))
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    # no file at all: ok, and nothing is touched (the address is made up); 101 frames of 16000 samples, or 100 of them
    for o in (good_opts(), good_opts(n_out=100), good_opts(n_out=101)):
        rc, _, res = call(0, o)
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entry_checks_its_arguments():
    for kw in (dict(frames=0), dict(frames=16000, samplerate=0), dict(frames=16000, channels=2), dict(frames=16000, n_out=102),
               dict(frames=399, center=False)):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mel([b"x"], **kw)
    assert afgpu.lib().afg_dev_option(b"mel_scratch_bytes", 1 << 20) == 0 and afgpu.lib().afg_dev_option(b"mel_scratch_bytes", -1) == 0
