"""The FFT path of the mel features without a GPU: the symbols, afg_mel_opts' layout, afg_mel_fft_tables against
tests/melspec_fft_model.py to the bit, and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import melspec_fft_model as fm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_mel_fft_tables", "afg_mel_fft_layout", "afg_mel_fft_check_rows", "afg_melspec_fft_hip")
INVALID, UNSUPPORTED = -1, -5


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
    for const, value in (("AFG_MEL_ALGO_DIRECT", afgpu.MEL_ALGO_DIRECT), ("AFG_MEL_ALGO_FFT", afgpu.MEL_ALGO_FFT)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
    assert (afgpu.MEL_ALGO_DIRECT, afgpu.MEL_ALGO_FFT) == (0, 1)
    assert lib.afg_abi_version() == 2
    for name in ("mel_fft_tables", "mel_fft_layout", "mel_fft_check_rows", "melspec_fft"):
        assert callable(getattr(afgpu, name))


def test_the_options_grew_at_their_end_and_the_parameters_did_not():
    names = [f[0] for f in afgpu.MelOpts._fields_] + ["algorithm", "reserved"]       # (_fields_: what positional arguments fill)
    assert len(names) == 18 and len(set(names)) == 18
    size, offs = c_layout("afg_mel_opts", names)
    assert size == C.sizeof(afgpu.MelOpts)
    assert offs == [getattr(afgpu.MelOpts, n).offset for n in names]
    assert offs[-2:] == [size - 8, size - 4]
    assert C.sizeof(afgpu.MelParams) == c_layout("afg_mel_params", ["n_fft"])[0] == 32
    # a positional construction without the new fields is the direct path
    o = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, afgpu.mel_params(), 0, 1, 0.0, 0.0)
    assert (o.algorithm, o.reserved) == (afgpu.MEL_ALGO_DIRECT, 0)
    o = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), algorithm=afgpu.MEL_ALGO_FFT, reserved=7)
    assert bytes(o)[-8:] == bytes([1, 0, 0, 0, 7, 0, 0, 0])


@pytest.mark.parametrize("n_fft,win", [(400, 400), (512, 400), (16, 16), (60, 45), (75, 75), (250, 250), (2048, 2048), (64, 1), (1024, 1023)])
def test_the_table_is_the_models_to_the_bit(n_fft, win):
    table = afgpu.mel_fft_tables(n_fft, win)
    want = fm.fft_tables32(n_fft, win)
    assert table.dtype == np.float32 and table.shape == want.shape == (win + 2 * n_fft,)
    assert (table.view(np.uint32) == want.view(np.uint32)).all()
    lib = afgpu.lib()
    assert lib.afg_mel_fft_tables(n_fft, win, None, 0) == table.size
    buf = np.full(table.size, 7, np.float32)
    assert lib.afg_mel_fft_tables(n_fft, win, buf.ctypes.data, table.size - 1) == table.size and (buf == 7).all()


def good_params(**kw):
    p = afgpu.mel_params(400, 160, 80, None, True, afgpu.MEL_PAD_REFLECT, afgpu.MEL_LOG10, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [dict(n_fft=15), dict(n_fft=2049, win_length=400), dict(win_length=0), dict(win_length=401), dict(hop=0), dict(hop=401),
              dict(n_mels=0), dict(n_mels=257), dict(center=2), dict(pad_mode=2), dict(out_kind=2), dict(log_floor=-1.0),
              dict(log_floor=float("nan")), dict(log_floor=float("inf"))]
ODD_N_FFT = [17, 77, 2047]


def test_sizes_the_path_does_not_take():
    lib = afgpu.lib()
    rows = np.zeros(1, afgpu.MEL_ROW_DTYPE)
    for n in ODD_N_FFT:
        assert not fm.supported(n)
        assert lib.afg_mel_fft_tables(n, n, None, 0) == 0 and "n_fft" in lib.afg_last_error().decode()
        with pytest.raises(afgpu.AfgError):
            afgpu.mel_fft_tables(n, n)
        p = good_params(n_fft=n, win_length=16, hop=16)
        assert lib.afg_mel_frames(C.byref(p), 4000) > 0                                # the direct path takes it
        assert lib.afg_mel_fft_layout(rows.ctypes.data, 1, C.byref(p)) == 0 and f"n_fft {n}" in lib.afg_last_error().decode()
        assert lib.afg_mel_fft_check_rows(rows.ctypes.data, 1, 0, C.byref(p), 0, 0, 0, 0) == UNSUPPORTED
        assert f"n_fft {n}" in lib.afg_last_error().decode()
        assert lib.afg_melspec_fft_hip(1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None) == UNSUPPORTED
        with pytest.raises(afgpu.AfgError, match="unsupported"):
            afgpu.mel_fft_check_rows(rows, 0, p, 0, 0, 0, 0)
    for args in ((15, 15), (2049, 400), (400, 0), (400, 401)):
        assert lib.afg_mel_fft_tables(*args, None, 0) == 0 and lib.afg_last_error().decode().startswith("afg_mel_fft_tables:")
    for n in (16, 75, 400, 480, 512, 800, 960, 1024, 2048):
        assert lib.afg_mel_fft_tables(n, n, None, 0) == 3 * n


def records(p, lengths, frames=None):
    rows = np.zeros(len(lengths), afgpu.MEL_ROW_DTYPE)
    i = o = 0
    for k, n in enumerate(lengths):
        f = afgpu.mel_frames(p, n) if frames is None else frames[k]
        rows[k]["in_off"], rows[k]["out_off"], rows[k]["in_frames"], rows[k]["out_frames"] = i, o, n, f
        i += n
        o += p.n_mels * f
    return rows, afgpu.mel_fft_layout(rows, p), i, o


def test_layout_in_tiles_of_sixteen_frames():
    p = good_params()
    rows = np.zeros(5, afgpu.MEL_ROW_DTYPE)
    rows["out_frames"] = [16, 17, 0, 1, 3000]
    assert afgpu.mel_fft_layout(rows, p) == 1 + 2 + 0 + 1 + 188
    assert list(rows["first_tile"]) == [0, 1, 3, 3, 4]
    big = good_params(n_fft=2048, win_length=2048, hop=2048, n_mels=256, center=0)
    assert afgpu.mel_fft_layout(rows, big) == 192                                      # the tile does not depend on the shape
    lib = afgpu.lib()
    for kw in BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_mel_fft_layout(rows.ctypes.data, len(rows), C.byref(bad)) == 0 and lib.afg_last_error().decode().startswith("afg_mel_params.")


def test_every_record_refusal_needs_no_device():
    lib = afgpu.lib()
    p = good_params()
    table, bank = 400 + 800, 80 * 201
    rows, tiles, nin, nout = records(p, [2000, 201, 700, 48000])
    afgpu.mel_fft_check_rows(rows, tiles, p, nin, table, bank, nout)                   # as it stands it passes
    afgpu.mel_fft_check_rows(rows[:0], 0, p, 0, 0, 0, 0)                               # no rows: the parameters alone
    seen = set()

    def refused(change=None, prm=p, **kw):
        bad = rows.copy()
        if change:
            change(bad)
        a = dict(tiles=tiles, nin=nin, table=table, bank=bank, nout=nout)
        a.update(kw)
        rc = lib.afg_mel_fft_check_rows(bad.ctypes.data, len(bad), a["tiles"], C.byref(prm), a["nin"], a["table"], a["bank"], a["nout"])
        msg = lib.afg_last_error().decode()
        assert rc == INVALID and msg, (rc, msg)
        seen.add(msg)

    for kw in BAD_PARAMS:                                                             # each parameter out of range
        refused(prm=good_params(**kw))
    n = len(seen)
    assert n == len(BAD_PARAMS)
    one = records(p, [200], [1])
    assert lib.afg_mel_fft_check_rows(one[0].ctypes.data, 1, one[1], C.byref(p), 200, table, bank, 80) == INVALID
    assert "reflect" in lib.afg_last_error().decode()                                  # 200 samples do have a frame, but not under reflect
    zero = good_params(pad_mode=afgpu.MEL_PAD_ZERO)
    assert lib.afg_mel_fft_check_rows(one[0].ctypes.data, 1, one[1], C.byref(zero), 200, table, bank, 80) == 0
    silent = records(p, [200], [0])
    assert lib.afg_mel_fft_check_rows(silent[0].ctypes.data, 1, 0, C.byref(p), 200, table, bank, 0) == 0
    refused(lambda b: b["in_frames"].__setitem__(1, 200), nin=nin + 1000)             # reflect with in_frames <= pad (and too many frames)
    refused(lambda b: b["out_frames"].__setitem__(2, 6))                               # out_frames > max_frames (700 samples: 5)
    assert "out_frames" in lib.afg_last_error().decode()
    refused(nin=nin - 1)                                                               # planes overrun
    refused(nout=nout - 1)
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(3, (1 << 64) - 8))
    refused(table=table - 1)
    refused(bank=bank - 1)
    refused(tiles=tiles + 1)                                                           # wrong tile count
    refused(lambda b: b["first_tile"].__setitem__(2, 0))
    direct = rows.copy()                                                               # the direct path's layout (tiles of 64) does not serve
    direct_tiles = afgpu.mel_layout(direct, p)
    assert direct_tiles != tiles
    refused(tiles=direct_tiles)
    assert len(seen) >= n + 9
    rows2, tiles2, nin2, nout2 = records(p, [480000], [3000])                          # fewer frames than the row has is fine
    afgpu.mel_fft_check_rows(rows2, tiles2, p, nin2, table, bank, nout2)


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = good_params()
    assert lib.afg_melspec_fft_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, 0, None, 0, None) == 0
    assert lib.afg_melspec_fft_hip(0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None) == INVALID
    for kw in BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_melspec_fft_hip(1, 0x1000, 1, C.byref(bad), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None) == INVALID
        assert lib.afg_last_error().decode().startswith("afg_mel_params.")
    for args in ((1, None, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, None, 8, 0x4000, 8, 0x5000, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, None, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, None, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2002, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1 << 32, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None)):
        assert lib.afg_melspec_fft_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_melspec_fft_hip:")


def call(n_files, opts, norm=False):
    """the batch entries with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    if norm:
        rc = lib.afg_batch_decode_mel_norm(ptrs, lens, n_files, C.byref(opts), None, None, 0x1000, C.byref(res))
    else:
        rc = lib.afg_batch_decode_mel(ptrs, lens, n_files, C.byref(opts), 0x1000, C.byref(res))
    return rc, lib.afg_last_error().decode(), res


def good_opts(mel=None, **kw):
    o = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, good_params(**(mel or {})), 0, 1, 0.0, 0.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("norm", [False, True], ids=["mel", "mel_norm"])
def test_batch_entries_refuse_before_any_device_call(norm):
    FFT = afgpu.MEL_ALGO_FFT
    cases = {
        "unknown algorithm": (call(1, good_opts(algorithm=2), norm), INVALID, "algorithm"),
        "reserved": (call(1, good_opts(reserved=1), norm), INVALID, "reserved"),
        "reserved with fft": (call(1, good_opts(algorithm=FFT, reserved=1 << 31), norm), INVALID, "reserved"),
        "short struct": (call(1, good_opts(algorithm=FFT, struct_size=C.sizeof(afgpu.MelOpts) - 8), norm), INVALID, "struct_size"),
        "fft, bad mel": (call(1, good_opts(algorithm=FFT, mel=dict(hop=0)), norm), INVALID, "hop"),
        "fft, no frame": (call(1, good_opts(algorithm=FFT, mel=dict(center=0), frames=399), norm), INVALID, "frame"),
        "fft, reflect": (call(1, good_opts(algorithm=FFT, frames=200), norm), INVALID, "reflect"),
    }
    for n in ODD_N_FFT:
        cases[f"fft {n}"] = (call(1, good_opts(algorithm=FFT, mel=dict(n_fft=n, win_length=16, hop=16)), norm), UNSUPPORTED, f"n_fft {n}")
    for what, ((rc, msg, res), want, word) in cases.items():
        assert rc == want and word in msg, (what, rc, msg)
        assert res.n_files == 0 and not res.items
    # algorithm 0 is what it was: the same sizes pass the argument check, and no file at all touches nothing
    for o in (good_opts(), good_opts(algorithm=FFT), good_opts(mel=dict(n_fft=401, win_length=16, hop=16)), good_opts(n_out=100)):
        rc, _, res = call(0, o, norm)
        assert rc == 0 and res.n_files == 0 and not res.items
    rc, msg, _ = call(1, good_opts(n_out=102), norm)                                   # ... and its refusals are the old ones
    assert rc == INVALID and "n_out" in msg


def test_python_entries_check_the_keyword():
    for fn in (afgpu.batch_decode_mel, afgpu.batch_decode_mel_normalized):
        with pytest.raises(ValueError, match="algorithm"):
            fn([b"x"], 16000, algorithm="fast")
        with pytest.raises(ValueError, match="algorithm"):
            fn([b"x"], 16000, algorithm=1)
