"""The linear spectrogram stage without a GPU: the symbols, the layout of afg_stft_params and afg_stft_opts, tile and layout,
and every refusal that needs no device -- of the parameters, of the records, of the batch entry."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import melspec_fft_model as fm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_stft_tile_frames", "afg_stft_layout", "afg_stft_check_rows", "afg_stft_hip", "afg_batch_decode_stft")
INVALID, UNSUPPORTED = -1, -5
KINDS = (afgpu.STFT_COMPLEX, afgpu.STFT_MAGNITUDE, afgpu.STFT_POWER, afgpu.STFT_LOG10)


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
    for const, value in (("AFG_STFT_COMPLEX", afgpu.STFT_COMPLEX), ("AFG_STFT_MAGNITUDE", afgpu.STFT_MAGNITUDE), ("AFG_STFT_POWER", afgpu.STFT_POWER),
                         ("AFG_STFT_LOG10", afgpu.STFT_LOG10)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
    assert KINDS == (0, 1, 2, 3)
    assert lib.afg_abi_version() == 2
    for name in ("stft_params", "stft_tile_frames", "stft_layout", "stft_check_rows", "stft", "batch_decode_stft"):
        assert callable(getattr(afgpu, name))


def test_struct_sizes_and_field_order():
    names = [f[0] for f in afgpu.StftParams._fields_]
    assert names == ["n_fft", "win_length", "hop", "center", "pad_mode", "out_kind", "log_floor", "reserved"]
    size, offs = c_layout("afg_stft_params", names)
    assert size == C.sizeof(afgpu.StftParams) == 32 and offs == list(range(0, 32, 4))
    names = [f[0] for f in afgpu.StftOpts._fields_]
    lead = [f[0] for f in afgpu.ResampleOpts._fields_]
    assert names == lead + ["n_out", "stft", "reserved"]
    assert names[:len(lead) + 1] == [f[0] for f in afgpu.MelOpts._fields_][:len(lead) + 1]        # as afg_mel_opts carries them
    size, offs = c_layout("afg_stft_opts", names)
    assert size == C.sizeof(afgpu.StftOpts) == 88
    assert offs == [getattr(afgpu.StftOpts, n).offset for n in names]
    assert offs[:len(lead) + 1] == [getattr(afgpu.MelOpts, n).offset for n in names[:len(lead) + 1]]
    assert c_layout("afg_mel_row", ["in_off"])[0] == afgpu.MEL_ROW_DTYPE.itemsize == 32             # the rows are the mel stage's, untouched
    assert c_layout("afg_mel_params", ["n_fft"])[0] == C.sizeof(afgpu.MelParams) == 32
    p = afgpu.stft_params()
    assert (p.n_fft, p.win_length, p.hop, p.center, p.pad_mode, p.out_kind, p.log_floor, p.reserved) == (400, 400, 160, 1, 0, afgpu.STFT_POWER, 0.0, 0)


def good_params(**kw):
    p = afgpu.stft_params(400, 160, None, True, afgpu.MEL_PAD_REFLECT, afgpu.STFT_POWER, 0.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_N_FFT = [dict(n_fft=15, win_length=15, hop=15), dict(n_fft=2049), dict(n_fft=14 * 3 * 5, win_length=16, hop=16), dict(n_fft=17, win_length=16, hop=16)]
BAD_PARAMS = [dict(win_length=0), dict(win_length=401), dict(hop=0), dict(hop=401), dict(center=2), dict(pad_mode=2), dict(out_kind=4),
              dict(log_floor=-1.0), dict(log_floor=float("nan")), dict(log_floor=float("inf")), dict(reserved=1)]


def test_tile_and_layout_are_consistent():
    lib = afgpu.lib()
    frames = [16, 17, 0, 1, 3000, 64, 65, 33]
    for n_fft in (16, 60, 75, 250, 400, 512, 1024, 1215, 1875, 2025, 2048):
        for kind in KINDS:
            p = good_params(n_fft=n_fft, win_length=n_fft, hop=min(n_fft, 160), out_kind=kind)
            tile = afgpu.stft_tile_frames(p)
            comps = 2 if kind == afgpu.STFT_COMPLEX else 1
            assert tile * comps in (16, 32, 64)
            # the widest row of the staging that fits beside four wavefronts' buffers; the two largest odd n_fft, which transform
            # at full length, fit only width 16 beside two (csrc/stft.hip)
            nc = n_fft // 2 if n_fft % 2 == 0 else n_fft
            lds = lambda waves, w: 4 * (waves * 4 * nc + (n_fft // 2 + 1) * (w + 1))
            fits = [w for w in (64, 32, 16) if lds(4, w) <= 152 * 1024]
            assert (fits == []) == (n_fft in (1875, 2025))
            assert tile * comps == (fits[0] if fits else 16) and (fits or lds(2, 16) <= 152 * 1024)
            rows = np.zeros(len(frames), afgpu.MEL_ROW_DTYPE)
            rows["out_frames"] = frames
            want = [math.ceil(f / tile) for f in frames]
            assert afgpu.stft_layout(rows, p) == sum(want)
            assert list(rows["first_tile"]) == [sum(want[:k]) for k in range(len(frames))]
    assert afgpu.stft_tile_frames(good_params()) == 64 and afgpu.stft_tile_frames(good_params(out_kind=afgpu.STFT_COMPLEX)) == 32
    rows = np.zeros(2, afgpu.MEL_ROW_DTYPE)
    for kw in BAD_N_FFT + BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_stft_tile_frames(C.byref(bad)) == 0 and lib.afg_last_error().decode().startswith("afg_stft_params.")
        assert lib.afg_stft_layout(rows.ctypes.data, len(rows), C.byref(bad)) == 0 and lib.afg_last_error().decode().startswith("afg_stft_params.")
        with pytest.raises(afgpu.AfgError):
            afgpu.stft_tile_frames(bad)
    assert lib.afg_stft_tile_frames(None) == 0


def records(p, lengths, frames=None):
    rows = np.zeros(len(lengths), afgpu.MEL_ROW_DTYPE)
    per = (2 if p.out_kind == afgpu.STFT_COMPLEX else 1) * (p.n_fft // 2 + 1)
    mel = afgpu.MelParams(p.n_fft, p.win_length, p.hop, 1, p.center, p.pad_mode, 0, 0.0)
    i = o = 0
    for k, n in enumerate(lengths):
        f = afgpu.mel_frames(mel, n) if frames is None else frames[k]
        rows[k]["in_off"], rows[k]["out_off"], rows[k]["in_frames"], rows[k]["out_frames"] = i, o, n, f
        i += n
        o += per * f
    return rows, afgpu.stft_layout(rows, p), i, o


@pytest.mark.parametrize("kind", KINDS, ids=["complex", "magnitude", "power", "log10"])
def test_every_parameter_and_record_refusal_needs_no_device(kind):
    lib = afgpu.lib()
    p = good_params(out_kind=kind)
    table = 400 + 800
    per = (2 if kind == afgpu.STFT_COMPLEX else 1) * 201
    rows, tiles, nin, nout = records(p, [2000, 201, 700, 48000])
    assert nout == per * (13 + 2 + 5 + 301)
    afgpu.stft_check_rows(rows, tiles, p, nin, table, nout)                            # as it stands it passes
    afgpu.stft_check_rows(rows[:0], 0, p, 0, 0, 0)                                     # no rows: the parameters alone
    seen = set()

    def refused(change=None, prm=p, want=INVALID, **kw):
        bad = rows.copy()
        if change:
            change(bad)
        a = dict(tiles=tiles, nin=nin, table=table, nout=nout)
        a.update(kw)
        rc = lib.afg_stft_check_rows(bad.ctypes.data, len(bad), a["tiles"], C.byref(prm), a["nin"], a["table"], a["nout"])
        msg = lib.afg_last_error().decode()
        assert rc == want and msg, (rc, msg)
        seen.add(msg)

    for kw in BAD_N_FFT:                                                              # each n_fft the path does not take
        refused(prm=good_params(out_kind=kind, **kw), want=UNSUPPORTED)
        assert f"n_fft {kw['n_fft']}" in lib.afg_last_error().decode()
        assert not fm.supported(kw["n_fft"])
        with pytest.raises(afgpu.AfgError, match="unsupported"):
            afgpu.stft_check_rows(rows, tiles, good_params(out_kind=kind, **kw), nin, table, nout)
    for kw in BAD_PARAMS:                                                             # each parameter out of range
        refused(prm=good_params(**dict(dict(out_kind=kind), **kw)))
    n = len(seen)
    assert n == len(BAD_N_FFT) + len(BAD_PARAMS)
    one = records(p, [200], [1])
    assert lib.afg_stft_check_rows(one[0].ctypes.data, 1, one[1], C.byref(p), 200, table, per) == INVALID
    assert "reflect" in lib.afg_last_error().decode()                                  # 200 samples do have a frame, but not under reflect
    zero = good_params(out_kind=kind, pad_mode=afgpu.MEL_PAD_ZERO)
    assert lib.afg_stft_check_rows(one[0].ctypes.data, 1, one[1], C.byref(zero), 200, table, per) == 0
    silent = records(p, [200], [0])
    assert lib.afg_stft_check_rows(silent[0].ctypes.data, 1, 0, C.byref(p), 200, table, 0) == 0
    refused(lambda b: b["in_frames"].__setitem__(1, 200), nin=nin + 1000)             # reflect with in_frames <= pad (and too many frames)
    refused(lambda b: b["out_frames"].__setitem__(2, 6))                               # out_frames > max_frames (700 samples: 5)
    assert "out_frames" in lib.afg_last_error().decode()
    refused(nin=nin - 1)                                                               # planes overrun
    refused(nout=nout - 1)                                                             # (complex: the 2 * n_bins * out_frames floats by one)
    assert f"{per * 301} floats" in lib.afg_last_error().decode()
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(3, (1 << 64) - 8))
    refused(table=table - 1)
    refused(tiles=tiles + 1)                                                           # wrong tile count
    refused(lambda b: b["first_tile"].__setitem__(2, 0))
    mel = rows.copy()                                                                  # the mel FFT path's layout (tiles of 16) does not serve
    mel_tiles = afgpu.mel_fft_layout(mel, afgpu.mel_params(400, 160, 80))
    assert mel_tiles != tiles
    refused(lambda b: b["first_tile"].__setitem__(slice(None), mel["first_tile"]), tiles=mel_tiles)
    assert len(seen) >= n + 9
    if kind != afgpu.STFT_COMPLEX:                                                     # a one-component record in a complex launch overruns
        assert lib.afg_stft_check_rows(rows.ctypes.data, len(rows), afgpu.stft_layout(rows.copy(), good_params(out_kind=0)), C.byref(good_params(out_kind=0)),
                                       nin, table, nout) == INVALID
    rows2, tiles2, nin2, nout2 = records(p, [480000], [3000])                          # fewer frames than the row has is fine
    afgpu.stft_check_rows(rows2, tiles2, p, nin2, table, nout2)


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = good_params()
    assert lib.afg_stft_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, 0, None) == 0
    assert lib.afg_stft_hip(0, None, 0, None, None, 0, None, 0, None, 0, None) == INVALID
    for kw in BAD_N_FFT + BAD_PARAMS:
        bad = good_params(**kw)
        assert lib.afg_stft_hip(1, 0x1000, 1, C.byref(bad), 0x2000, 8, 0x3000, 8, 0x5000, 8, None) == (UNSUPPORTED if kw in BAD_N_FFT else INVALID)
        assert lib.afg_last_error().decode().startswith("afg_stft_params.")
    for args in ((1, None, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, None, 8, 0x5000, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, None, 8, None), (1, 0x1000, 1, C.byref(p), 0x2002, 8, 0x3000, 8, 0x5000, 8, None),
                 (1 << 32, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x5000, 8, None)):
        assert lib.afg_stft_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_stft_hip:")


def call(n_files, opts):
    """the batch entry with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_stft(ptrs, lens, n_files, C.byref(opts), 0x1000, C.byref(res))
    return rc, lib.afg_last_error().decode(), res


def good_opts(stft=None, **kw):
    o = afgpu.StftOpts(C.sizeof(afgpu.StftOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, good_params(**(stft or {})), 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_the_batch_entry_refuses_before_any_device_call():
    cases = {
        "short struct": (call(1, good_opts(struct_size=C.sizeof(afgpu.StftOpts) - 8)), INVALID, "struct_size"),
        "reserved": (call(1, good_opts(reserved=1)), INVALID, "reserved"),
        "reserved in the parameters": (call(1, good_opts(stft=dict(reserved=1 << 31))), INVALID, "reserved"),
        "n_out": (call(1, good_opts(n_out=102)), INVALID, "n_out"),                   # 16000 samples have 101 frames
        "reflect": (call(1, good_opts(frames=200)), INVALID, "reflect"),
        "no frame": (call(1, good_opts(stft=dict(center=0), frames=399)), INVALID, "frame"),
        "bad hop": (call(1, good_opts(stft=dict(hop=0))), INVALID, "hop"),
        "bad kind": (call(1, good_opts(stft=dict(out_kind=4))), INVALID, "out_kind"),
        "no channels": (call(1, good_opts(channels=0)), INVALID, "channels"),
    }
    for kw in BAD_N_FFT:
        cases[f"n_fft {kw['n_fft']}"] = (call(1, good_opts(stft=kw)), UNSUPPORTED, f"n_fft {kw['n_fft']}")
    for what, ((rc, msg, res), want, word) in cases.items():
        assert rc == want and word in msg, (what, rc, msg)
        assert res.n_files == 0 and not res.items
    for o in (good_opts(), good_opts(n_out=100), good_opts(stft=dict(out_kind=afgpu.STFT_COMPLEX)), good_opts(stft=dict(n_fft=75, win_length=75, hop=25))):
        rc, _, res = call(0, o)                                                        # no file at all touches nothing
        assert rc == 0 and res.n_files == 0 and not res.items
    lib = afgpu.lib()
    res = afgpu.BatchResult()
    assert lib.afg_batch_decode_stft(None, None, 0, None, 0x1000, C.byref(res)) == INVALID
    assert lib.afg_batch_decode_stft(None, None, 0, C.byref(good_opts()), None, C.byref(res)) == INVALID


def test_the_python_entry_checks_its_arguments_first():
    with pytest.raises(ValueError, match="mono"):
        afgpu.batch_decode_stft([b"x"], 16000, channels=2)
    with pytest.raises(ValueError, match="n_out"):
        afgpu.batch_decode_stft([b"x"], 16000, n_out=102)
    with pytest.raises(ValueError, match="no frame"):
        afgpu.batch_decode_stft([b"x"], 399, center=False)
    with pytest.raises(afgpu.AfgError, match="n_fft 210"):
        afgpu.batch_decode_stft([b"x"], 16000, n_fft=210, hop=16)
    with pytest.raises(afgpu.AfgError, match="out_kind"):
        afgpu.batch_decode_stft([b"x"], 16000, out_kind=4)
