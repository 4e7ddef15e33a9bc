"""afg_norm_layout / afg_norm_check_groups / afg_normalize_hip / afg_batch_decode_resampled_norm / afg_batch_decode_mel_norm
without a GPU: the symbols, the structures, the tile counts and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import normalize_model as nm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_norm_layout", "afg_norm_check_groups", "afg_normalize_hip", "afg_batch_decode_resampled_norm", "afg_batch_decode_mel_norm")
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
    assert code.index("afg_batch_decode_mel(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    for const, value in (("AFG_NORM_NONE", afgpu.NORM_NONE), ("AFG_NORM_PEAK", afgpu.NORM_PEAK), ("AFG_NORM_RMS", afgpu.NORM_RMS),
                         ("AFG_NORM_STANDARD", afgpu.NORM_STANDARD), ("AFG_NORM_DYNAMIC_RANGE", afgpu.NORM_DYNAMIC_RANGE)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
        assert getattr(nm, const[9:]) == value
    assert afgpu.NORM_TILE == nm.TILE == 4096


def test_structures_match_the_header():
    for struct, cls, size in (("afg_norm_group", afgpu.NormGroup, 48), ("afg_norm_stats", afgpu.NormStats, 40), ("afg_norm_params", afgpu.NormParams, 24)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
    assert afgpu.NORM_GROUP_DTYPE.itemsize == nm.GROUP_DTYPE.itemsize == 48 and afgpu.NORM_STATS_DTYPE.itemsize == nm.STATS_DTYPE.itemsize == 40
    for mine, theirs in ((afgpu.NORM_GROUP_DTYPE, nm.GROUP_DTYPE), (afgpu.NORM_STATS_DTYPE, nm.STATS_DTYPE)):
        assert [(n, mine.fields[n][1]) for n in mine.names] == [(n, theirs.fields[n][1]) for n in theirs.names]
    # the option structures the batch entries take are the ones they were
    assert C.sizeof(afgpu.ResampleOpts) == c_layout("afg_resample_opts", ["struct_size"])[0]
    assert C.sizeof(afgpu.MelOpts) == c_layout("afg_mel_opts", ["struct_size"])[0]


def groups_of(shapes, gap=7):
    """one group per (rows, valid), stride valid + gap, packed one after the other; returns (groups, tiles, floats)"""
    g = np.zeros(len(shapes), afgpu.NORM_GROUP_DTYPE)
    at = 0
    for k, (rows, valid) in enumerate(shapes):
        g[k]["in_off"] = g[k]["out_off"] = at
        g[k]["stride"] = valid + gap
        g[k]["rows"], g[k]["valid"] = rows, valid
        at += rows * (valid + gap)
    return g, afgpu.norm_layout(g), at


def test_layout_counts_tiles():
    for valid, tiles in ((0, 0), (1, 1), (4096, 1), (4097, 2)):
        g, n, _ = groups_of([(1, valid)])
        assert n == tiles and g["first_tile"][0] == 0
    g, n, _ = groups_of([(3, 4097)])
    assert n == 6
    g, n, _ = groups_of([(1, 0), (3, 4097), (2, 1), (1, 0), (1, 4096)])
    assert n == 9 and g["first_tile"].tolist() == [0, 0, 6, 8, 8]
    mine = g.view(nm.GROUP_DTYPE).copy()
    mine["first_tile"] = 99
    assert nm.layout(mine) == 9 and mine["first_tile"].tolist() == g["first_tile"].tolist()
    assert afgpu.lib().afg_norm_layout(None, 3) == 0
    big, n, _ = groups_of([(65535, 0xffffffff)])
    assert n == 65535 * (1 << 20)


BAD_PARAMS = [dict(mode=5), dict(mode="peak", target=0.0), dict(mode="peak", target=float("inf")), dict(mode="rms", target=-1.0),
              dict(mode="rms", target=float("nan")), dict(mode="standard", eps=-1e-9), dict(mode="standard", eps=float("inf")),
              dict(mode="dynamic_range", range=0.0), dict(mode="dynamic_range", range=float("nan")), dict(mode="dynamic_range", gain=0.0),
              dict(mode="dynamic_range", gain=float("-inf")), dict(mode="dynamic_range", shift=float("nan"))]


def refused(groups, n_tiles, prm, in_floats, out_floats):
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.norm_check_groups(groups, n_tiles, prm, in_floats, out_floats)
    return str(e.value)


def test_every_group_refusal_needs_no_device():
    peak = afgpu.norm_params("peak")
    g, tiles, floats = groups_of([(1, 5000), (2, 4097), (1, 0), (3, 1)])
    for mode in ("none", "peak", "rms", "standard", "dynamic_range", "whisper"):
        afgpu.norm_check_groups(g, tiles, afgpu.norm_params(mode), floats - 7, floats - 7)      # the last row's gap is not part of it
    afgpu.norm_check_groups(g, tiles, afgpu.norm_params("none"), floats, 0)                 # statistics only: no output plane
    seen = set()

    def one(change, n_tiles=tiles, prm=peak, in_floats=floats, out_floats=floats):
        bad = g.copy()
        change(bad)
        msg = refused(bad, n_tiles, prm, in_floats, out_floats)
        assert msg not in seen, msg
        seen.add(msg)

    one(lambda b: None, in_floats=floats - 8)                   # a group outside its input plane ...
    one(lambda b: None, out_floats=floats - 8)                  # ... its output plane ...
    one(lambda b: b["in_off"].__setitem__(0, 2 ** 64 - 4))     # ... by an offset that would wrap
    one(lambda b: b["out_off"].__setitem__(1, 2 ** 64 - 4))
    one(lambda b: b["stride"].__setitem__(1, 2 ** 63))          # ... by a stride that would
    one(lambda b: b["stride"].__setitem__(1, 4096))             # stride < valid with two rows
    one(lambda b: b["rows"].__setitem__(0, 0))                  # rows == 0
    one(lambda b: b["rows"].__setitem__(2, 65536))
    one(lambda b: b["first_tile"].__setitem__(1, 3))            # a wrong first_tile
    one(lambda b: None, n_tiles=tiles + 1)                      # a wrong n_tiles
    # stride < valid is fine for a single row; nothing of a group without floats is looked at but its rows
    ok = g.copy()
    ok["stride"][0] = 0
    ok["in_off"][2] = 2 ** 64 - 1
    afgpu.norm_check_groups(ok, tiles, peak, floats, floats)
    for case in BAD_PARAMS:
        kw = dict(case)
        mode = kw.pop("mode")
        prm = afgpu.norm_params(mode, **kw) if isinstance(mode, str) else afgpu.NormParams(mode, 1.0, 0.0, 8.0, 4.0, 0.25)
        assert refused(g, tiles, prm, floats, floats).count("afg_norm_params") == 1
        assert afgpu.lib().afg_norm_check_groups(None, 0, 0, C.byref(prm), 0, 0) == INVALID       # the parameters alone
    assert afgpu.lib().afg_norm_check_groups(g.ctypes.data, len(g), tiles, None, floats, floats) == INVALID
    assert afgpu.lib().afg_norm_check_groups(None, 1, 0, C.byref(peak), 0, 0) == INVALID
    with pytest.raises(ValueError):
        afgpu.norm_params("loudness")


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = afgpu.norm_params("peak")
    assert lib.afg_normalize_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, None, None) == 0           # no groups: nothing to do
    good = (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 0x5000, None)
    for at, value in ((1, None), (3, None), (4, None), (6, None), (8, None), (9, None), (4, 0x2002), (6, 0x3001), (8, 0x4004), (9, 0x5004),
                      (0, 1 << 32), (2, 1 << 31)):
        args = list(good)
        args[at] = value
        assert lib.afg_normalize_hip(*args) == INVALID, at
        assert lib.afg_last_error().decode().startswith("afg_normalize_hip:"), at


def call_resampled(n_files, opts, norm, d_out=0x1000, d_stats=None, out=True):
    """afg_batch_decode_resampled_norm with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_resampled_norm(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if norm is None else C.byref(norm),
                                             d_out, d_stats, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def call_mel(n_files, opts, wave, feat, d_out=0x1000, out=True):
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_mel_norm(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if wave is None else C.byref(wave),
                                       None if feat is None else C.byref(feat), d_out, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def resample_opts(**kw):
    o = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def mel_opts(mel=None, **kw):
    o = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, afgpu.mel_params(**(mel or {})), 0, 1, 0.0, 0.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def all_invalid_and_distinct(cases):
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items


def test_resampled_entry_refuses_its_arguments_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    peak, neg = afgpu.norm_params("peak"), (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call_resampled(1, None, peak),
        "NULL norm": call_resampled(1, resample_opts(), None),
        "NULL d_out": call_resampled(1, resample_opts(), peak, d_out=None),
        "NULL out": call_resampled(1, resample_opts(), peak, out=False),
        "short struct": call_resampled(1, resample_opts(struct_size=C.sizeof(afgpu.ResampleOpts) - 8), peak),
        "d_stats alignment": call_resampled(1, resample_opts(), peak, d_stats=0x2004),
        # what afg_batch_decode_resampled checks
        "no channels": call_resampled(1, resample_opts(channels=0), peak),
        "no samplerate": call_resampled(1, resample_opts(samplerate=0), peak),
        "mono with two channels": call_resampled(1, resample_opts(channels=2), peak),
        "in_channels": call_resampled(1, resample_opts(in_channels=65536), peak),
        "max_in_rate": call_resampled(1, resample_opts(max_in_rate=(1 << 20) + 1), peak),
        "lowpass_width": call_resampled(1, resample_opts(lowpass_width=65), peak),
        "negative first_frame": call_resampled(1, resample_opts(first_frame=neg), peak),
        "negative n_files": call_resampled(-1, resample_opts(), peak),
        # the norm parameters
        "mode": call_resampled(1, resample_opts(), afgpu.NormParams(5, 1.0, 0.0, 8.0, 4.0, 0.25)),
        "target": call_resampled(1, resample_opts(), afgpu.norm_params("rms", target=0.0)),
        "eps": call_resampled(1, resample_opts(), afgpu.norm_params("standard", eps=-1.0)),
        "range": call_resampled(1, resample_opts(), afgpu.norm_params("dynamic_range", range=float("inf"))),
    }
    all_invalid_and_distinct(cases)
    rc, _, res = call_resampled(0, resample_opts(), peak)        # no file at all: ok, and nothing is touched
    assert rc == 0 and res.n_files == 0 and not res.items


def test_mel_entry_refuses_its_arguments_before_any_device_call():
    whisper, std = afgpu.norm_params("whisper"), afgpu.norm_params("standard")
    cases = {
        "NULL opts": call_mel(1, None, std, whisper),
        "NULL d_out": call_mel(1, mel_opts(), std, whisper, d_out=None),
        "NULL out": call_mel(1, mel_opts(), std, whisper, out=False),
        "short struct": call_mel(1, mel_opts(struct_size=C.sizeof(afgpu.MelOpts) - 8), std, whisper),
        "no channels": call_mel(1, mel_opts(channels=0), std, whisper),
        "mel parameters": call_mel(1, mel_opts(mel=dict(n_fft=15)), std, whisper),
        "bank": call_mel(1, mel_opts(scale=2), std, whisper),
        "n_out": call_mel(1, mel_opts(n_out=102), std, whisper),
        "reflect": call_mel(1, mel_opts(frames=200), std, whisper),
        "wave mode": call_mel(1, mel_opts(), afgpu.NormParams(9, 1.0, 0.0, 8.0, 4.0, 0.25), whisper),
        "wave eps": call_mel(1, mel_opts(), afgpu.norm_params("standard", eps=float("nan")), None),
        "feat gain": call_mel(1, mel_opts(), None, afgpu.norm_params("dynamic_range", gain=-0.25)),
        "feat shift": call_mel(1, mel_opts(), std, afgpu.norm_params("dynamic_range", shift=float("inf"))),
    }
    all_invalid_and_distinct(cases)
    for wave, feat in ((None, None), (std, None), (None, whisper), (std, whisper)):       # NULL means none; no file: nothing is touched
        rc, _, res = call_mel(0, mel_opts(), wave, feat)
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entries_check_their_arguments():
    for kw in (dict(frames=0, channels=1, samplerate=16000, mode="peak"), dict(frames=100, channels=1, samplerate=0, mode="peak"),
               dict(frames=100, channels=2, samplerate=16000, mode="peak", mono=True), dict(frames=100, channels=1, samplerate=16000, mode="loud")):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_normalized([b"x"], **kw)
    for kw in (dict(frames=0), dict(frames=16000, n_out=102), dict(frames=16000, feat_norm="wisper"), dict(frames=16000, wave_norm="unit")):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mel_normalized([b"x"], **kw)
    w = afgpu.norm_params("whisper")
    assert (w.mode, w.range, w.shift, w.gain) == (afgpu.NORM_DYNAMIC_RANGE, 8.0, 4.0, 0.25)
