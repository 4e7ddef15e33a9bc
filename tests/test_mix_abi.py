"""afg_mix_ratio / afg_mix_layout / afg_mix_check_groups / afg_mix_hip / afg_batch_decode_mixed without a GPU: the symbols, the
structures, the tile counts and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import mix_model as mm
from test_collate_abi import c_layout
from test_normalize_abi import all_invalid_and_distinct, resample_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_mix_ratio", "afg_mix_layout", "afg_mix_check_groups", "afg_mix_hip", "afg_batch_decode_mixed")
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
    assert code.index("afg_convolve_hip(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    for const, value, mine in (("AFG_MIX_SNR", afgpu.MIX_SNR, mm.SNR), ("AFG_MIX_GAIN", afgpu.MIX_GAIN, mm.GAIN),
                               ("AFG_MIX_SILENT_SIGNAL", afgpu.MIX_SILENT_SIGNAL, mm.SILENT_SIGNAL),
                               ("AFG_MIX_SILENT_NOISE", afgpu.MIX_SILENT_NOISE, mm.SILENT_NOISE),
                               ("AFG_MIX_ENERGY_NOT_FINITE", afgpu.MIX_ENERGY_NOT_FINITE, mm.ENERGY_NOT_FINITE),
                               ("AFG_MIX_GAIN_NOT_FINITE", afgpu.MIX_GAIN_NOT_FINITE, mm.GAIN_NOT_FINITE)):
        assert re.search(rf"#define\s+{const}\s+{value}u\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
        assert mine == value
    assert afgpu.MIX_TILE == mm.TILE == 4096


def test_structures_match_the_header():
    for struct, cls, size in (("afg_mix_group", afgpu.MixGroup, 80), ("afg_mix_stats", afgpu.MixStats, 24), ("afg_mix_noise", afgpu.MixNoise, 56)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
    for mine, theirs in ((afgpu.MIX_GROUP_DTYPE, mm.GROUP_DTYPE), (afgpu.MIX_STATS_DTYPE, mm.STATS_DTYPE)):
        assert mine.itemsize == theirs.itemsize
        assert [(n, mine.fields[n][1]) for n in mine.names] == [(n, theirs.fields[n][1]) for n in theirs.names]
    assert C.sizeof(afgpu.ResampleOpts) == c_layout("afg_resample_opts", ["struct_size"])[0]      # the options are the ones they were


def groups_of(shapes, gap=7, N=100, per_row=False):
    """one group per (rows, valid), stride valid + gap, packed one after the other, each with a clip (or one per row) of N of its
    own; returns (groups, tiles, signal floats, noise floats)"""
    g = np.zeros(len(shapes), afgpu.MIX_GROUP_DTYPE)
    at = nat = 0
    for k, (rows, valid) in enumerate(shapes):
        g[k]["in_off"] = g[k]["out_off"] = at
        g[k]["stride"] = valid + gap
        g[k]["rows"], g[k]["valid"] = rows, valid
        g[k]["noise_off"], g[k]["noise_len"], g[k]["noise_start"], g[k]["noise_stride"] = nat, N, N - 1, (N if per_row else 0)
        g[k]["flags"], g[k]["ratio"] = afgpu.MIX_SNR, 1.0
        at += rows * (valid + gap)
        nat += (rows if per_row else 1) * N
    return g, afgpu.mix_layout(g), at, nat


def test_layout_counts_tiles_and_the_ratio_is_a_power_of_ten():
    for valid, tiles in ((0, 0), (1, 1), (4096, 1), (4097, 2)):
        g, n, _, _ = groups_of([(1, valid)])
        assert n == tiles and g["first_tile"][0] == 0
    g, n, _, _ = groups_of([(1, 0), (3, 4097), (2, 1), (1, 0), (1, 4096)])
    assert n == 9 and g["first_tile"].tolist() == [0, 0, 6, 8, 8]
    mine = g.view(mm.GROUP_DTYPE).copy()
    mine["first_tile"] = 99
    assert mm.layout(mine) == 9 and mine["first_tile"].tolist() == g["first_tile"].tolist()
    assert afgpu.lib().afg_mix_layout(None, 3) == 0
    big, n, _, _ = groups_of([(65535, 0xffffffff)])
    assert n == 65535 * (1 << 20)
    assert afgpu.mix_ratio(0) == 1.0 and afgpu.mix_ratio(10) == 0.1 and afgpu.mix_ratio(-30) == 1000.0 and afgpu.mix_ratio(float("inf")) == 0.0


def refused(groups, n_tiles, in_floats, noise_floats, out_floats, plane_at=None):
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.mix_check_groups(groups, n_tiles, in_floats, noise_floats, out_floats, plane_at)
    assert "(-1)" in str(e.value)
    return str(e.value)


def test_every_group_refusal_needs_no_device():
    for per_row in (False, True):
        g, tiles, floats, nfloats = groups_of([(1, 5000), (2, 4097), (1, 0), (3, 1)], per_row=per_row)
        afgpu.mix_check_groups(g, tiles, floats - 7, nfloats, floats - 7)                      # the last row's gap is not part of it
        afgpu.mix_check_groups(g, tiles, floats, nfloats, floats, (0, floats, 1 << 40))        # in one address space, apart
        afgpu.mix_check_groups(g, tiles, floats, nfloats, floats, (1 << 20, 0, 1 << 20))       # in place
        seen = set()

        def one(change, n_tiles=tiles, in_floats=floats, noise_floats=nfloats, out_floats=floats, plane_at=None):
            bad = g.copy()
            change(bad)
            msg = refused(bad, n_tiles, in_floats, noise_floats, out_floats, plane_at)
            assert msg not in seen, msg
            seen.add(msg)

        one(lambda b: None, in_floats=floats - 8)               # a group outside its input plane ...
        one(lambda b: None, out_floats=floats - 8)              # ... its output plane ...
        one(lambda b: None, noise_floats=nfloats - 1)           # ... its noise outside the noise plane
        one(lambda b: b["in_off"].__setitem__(0, 2 ** 64 - 4))  # ... by an offset that would wrap
        one(lambda b: b["out_off"].__setitem__(1, 2 ** 64 - 4))
        one(lambda b: b["noise_off"].__setitem__(3, 2 ** 64 - 4))
        one(lambda b: b["stride"].__setitem__(1, 2 ** 63))      # ... by a stride that would
        one(lambda b: b["stride"].__setitem__(1, 4096))         # stride < valid with two rows
        one(lambda b: b["rows"].__setitem__(0, 0))
        one(lambda b: b["rows"].__setitem__(2, 65536))
        one(lambda b: b["first_tile"].__setitem__(1, 3))
        one(lambda b: None, n_tiles=tiles + 1)
        one(lambda b: b["flags"].__setitem__(0, 2))             # an unknown mode
        one(lambda b: b["ratio"].__setitem__(0, float("nan")))
        one(lambda b: b["ratio"].__setitem__(1, -1.0))
        one(lambda b: b["ratio"].__setitem__(3, float("inf")))
        one(lambda b: (b["flags"].__setitem__(0, 1), b["gain"].__setitem__(0, float("nan"))))
        one(lambda b: (b["flags"].__setitem__(1, 1), b["gain"].__setitem__(1, -0.5)))
        one(lambda b: b["noise_len"].__setitem__(0, 0))
        one(lambda b: b["noise_start"].__setitem__(1, 100))     # noise_start == noise_len
        one(lambda b: b["noise_stride"].__setitem__(3, 99))     # neither 0 nor >= noise_len
        one(lambda b: b["noise_stride"].__setitem__(1, 2 ** 63))
        one(lambda b: b["out_off"].__setitem__(3, int(b["out_off"][0]) + 10))                  # an output over another output
        one(lambda b: b["out_off"].__setitem__(0, 1), plane_at=(0, 1 << 40, 0))                # an output over its own input, shifted
        one(lambda b: None, plane_at=(0, 1 << 40, 5000 + 7))    # an output over another group's input


def test_planes_and_ignored_fields():
    g, tiles, floats, nfloats = groups_of([(1, 5000), (2, 4097), (1, 0), (3, 1)])
    assert "noise plane" in refused(g, tiles, floats, nfloats, floats, (0, floats + 5, floats))       # the output plane over the noise plane
    assert "noise plane" in refused(g, tiles, floats, nfloats, floats, (0, 1 << 30, (1 << 30) + nfloats - 1))
    afgpu.mix_check_groups(g, tiles, floats, nfloats, floats, (0, 1 << 30, (1 << 30) + nfloats))      # ... behind it: fine
    afgpu.mix_check_groups(g, tiles, floats, nfloats, floats, (0, 5, 1 << 30))                        # inputs may meet the noise
    ok = g.copy()
    ok["stride"][0] = 0                                          # one row: the stride is not used
    ok["in_off"][2] = ok["noise_off"][2] = 2 ** 64 - 1           # no floats: only mode, level and rows are looked at
    ok["noise_len"][2] = 0
    ok["ratio"][3] = 0.0
    ok["gain"][0] = float("nan")                                 # the other mode's field is ignored
    afgpu.mix_check_groups(ok, tiles, floats, nfloats, floats)
    assert afgpu.lib().afg_mix_check_groups(None, 1, 0, 0, 0, 0, None) == INVALID
    assert afgpu.lib().afg_mix_check_groups(None, 0, 0, 0, 0, 0, None) == 0


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    assert lib.afg_mix_hip(0, None, 0, None, 0, None, 0, None, 0, None, None, None) == 0          # no groups: nothing to do
    good = (1, 0x1000, 1, 0x2000, 8, 0x6000, 8, 0x3000, 8, 0x4000, 0x5000, None)
    for at, value in ((1, None), (3, None), (5, None), (7, None), (9, None), (10, None), (1, 0x1004), (3, 0x2002), (5, 0x6001), (7, 0x3001),
                      (9, 0x4008), (10, 0x5004), (0, 1 << 32), (2, 1 << 31)):
        args = list(good)
        args[at] = value
        assert lib.afg_mix_hip(*args) == INVALID, at
        assert lib.afg_last_error().decode().startswith("afg_mix_hip:"), at


def bank(n_files=1, **kw):
    """an afg_mix_noise over a made-up device address, with its host arrays kept alive beside it"""
    keep = {"lengths": (C.c_uint32 * 2)(100, 50), "index": (C.c_uint32 * max(n_files, 1))(), "start": (C.c_uint64 * max(n_files, 1))(),
            "snr_db": (C.c_double * max(n_files, 1))()}
    b = afgpu.MixNoise(0x100000, 2, 100, 1, keep["lengths"], keep["index"], keep["start"], keep["snr_db"])
    for k, v in kw.items():
        if k in keep and v is not None and not isinstance(v, C.Array):
            keep[k][0] = v
        else:
            setattr(b, k, v)
    b._keep = keep
    return b


def call_mixed(n_files, opts, noise, d_out=0x1000, out=True):
    """afg_batch_decode_mixed with made-up device addresses: an argument error comes back before anything touches them"""
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_mixed(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if noise is None else C.byref(noise), d_out,
                                    None, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def test_batch_entry_refuses_its_arguments_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    neg = (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call_mixed(1, None, bank()),
        "NULL noise": call_mixed(1, resample_opts(), None),
        "NULL d_out": call_mixed(1, resample_opts(), bank(), d_out=None),
        "NULL out": call_mixed(1, resample_opts(), bank(), out=False),
        "short struct": call_mixed(1, resample_opts(struct_size=C.sizeof(afgpu.ResampleOpts) - 8), bank()),
        # what afg_batch_decode_resampled checks
        "no channels": call_mixed(1, resample_opts(channels=0), bank()),
        "no samplerate": call_mixed(1, resample_opts(samplerate=0), bank()),
        "mono with two channels": call_mixed(1, resample_opts(channels=2), bank()),
        "negative first_frame": call_mixed(1, resample_opts(first_frame=neg), bank()),
        "negative n_files": call_mixed(-1, resample_opts(), bank()),
        # the bank
        "NULL d_noise": call_mixed(1, resample_opts(), bank(d_noise=None)),
        "NULL snr_db": call_mixed(1, resample_opts(), bank(snr_db=None)),
        "d_noise alignment": call_mixed(1, resample_opts(), bank(d_noise=0x100002)),
        "no clips": call_mixed(1, resample_opts(), bank(n_clips=0)),
        "clip_rows": call_mixed(1, resample_opts(), bank(clip_rows=2)),
        "no clip_rows": call_mixed(1, resample_opts(), bank(clip_rows=0)),
        "too many clips": call_mixed(1, resample_opts(), bank(n_clips=1 << 62, lengths=None)),
        "a length of 0": call_mixed(1, resample_opts(), bank(lengths=0)),
        "a length past the pitch": call_mixed(1, resample_opts(), bank(lengths=101)),
        "index": call_mixed(1, resample_opts(), bank(index=2)),
        "snr nan": call_mixed(1, resample_opts(), bank(snr_db=float("nan"))),
        "snr ratio": call_mixed(1, resample_opts(), bank(snr_db=-4000.0)),
        "bank over the tensor": call_mixed(1, resample_opts(), bank(d_noise=0x1000 + 4 * 15999)),
    }
    all_invalid_and_distinct(cases)
    rc, _, res = call_mixed(0, resample_opts(), bank(0))         # no file at all: ok, and nothing is touched
    assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entries_check_their_arguments():
    class FakeTensor:                                            # no device here: the checks in front of the tensor's own
        pass
    for kw in (dict(frames=0, channels=1, samplerate=16000), dict(frames=100, channels=1, samplerate=0), dict(frames=100, channels=2, samplerate=16000, mono=True),
               dict(frames=100, channels=1, samplerate=16000)):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_noisy([b"x"], noise=FakeTensor(), snr_db=0.0, **kw)
    with pytest.raises(ValueError):
        afgpu.add_noise_tensor(FakeTensor(), FakeTensor(), snr_db=0.0)
