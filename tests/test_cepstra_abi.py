"""afg_cep_dct / afg_cep_layout / afg_cep_check_rows / afg_cepstra_hip / afg_batch_decode_mfcc without a GPU: the symbols, the
structures, the tile counts and every refusal that needs no device, each with its message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import cepstra_model as cm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_cep_dct", "afg_cep_layout", "afg_cep_check_rows", "afg_cepstra_hip", "afg_batch_decode_mfcc")
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
    assert code.index("afg_batch_decode_mel_norm(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    for const, value in (("AFG_CEP_DCT_NONE", afgpu.CEP_DCT_NONE), ("AFG_CEP_DCT_ORTHO", afgpu.CEP_DCT_ORTHO), ("AFG_CEP_TILE", afgpu.CEP_TILE)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
    assert (afgpu.CEP_DCT_NONE, afgpu.CEP_DCT_ORTHO, afgpu.CEP_TILE) == (cm.DCT_NONE, cm.DCT_ORTHO, cm.TILE)
    for name in ("CepParams", "CepRow", "MfccOpts", "cep_dct", "cep_layout", "cep_check_rows", "cepstra", "batch_decode_mfcc"):
        assert hasattr(afgpu, name), name


def test_structures_match_the_header():
    for struct, cls, size in (("afg_cep_params", afgpu.CepParams, 32), ("afg_cep_row", afgpu.CepRow, 32)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
    names = [f[0] for f in afgpu.MfccOpts._fields_]
    got, offs = c_layout("afg_mfcc_opts", names)
    assert got == C.sizeof(afgpu.MfccOpts) and offs == [getattr(afgpu.MfccOpts, n).offset for n in names]
    assert afgpu.CEP_ROW_DTYPE.itemsize == cm.ROW_DTYPE.itemsize == 32
    assert [(n, afgpu.CEP_ROW_DTYPE.fields[n][1]) for n in afgpu.CEP_ROW_DTYPE.names] == [(n, cm.ROW_DTYPE.fields[n][1]) for n in cm.ROW_DTYPE.names]
    # the structures the new one embeds and the entries beside it take are the ones they were
    assert C.sizeof(afgpu.MelOpts) == c_layout("afg_mel_opts", ["struct_size"])[0]
    assert C.sizeof(afgpu.NormParams) == c_layout("afg_norm_params", ["mode"])[0] == 24


def rows_of(frames, n_mels, out_rows, gap=3):
    """one record per length, slabs packed one after the other with `gap` floats between; returns (rows, in_floats, out_floats)"""
    r = np.zeros(len(frames), afgpu.CEP_ROW_DTYPE)
    a = b = gap
    for k, F in enumerate(frames):
        r[k]["in_off"], r[k]["out_off"], r[k]["frames"] = a, b, F
        a += n_mels * F + gap
        b += out_rows * F + gap
    return r, a - gap, b - gap


def test_layout_counts_tiles():
    p = afgpu.cep_params(80, 13, 2, 2)
    for F, tiles in ((0, 0), (1, 1), (63, 1), (64, 1), (65, 2), (128, 2), (129, 3), (0xffffffff, 1 << 26)):
        r, _, _ = rows_of([F], 80, 39)
        assert afgpu.cep_layout(r, p) == tiles and r["first_tile"][0] == 0
    r, _, _ = rows_of([0, 65, 1, 0, 64, 3000], 80, 39)
    assert afgpu.cep_layout(r, p) == 2 + 1 + 1 + 47 and r["first_tile"].tolist() == [0, 0, 2, 3, 3, 4]
    mine = r.view(cm.ROW_DTYPE).copy()
    mine["first_tile"] = 99
    assert cm.layout(mine) == 51 and mine["first_tile"].tolist() == r["first_tile"].tolist()
    assert afgpu.lib().afg_cep_layout(None, 3, C.byref(p)) == 0
    assert afgpu.lib().afg_cep_layout(r.ctypes.data, len(r), C.byref(afgpu.cep_params(80, 81))) == 0          # params out of range
    assert "n_ceps" in afgpu.lib().afg_last_error().decode()


BAD_PARAMS = [dict(n_mels=0), dict(n_mels=257), dict(n_ceps=0), dict(n_ceps=81), dict(delta_order=3), dict(delta_order=1, delta_win=0),
              dict(delta_order=2, delta_win=9)]


def refused(rows, n_tiles, prm, in_floats, dct_floats, out_floats):
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.cep_check_rows(rows, n_tiles, prm, in_floats, dct_floats, out_floats)
    return str(e.value)


def test_every_record_refusal_needs_no_device():
    p = afgpu.cep_params(80, 13, 2, 2)
    r, in_floats, out_floats = rows_of([100, 0, 65, 1], 80, 39)
    tiles = afgpu.cep_layout(r, p)
    dct = 13 * 80
    afgpu.cep_check_rows(r, tiles, p, in_floats, dct, out_floats)
    afgpu.cep_check_rows(r, tiles, afgpu.cep_params(80, 13, 0, 99), in_floats, dct, out_floats - 26)      # delta_win is ignored without deltas
    seen = set()

    def one(change, n_tiles=tiles, prm=p, in_floats=in_floats, dct_floats=dct, out_floats=out_floats):
        bad = r.copy()
        change(bad)
        msg = refused(bad, n_tiles, prm, in_floats, dct_floats, out_floats)
        assert msg not in seen, msg
        seen.add(msg)

    one(lambda b: None, in_floats=in_floats - 1)                # a record outside its input plane ...
    one(lambda b: None, out_floats=out_floats - 1)              # ... its output plane ...
    one(lambda b: b["in_off"].__setitem__(0, 2 ** 64 - 4))     # ... by an offset that would wrap
    one(lambda b: b["out_off"].__setitem__(2, 2 ** 64 - 4))
    one(lambda b: None, dct_floats=dct - 1)                     # a table too small
    one(lambda b: b["first_tile"].__setitem__(2, 3))            # a wrong first_tile
    one(lambda b: None, n_tiles=tiles + 1)                      # a wrong n_tiles
    one(lambda b: b["reserved"].__setitem__(1, 7))              # a reserved word, even of a record without frames
    ok = r.copy()                                               # nothing else of a record without frames is looked at
    ok["in_off"][1] = ok["out_off"][1] = 2 ** 64 - 1
    afgpu.cep_check_rows(ok, tiles, p, in_floats, dct, out_floats)
    for case in BAD_PARAMS:
        kw = dict(n_mels=80, n_ceps=13, delta_order=2, delta_win=2)
        kw.update(case)
        prm = afgpu.cep_params(**kw)
        msg = refused(r, tiles, prm, in_floats, dct, out_floats)
        assert msg.count("afg_cep_params") == 1 and msg not in seen, msg
        seen.add(msg)
        assert afgpu.lib().afg_cep_check_rows(None, 0, 0, C.byref(prm), 0, 0, 0) == INVALID          # the parameters alone
    for k in range(4):
        prm = afgpu.cep_params(80, 13, 2, 2)
        prm.reserved[k] = 1
        assert f"reserved[{k}]" in refused(r, tiles, prm, in_floats, dct, out_floats)
    assert afgpu.lib().afg_cep_check_rows(None, 0, 0, C.byref(p), 0, 0, 0) == 0
    assert afgpu.lib().afg_cep_check_rows(r.ctypes.data, len(r), tiles, None, in_floats, dct, out_floats) == INVALID
    assert afgpu.lib().afg_cep_check_rows(None, 1, 0, C.byref(p), 0, dct, 0) == INVALID


def test_the_table_entry_refuses_its_arguments():
    lib = afgpu.lib()
    seen = set()
    for args in ((13, 0, 1, 0.0, 1.0), (13, 257, 1, 0.0, 1.0), (0, 80, 1, 0.0, 1.0), (81, 80, 1, 0.0, 1.0), (13, 80, 2, 0.0, 1.0),
                 (13, 80, 1, -1.0, 1.0), (13, 80, 1, float("nan"), 1.0), (13, 80, 1, float("inf"), 1.0), (13, 80, 1, 0.0, 0.0),
                 (13, 80, 1, 0.0, float("nan")), (13, 80, 1, 0.0, float("-inf"))):
        assert lib.afg_cep_dct(*args, None, 0) == 0, args
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_cep_dct:"), msg
        seen.add(msg)
        with pytest.raises(afgpu.AfgError):
            afgpu.cep_dct(*args)
    assert len(seen) == 11
    assert lib.afg_cep_dct(13, 80, 1, 22.0, 10.0, None, 0) == 13 * 80
    small = np.full(13 * 80, 5.0, np.float32)
    assert lib.afg_cep_dct(13, 80, 1, 22.0, 10.0, small.ctypes.data, 13 * 80 - 1) == 13 * 80 and (small == 5.0).all()    # too small: untouched
    with pytest.raises(ValueError):
        afgpu.cep_dct(13, 80, "orthonormal")


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = afgpu.cep_params(80, 13, 2, 2)
    assert lib.afg_cepstra_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, 0, None) == 0        # no records: nothing to do
    bad = afgpu.cep_params(80, 81, 2, 2)
    assert lib.afg_cepstra_hip(0, None, 0, C.byref(bad), None, 0, None, 0, None, 0, None) == INVALID      # ... but the parameters count
    assert lib.afg_cepstra_hip(0, None, 0, None, None, 0, None, 0, None, 0, None) == INVALID
    good = (1, 0x1000, 1, C.byref(p), 0x2000, 8000, 0x3000, 1040, 0x4000, 8000, None)
    for at, value in ((1, None), (4, None), (6, None), (8, None), (1, 0x1004), (4, 0x2002), (6, 0x3001), (8, 0x4002), (0, 1 << 32), (2, 1 << 31)):
        args = list(good)
        args[at] = value
        assert lib.afg_cepstra_hip(*args) == INVALID, at
        assert lib.afg_last_error().decode().startswith("afg_cepstra_hip:"), at


def mfcc_opts(mel=None, cep=None, **kw):
    m = afgpu.MelOpts(C.sizeof(afgpu.MelOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, afgpu.mel_params(**(mel or {})), 0, 1, 0.0, 0.0)
    o = afgpu.MfccOpts(C.sizeof(afgpu.MfccOpts), afgpu.CEP_DCT_ORTHO, m, afgpu.cep_params(**(cep or {})), 0.0, 0.0)
    for k, v in kw.items():
        target = o
        while "__" in k:                                         # mel__channels: a field of the embedded structure
            head, k = k.split("__", 1)
            target = getattr(target, head)
        setattr(target, k, v)
    return o


def call_mfcc(n_files, opts, wave, cmvn, d_out=0x1000, out=True):
    """afg_batch_decode_mfcc with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_mfcc(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if wave is None else C.byref(wave),
                                   None if cmvn is None else C.byref(cmvn), d_out, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def test_batch_entry_refuses_its_arguments_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    std, neg = afgpu.norm_params("standard"), (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call_mfcc(1, None, std, std),
        "NULL d_out": call_mfcc(1, mfcc_opts(), std, std, d_out=None),
        "NULL out": call_mfcc(1, mfcc_opts(), std, std, out=False),
        "short struct": call_mfcc(1, mfcc_opts(struct_size=C.sizeof(afgpu.MfccOpts) - 8), std, std),
        # what afg_batch_decode_mel_norm checks
        "short mel struct": call_mfcc(1, mfcc_opts(mel__struct_size=C.sizeof(afgpu.MelOpts) - 8), std, std),
        "no channels": call_mfcc(1, mfcc_opts(mel__channels=0), std, std),
        "mel parameters": call_mfcc(1, mfcc_opts(mel=dict(n_fft=15)), std, std),
        "bank": call_mfcc(1, mfcc_opts(mel__scale=2), std, std),
        "n_out": call_mfcc(1, mfcc_opts(mel__n_out=102), std, std),
        "reflect": call_mfcc(1, mfcc_opts(mel__frames=200), std, std),
        "algorithm": call_mfcc(1, mfcc_opts(mel__algorithm=2), std, std),
        "mel reserved": call_mfcc(1, mfcc_opts(mel__reserved=1), std, std),
        "negative first_frame": call_mfcc(1, mfcc_opts(mel__first_frame=neg), std, std),
        "negative n_files": call_mfcc(-1, mfcc_opts(), std, std),
        "wave mode": call_mfcc(1, mfcc_opts(), afgpu.NormParams(5, 1.0, 0.0, 8.0, 4.0, 0.25), std),
        # its own
        "out_kind power": call_mfcc(1, mfcc_opts(mel=dict(out_kind=afgpu.MEL_POWER)), std, std),
        "n_mels mismatch": call_mfcc(1, mfcc_opts(cep=dict(n_mels=40)), std, std),
        "n_ceps": call_mfcc(1, mfcc_opts(cep=dict(n_ceps=81)), std, std),
        "delta_order": call_mfcc(1, mfcc_opts(cep=dict(delta_order=3)), std, std),
        "delta_win": call_mfcc(1, mfcc_opts(cep=dict(delta_order=1, delta_win=9)), std, std),
        "dct_norm": call_mfcc(1, mfcc_opts(dct_norm=2), std, std),
        "lifter": call_mfcc(1, mfcc_opts(lifter=-22.0), std, std),
        "log_scale": call_mfcc(1, mfcc_opts(log_scale=float("inf")), std, std),
        "cmvn eps": call_mfcc(1, mfcc_opts(), None, afgpu.norm_params("standard", eps=-1.0)),
        "cmvn gain": call_mfcc(1, mfcc_opts(), std, afgpu.norm_params("dynamic_range", gain=float("nan"))),
    }
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    reserved = mfcc_opts()
    reserved.cep.reserved[2] = 1
    rc, msg, _ = call_mfcc(1, reserved, None, None)
    assert rc == INVALID and "reserved[2]" in msg
    rc, msg, _ = call_mfcc(1, mfcc_opts(), None, afgpu.NormParams(5, 1.0, 0.0, 8.0, 4.0, 0.25))      # mode 5 stays refused
    assert rc == INVALID and "afg_norm_params.mode 5" in msg
    for wave, cmvn in ((None, None), (std, None), (None, std), (std, std)):                # NULL means none; no file: nothing is touched
        rc, _, res = call_mfcc(0, mfcc_opts(log_scale=0.0), wave, cmvn)                     # (log_scale 0 means 1)
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entry_checks_its_arguments():
    for kw in (dict(frames=0), dict(frames=16000, n_out=102), dict(frames=16000, cmvn="wisper"), dict(frames=16000, wave_norm="unit"),
               dict(frames=16000, dct_norm="orthonormal"), dict(frames=16000, algorithm="fast"), dict(frames=16000, n_mfcc=0),
               dict(frames=16000, channels=2)):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mfcc([b"x"], **kw)
