"""afg_trim_layout / afg_trim_check_groups / afg_trim_hip / afg_batch_decode_trimmed without a GPU: the symbols, the structures,
the block and tile counts and every refusal that needs no device, each with its message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import trim_model as tm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_trim_layout", "afg_trim_check_groups", "afg_trim_hip", "afg_batch_decode_trimmed")
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
    assert code.index("afg_batch_decode_mfcc(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    for const, value in (("AFG_TRIM_REF_MAX", afgpu.TRIM_REF_MAX), ("AFG_TRIM_REF_ABS", afgpu.TRIM_REF_ABS)):
        assert re.search(rf"#define\s+{const}\s+{value}\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
    assert (afgpu.TRIM_REF_MAX, afgpu.TRIM_REF_ABS, afgpu.TRIM_TILE) == (tm.REF_MAX, tm.REF_ABS, tm.TILE)
    for name in ("TrimParams", "TrimGroup", "TRIM_GROUP_DTYPE", "TRIM_REGION_DTYPE", "trim_params", "trim_layout", "trim_check_groups", "trim",
                 "batch_decode_tensor_trimmed"):
        assert hasattr(afgpu, name), name
    assert lib.afg_dev_option(b"trim_scratch_bytes", 1 << 20) == 0 and lib.afg_dev_option(b"trim_scratch_bytes", -1) == 0


def test_structures_match_the_header():
    for struct, cls, size in (("afg_trim_params", afgpu.TrimParams, 48), ("afg_trim_group", afgpu.TrimGroup, 64), ("afg_trim_region", afgpu.TrimRegion, 16)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
    for mine, theirs in ((afgpu.TRIM_GROUP_DTYPE, tm.GROUP_DTYPE), (afgpu.TRIM_REGION_DTYPE, tm.REGION_DTYPE)):
        assert mine.itemsize == theirs.itemsize
        assert [(n, mine.fields[n][1]) for n in mine.names] == [(n, theirs.fields[n][1]) for n in theirs.names]
    # the structures beside it are the ones they were
    assert C.sizeof(afgpu.NormParams) == c_layout("afg_norm_params", ["mode"])[0] == 24
    assert C.sizeof(afgpu.NormGroup) == c_layout("afg_norm_group", ["in_off"])[0] == 48
    assert C.sizeof(afgpu.ResampleOpts) == c_layout("afg_resample_opts", ["struct_size"])[0]
    p = afgpu.trim_params()
    assert (p.frame_length, p.hop, p.reference, p.lead, p.trail, list(p.reserved), p.ratio, p.abs_power) == (2048, 512, 0, 0, 0, [0, 0, 0], 1e-6, 1.0)
    assert afgpu.trim_params(top_db=37.0).ratio == 10.0 ** (-37.0 / 10.0) == tm.params(37.0)["ratio"]
    with pytest.raises(ValueError):
        afgpu.trim_params(reference="mean")


def groups_of(shapes, gap=3):
    """one group per (rows, valid, out_rows, out_frames), packed one after the other with `gap` floats between, strides
    valid + 1 and out_frames + 2; returns (groups, in_floats, out_floats)"""
    g = np.zeros(len(shapes), afgpu.TRIM_GROUP_DTYPE)
    a = b = gap
    for k, (rows, valid, out_rows, out_frames) in enumerate(shapes):
        g[k]["in_off"], g[k]["out_off"], g[k]["in_stride"], g[k]["out_stride"] = a, b, valid + 1, out_frames + 2
        g[k]["rows"], g[k]["valid"], g[k]["out_rows"], g[k]["out_frames"] = rows, valid, out_rows, out_frames
        a += (rows - 1) * (valid + 1) + valid + gap
        b += (out_rows - 1) * (out_frames + 2) + out_frames + gap
    return g, a - gap, b - gap


def test_layout_counts_blocks_and_tiles():
    p = afgpu.trim_params()
    for valid, blocks in ((0, 0), (1, 1), (511, 1), (512, 1), (513, 2), (2048, 4), (0xffffffff, 1 << 23)):
        g, _, _ = groups_of([(2, valid, 2, 100)])
        assert afgpu.trim_layout(g, p) == (blocks, 2)
    assert afgpu.trim_layout(groups_of([(1, 0xffffffff, 1, 1)])[0], afgpu.trim_params(frame_length=1, hop=1)) == (0xffffffff, 1)
    for out_frames, tiles in ((0, 0), (1, 3), (4096, 3), (4097, 6), (0xffffffff, 3 << 20)):
        g, _, _ = groups_of([(1, 10, 3, out_frames)])
        assert afgpu.trim_layout(g, p) == (1, tiles)
    shapes = [(1, 0, 1, 5), (2, 1300, 3, 4097), (1, 512, 1, 0), (3, 7, 3, 7), (1, 0, 2, 0), (1, 5000, 1, 9000)]
    g, _, _ = groups_of(shapes)
    assert afgpu.trim_layout(g, p) == (0 + 3 + 1 + 1 + 0 + 10, 1 + 6 + 0 + 3 + 0 + 3)
    assert g["first_block"].tolist() == [0, 0, 3, 4, 5, 5] and g["first_tile"].tolist() == [0, 1, 7, 7, 10, 10]
    mine = g.view(tm.GROUP_DTYPE).copy()
    mine["first_block"] = mine["first_tile"] = 99
    assert tm.layout(mine, tm.params()) == (15, 13) and (mine == g.view(tm.GROUP_DTYPE)).all()
    assert afgpu.trim_layout(g, afgpu.trim_params(frame_length=10, hop=5)) == (0 + 260 + 103 + 2 + 0 + 1000, 13)
    lib = afgpu.lib()
    nb, nt = C.c_uint64(7), C.c_uint64(7)
    assert lib.afg_trim_layout(g.ctypes.data, len(g), C.byref(afgpu.trim_params(frame_length=2048, hop=500)), C.byref(nb), C.byref(nt)) == 0
    assert "frame_length" in lib.afg_last_error().decode() and (nb.value, nt.value) == (0, 0)
    assert lib.afg_trim_layout(g.ctypes.data, len(g), None, C.byref(nb), C.byref(nt)) == 0
    assert lib.afg_trim_layout(g.ctypes.data, len(g), C.byref(p), None, C.byref(nt)) == 0
    assert lib.afg_trim_layout(None, 3, C.byref(p), C.byref(nb), C.byref(nt)) == 0
    assert lib.afg_trim_layout(None, 0, C.byref(p), C.byref(nb), C.byref(nt)) == 1 and (nb.value, nt.value) == (0, 0)


BAD_PARAMS = [dict(hop=0), dict(frame_length=0), dict(frame_length=65536 + 512), dict(frame_length=2048, hop=500), dict(frame_length=1536),
              dict(frame_length=66 * 512), dict(reference=2), dict(top_db=float("inf")), dict(top_db=float("nan")), dict(top_db=-1.0),
              dict(reference="abs", abs_power=0.0), dict(reference="abs", abs_power=float("inf")), dict(reference="abs", abs_power=float("nan"))]


def refused(groups, n_blocks, n_tiles, prm, in_floats, out_floats):
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.trim_check_groups(groups, n_blocks, n_tiles, prm, in_floats, out_floats)
    return str(e.value).split("): ", 1)[1]


def test_every_group_refusal_needs_no_device():
    p = afgpu.trim_params()
    g, in_floats, out_floats = groups_of([(2, 1300, 3, 700), (1, 0, 1, 9), (3, 513, 3, 0), (1, 5000, 2, 4097)])
    blocks, tiles = afgpu.trim_layout(g, p)
    afgpu.trim_check_groups(g, blocks, tiles, p, in_floats, out_floats)
    afgpu.trim_check_groups(g, blocks, tiles, afgpu.trim_params(top_db=-3.0, reference="abs"), in_floats, out_floats)      # a ratio above 1 over an absolute power
    afgpu.trim_check_groups(g, blocks, tiles, afgpu.trim_params(abs_power=-1.0), in_floats, out_floats)                   # abs_power is ignored with REF_MAX
    seen = set()

    def one(change, n_blocks=blocks, n_tiles=tiles, prm=p, in_floats=in_floats, out_floats=out_floats):
        bad = g.copy()
        change(bad)
        msg = refused(bad, n_blocks, n_tiles, prm, in_floats, out_floats)
        assert msg.startswith("afg_trim_group") and msg not in seen, msg
        seen.add(msg)

    one(lambda b: b["rows"].__setitem__(0, 0))
    one(lambda b: b["rows"].__setitem__(0, 65536) or b["out_rows"].__setitem__(0, 65536))
    one(lambda b: b["out_rows"].__setitem__(0, 1))              # fewer output rows than input rows
    one(lambda b: b["in_stride"].__setitem__(0, 1299))          # a stride smaller than the row ...
    one(lambda b: b["out_stride"].__setitem__(3, 4096))
    one(lambda b: None, in_floats=in_floats - 1)                # rows outside their input plane ...
    one(lambda b: None, out_floats=out_floats - 1)              # ... their output plane ...
    one(lambda b: b["in_off"].__setitem__(3, 2 ** 64 - 4))     # ... by an offset that would wrap
    one(lambda b: b["out_off"].__setitem__(0, 2 ** 64 - 4))
    one(lambda b: b["in_stride"].__setitem__(0, 2 ** 63))       # ... by a stride that would
    one(lambda b: b["out_stride"].__setitem__(3, 2 ** 63))
    one(lambda b: b["first_block"].__setitem__(2, 2))           # a wrong first_block, first_tile or count
    one(lambda b: b["first_tile"].__setitem__(1, 2))
    one(lambda b: None, n_blocks=blocks + 1)
    one(lambda b: None, n_tiles=tiles - 1)
    assert len(seen) == 15
    ok = g.copy()                                               # a single row's stride is not looked at; nor the planes of a group without floats
    ok["in_stride"][3] = ok["out_stride"][1] = 0
    ok["in_off"][1] = ok["out_off"][2] = 2 ** 64 - 1
    afgpu.trim_check_groups(ok, blocks, tiles, p, in_floats, out_floats)
    for case in BAD_PARAMS:
        prm = afgpu.trim_params(**case)
        msg = refused(g, blocks, tiles, prm, in_floats, out_floats)
        assert msg.startswith("afg_trim_params.") and msg not in seen, msg
        seen.add(msg)
        assert afgpu.lib().afg_trim_check_groups(None, 0, 0, 0, C.byref(prm), 0, 0) == INVALID          # the parameters alone
    prm = afgpu.trim_params(top_db=-0.5)
    assert "at most 1" in refused(g, blocks, tiles, prm, in_floats, out_floats)                          # REF_MAX: a ratio above 1
    for k in range(3):
        prm = afgpu.trim_params()
        prm.reserved[k] = 1
        assert refused(g, blocks, tiles, prm, in_floats, out_floats).startswith(f"afg_trim_params.reserved[{k}]")
    lib = afgpu.lib()
    assert lib.afg_trim_check_groups(None, 0, 0, 0, C.byref(p), 0, 0) == 0
    assert lib.afg_trim_check_groups(g.ctypes.data, len(g), blocks, tiles, None, in_floats, out_floats) == INVALID
    assert lib.afg_trim_check_groups(None, 1, 0, 0, C.byref(p), 0, 0) == INVALID
    # the extremes: the longest row, the shortest hop, the largest frame
    wide, wi, wo = groups_of([(2, 0xffffffff, 2, 0xffffffff)])
    for prm in (afgpu.trim_params(frame_length=1, hop=1), afgpu.trim_params(frame_length=65536, hop=1024), afgpu.trim_params(frame_length=64, hop=1)):
        nb, nt = afgpu.trim_layout(wide, prm)
        afgpu.trim_check_groups(wide, nb, nt, prm, wi, wo)
        assert "leave the input" in refused(wide, nb, nt, prm, wi - 1, wo)


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = afgpu.trim_params()
    assert lib.afg_trim_hip(0, None, 0, 0, C.byref(p), None, 0, None, 0, None, None, None) == 0         # no groups: nothing to do
    bad = afgpu.trim_params(frame_length=2048, hop=500)
    assert lib.afg_trim_hip(0, None, 0, 0, C.byref(bad), None, 0, None, 0, None, None, None) == INVALID     # ... but the parameters count
    assert lib.afg_last_error().decode().startswith("afg_trim_params.frame_length")
    assert lib.afg_trim_hip(0, None, 0, 0, None, None, 0, None, 0, None, None, None) == INVALID
    good = (1, 0x1000, 2, 1, C.byref(p), 0x20000, 1000, 0x30000, 1000, 0x4000, 0x5000, None)
    seen = set()
    for at, value in ((1, None), (5, None), (7, None), (9, None), (10, None), (1, 0x1004), (5, 0x20002), (7, 0x30001), (9, 0x4004), (10, 0x5004),
                      (0, 1 << 31), (3, 1 << 31), (2, 1 << 35), (6, 1 << 61), (7, 0x20000 + 3996), (7, 0x20000 - 3996), (7, 0x20000)):
        args = list(good)
        args[at] = value
        assert lib.afg_trim_hip(*args) == INVALID, (at, value)
        msg = lib.afg_last_error().decode()
        assert msg.startswith("afg_trim_hip:"), (at, msg)
        seen.add(msg)
    assert len(seen) == 5                                        # NULL, alignment, the launch's caps, a plane's size, overlap


def resample_opts(**kw):
    o = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def call_trimmed(n_files, opts, trim, scan_frames=0, d_out=0x1000, out=True, regions=False):
    """afg_batch_decode_trimmed with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs, lens = (C.c_char_p * 1)(b"x"), (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    rec = np.zeros(1, afgpu.TRIM_REGION_DTYPE)
    rc = lib.afg_batch_decode_trimmed(ptrs, lens, n_files, None if opts is None else C.byref(opts), None if trim is None else C.byref(trim),
                                      scan_frames, d_out, rec.ctypes.data if regions else None, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def test_batch_entry_refuses_its_arguments_before_any_device_call():
    """every one of them is AFG_ERR_INVALID with a message of its own -- on a machine without a GPU a device call would have
    answered AFG_ERR_NO_DEVICE instead"""
    p, neg = afgpu.trim_params(), (C.c_int64 * 1)(-1)
    cases = {
        "NULL opts": call_trimmed(1, None, p),
        "NULL trim": call_trimmed(1, resample_opts(), None),
        "NULL d_out": call_trimmed(1, resample_opts(), p, d_out=None),
        "NULL out": call_trimmed(1, resample_opts(), p, out=False),
        "scan_frames below frames": call_trimmed(1, resample_opts(), p, scan_frames=15999),
        # what afg_batch_decode_resampled refuses
        "short struct": call_trimmed(1, resample_opts(struct_size=C.sizeof(afgpu.ResampleOpts) - 8), p),
        "no channels": call_trimmed(1, resample_opts(channels=0), p),
        "samplerate": call_trimmed(1, resample_opts(samplerate=0), p),
        "mono with two channels": call_trimmed(1, resample_opts(channels=2), p),
        "in_channels": call_trimmed(1, resample_opts(in_channels=1 << 16), p),
        "max_in_rate": call_trimmed(1, resample_opts(max_in_rate=(1 << 20) + 1), p),
        "lowpass_width": call_trimmed(1, resample_opts(lowpass_width=65), p),
        "negative n_files": call_trimmed(-1, resample_opts(), p),
        "negative first_frame": call_trimmed(1, resample_opts(first_frame=neg), p),
        "a scratch row too long": call_trimmed(1, resample_opts(samplerate=8000), p, scan_frames=0xffffffff),
        # the trim parameters
        "hop": call_trimmed(1, resample_opts(), afgpu.trim_params(hop=0)),
        "frame_length": call_trimmed(1, resample_opts(), afgpu.trim_params(frame_length=2048, hop=500)),
        "k": call_trimmed(1, resample_opts(), afgpu.trim_params(frame_length=1536)),
        "reference": call_trimmed(1, resample_opts(), afgpu.trim_params(reference=2)),
        "ratio": call_trimmed(1, resample_opts(), afgpu.trim_params(top_db=float("nan"))),
        "ratio above 1": call_trimmed(1, resample_opts(), afgpu.trim_params(top_db=-1.0)),
        "abs_power": call_trimmed(1, resample_opts(), afgpu.trim_params(reference="abs", abs_power=-1.0)),
    }
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    reserved = afgpu.trim_params()
    reserved.reserved[1] = 1
    rc, msg, _ = call_trimmed(1, resample_opts(), reserved, regions=True)
    assert rc == INVALID and "reserved[1]" in msg
    for scan, regions in ((0, False), (16000, True), (64000, True)):                       # no file: nothing is touched
        rc, _, res = call_trimmed(0, resample_opts(), p, scan_frames=scan, regions=regions)
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entry_checks_its_arguments():
    for kw in (dict(frames=0), dict(channels=0), dict(samplerate=0), dict(channels=2, mono=True), dict(scan_frames=15999), dict(scan_frames=1 << 32),
               dict(hop=0), dict(frame_length=2048, hop=500), dict(frame_length=1536), dict(reference="mean"), dict(top_db=float("nan")),
               dict(top_db=-1.0), dict(reference="abs", abs_power=0.0)):
        args = dict(frames=16000, channels=1, samplerate=16000)
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_trimmed([b"x"], **args)
