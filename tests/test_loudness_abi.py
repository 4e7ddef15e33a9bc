"""afg_kweight_design / afg_loudness_lufs / afg_loudness_layout / afg_loudness_check_groups / afg_loudness_hip /
afg_batch_decode_loudnorm without a GPU: the symbols, the structures, the design and the layout against
tests/loudness_model.py, and every refusal that needs no device, each with its status and its own message."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import filter_model as fm
import loudness_model as lm
from test_collate_abi import c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_kweight_design", "afg_loudness_lufs", "afg_loudness_layout", "afg_loudness_check_groups", "afg_loudness_hip",
       "afg_batch_decode_loudnorm")
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
        assert re.search(rf"\b{name}\s*\(", d), name                                         # the D prototypes
        assert name in afgpu.ABI_SYMBOLS
    assert code.index("afg_batch_decode_filtered(") < min(code.index(n + "(") for n in NEW)   # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    for const, value in (("AFG_LOUDNESS_K", afgpu.LOUDNESS_K), ("AFG_LOUDNESS_UNGATED", afgpu.LOUDNESS_UNGATED),
                         ("AFG_LOUDNESS_GAIN_CLAMPED", afgpu.LOUDNESS_GAIN_CLAMPED), ("AFG_LOUDNESS_PEAK_CLAMPED", afgpu.LOUDNESS_PEAK_CLAMPED)):
        assert re.search(rf"#define\s+{const}\s+{value}u?\b", code), const
        assert re.search(rf"\b{const}\s*=\s*{value}\b", d), const
    assert afgpu.LOUDNESS_K == lm.K_L == afgpu.FILTER_K
    assert (afgpu.LOUDNESS_UNGATED, afgpu.LOUDNESS_GAIN_CLAMPED, afgpu.LOUDNESS_PEAK_CLAMPED) == (lm.UNGATED, lm.GAIN_CLAMPED, lm.PEAK_CLAMPED)
    for name in ("LoudnessParams", "LoudnessGroup", "LoudnessCounts", "LoudnessStats", "LOUDNESS_GROUP_DTYPE", "LOUDNESS_STATS_DTYPE",
                 "kweight_design", "loudness_lufs", "loudness_params", "loudness_layout", "loudness_check_groups", "loudness", "loudness_tensor",
                 "batch_decode_tensor_loudnorm"):
        assert hasattr(afgpu, name), name


def test_structures_match_the_header():
    for struct, cls, size, model in (("afg_loudness_params", afgpu.LoudnessParams, 96, None), ("afg_loudness_group", afgpu.LoudnessGroup, 64, lm.GROUP_DTYPE),
                                     ("afg_loudness_counts", afgpu.LoudnessCounts, 16, None), ("afg_loudness_stats", afgpu.LoudnessStats, 40, lm.STATS_DTYPE)):
        names = [f[0] for f in cls._fields_]
        got, offs = c_layout(struct, names)
        assert got == C.sizeof(cls) == size, struct
        assert offs == [getattr(cls, n).offset for n in names], struct
        if model is not None:
            assert model.itemsize == size and [model.fields[n][1] for n in names] == offs, struct
    assert afgpu.LOUDNESS_GROUP_DTYPE.itemsize == 64 and afgpu.LOUDNESS_STATS_DTYPE.itemsize == 40


def test_the_design_is_the_models_and_the_standards():
    for rate in (8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000):
        got, want = afgpu.kweight_design(rate), lm.kweight(rate)
        assert len(got) == 2
        for g, w in zip(got, want):
            assert np.abs(np.array(g) - np.array(w)).max() <= 1e-15 * np.abs(np.array(w)).max(), (rate, g, w)
            assert fm.stable(g)
        assert got[1][:3] == (1.0, -2.0, 1.0)
        bound = afgpu.filter_bound(got)                          # the cascade passes the filter stage's own checks
        assert abs(bound / lm.filter_bound(rate) - 1.0) < 1e-9
    for got, want in zip(afgpu.kweight_design(48000), lm.BS1770_48K):
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12
    lib = afgpu.lib()
    keep = afgpu.FilterParams()
    keep.n_sections = 7
    for rate in (0, 7999, 192001, 0xffffffff):
        assert lib.afg_kweight_design(rate, C.byref(keep)) == INVALID and b"samplerate" in lib.afg_last_error() and keep.n_sections == 7
        with pytest.raises(ValueError):
            afgpu.kweight_design(rate)
    assert lib.afg_kweight_design(48000, None) == INVALID and b"NULL" in lib.afg_last_error()
    assert afgpu.loudness_lufs(0.0) == -math.inf and afgpu.loudness_lufs(1.0) == -0.691
    assert abs(afgpu.loudness_lufs(10.0 ** -2.2309) + 23.0) < 1e-12


def groups_of(shapes, stride=None, offs=None):
    g = np.zeros(len(shapes), afgpu.LOUDNESS_GROUP_DTYPE)
    at = 0
    for k, (rows, valid) in enumerate(shapes):
        g[k]["rows"], g[k]["valid"], g[k]["stride"] = rows, valid, stride if stride is not None else valid
        g[k]["in_off"] = g[k]["out_off"] = at if offs is None else offs[k]
        at += rows * int(g[k]["stride"])
    return g, at


def test_the_layout_counts_sub_blocks_and_blocks():
    for rate in (8000, 11025, 44100, 192000):
        step = lm.step_of(rate)
        prm = afgpu.loudness_params(rate)
        shapes = [(1, 0), (2, 4 * step - 1), (1, 4 * step), (8, 5 * step - 1), (3, 5 * step), (1, 0), (2, 100 * step + 17), (1, 1)]
        g, floats = groups_of(shapes)
        counts = afgpu.loudness_layout(g, prm)
        subs = blocks = 0
        for rec, (rows, valid) in zip(g, shapes):
            assert (rec["first_sub"], rec["first_block"]) == (subs, blocks)
            nb = lm.blocks_of(valid, step)
            subs += rows * ((nb + 3 if nb else 0) + 1) if valid else 0
            blocks += nb
        assert (counts.n_sub, counts.n_blocks) == (subs, blocks)
        afgpu.loudness_check_groups(g, counts, prm, floats, floats, True)
        afgpu.loudness_check_groups(g, counts, afgpu.loudness_params(rate, apply=False), floats, 0, False)
    lib = afgpu.lib()
    counts = afgpu.LoudnessCounts(5, 5)
    assert lib.afg_loudness_layout(None, 0, C.byref(afgpu.loudness_params(4000)), C.byref(counts)) == 0 and (counts.n_sub, counts.n_blocks) == (0, 0)
    assert lib.afg_loudness_layout(None, 2, C.byref(prm), C.byref(counts)) == 0 and b"NULL groups" in lib.afg_last_error()
    assert lib.afg_loudness_layout(None, 0, C.byref(prm), None) == 0 and b"NULL counts" in lib.afg_last_error()
    assert lib.afg_loudness_layout(None, 0, C.byref(prm), C.byref(counts)) == 1


def refused(groups, counts, prm, in_floats, out_floats, same, message):
    lib = afgpu.lib()
    rc = lib.afg_loudness_check_groups(groups.ctypes.data if groups is not None else None, 0 if groups is None else len(groups),
                                       C.byref(counts) if counts is not None else None, C.byref(prm) if prm is not None else None, in_floats, out_floats,
                                       same)
    text = lib.afg_last_error().decode()
    assert rc == INVALID and message in text, (rc, text, message)
    return text


def test_every_refusal_has_its_message():
    lib = afgpu.lib()
    nan, inf = float("nan"), float("inf")
    seen = set()
    # the parameters, which count without groups too -- in the check function, the kernel entry and the batch entry alike
    for kw, message in ((dict(samplerate=7999), "samplerate"), (dict(samplerate=192001), "samplerate"), (dict(target_lufs=nan), "target_lufs"),
                        (dict(target_lufs=201.0), "target_lufs"), (dict(max_peak=-1.0), "max_peak"), (dict(max_peak=inf), "max_peak"),
                        (dict(max_gain=-0.5), "max_gain"), (dict(max_gain=nan), "max_gain"), (dict(weights=[1, -1]), "weights[1]"),
                        (dict(weights=[1] * 7 + [inf]), "weights[7]")):
        args = dict(samplerate=16000)
        args.update(kw)
        prm = afgpu.loudness_params(**args)
        seen.add(refused(None, None, prm, 0, 0, 0, message))
        assert lib.afg_loudness_hip(0, None, None, C.byref(prm), None, 0, None, 0, None, None, None, None) == INVALID and message in lib.afg_last_error().decode()
    prm = afgpu.loudness_params(16000)
    prm.apply = 2
    seen.add(refused(None, None, prm, 0, 0, 0, "apply"))
    prm = afgpu.loudness_params(16000)
    prm.reserved[1] = 3
    seen.add(refused(None, None, prm, 0, 0, 0, "reserved[1]"))
    seen.add(refused(None, None, None, 0, 0, 0, "NULL"))
    prm = afgpu.loudness_params(16000)
    assert lib.afg_loudness_check_groups(None, 0, None, C.byref(prm), 0, 0, 0) == 0
    assert lib.afg_loudness_hip(0, None, None, C.byref(prm), None, 0, None, 0, None, None, None, None) == 0
    # the groups
    good, _ = groups_of([(2, 8000), (1, 6400), (1, 0)], stride=8001)
    floats = 2 * 8001 + 6400                                     # the plane ends with the last group's samples
    counts = afgpu.loudness_layout(good, prm)
    afgpu.loudness_check_groups(good, counts, prm, floats, floats, True)
    top = 2 ** 64 - 1

    def bad(**kw):
        g = good.copy()
        for name, (k, v) in kw.items():
            g[k][name] = v
        return g
    for g, c, inf_, outf, same, message in (
            (bad(rows=(0, 0)), counts, floats, floats, 1, "rows 0"), (bad(rows=(1, 9)), counts, floats, floats, 1, "rows 9"),
            (bad(reserved=(0, [0, 0, 1, 0])), counts, floats, floats, 1, "reserved[2]"),
            (bad(first_sub=(1, 7)), counts, floats, floats, 1, "first_sub"), (bad(first_block=(2, 1)), counts, floats, floats, 1, "first_block"),
            (good, afgpu.LoudnessCounts(counts.n_sub + 1, counts.n_blocks), floats, floats, 1, "n_sub"),
            (good, afgpu.LoudnessCounts(counts.n_sub, counts.n_blocks - 1), floats, floats, 1, "n_blocks"),
            (bad(stride=(0, 7999)), counts, floats, floats, 1, "stride"),
            (good, counts, floats - 1, floats, 0, "leave the input"), (good, counts, floats, floats - 1, 0, "leave the output"),
            (bad(in_off=(1, top - 5)), counts, top, top, 0, "leave the input"),             # an offset that would wrap
            (bad(out_off=(1, top - 5)), counts, top, top, 0, "leave the output"),
            (bad(stride=(0, top - 100)), counts, top, top, 0, "leave the input"),        # a stride that would
            (bad(out_off=(1, 100)), counts, floats, floats, 0, "overlaps"),                  # two outputs
            (bad(out_off=(1, 100)), counts, floats, floats, 1, "overlaps"),
            (bad(out_off=(0, 1)), counts, floats + 1, floats + 1, 1, "overlaps"),            # a group shifted onto itself
            (bad(in_off=(1, 0)), counts, floats, floats, 1, "overlaps")):                    # an output over another group's input
        seen.add(refused(g, c, prm, inf_, outf, same, message))
    assert lib.afg_loudness_check_groups(None, 2, C.byref(counts), C.byref(prm), floats, floats, 1) == INVALID and b"NULL groups" in lib.afg_last_error()
    assert lib.afg_loudness_check_groups(good.ctypes.data, 3, None, C.byref(prm), floats, floats, 1) == INVALID and b"NULL counts" in lib.afg_last_error()
    assert len(seen) >= 24                                        # messages of their own
    # without the product nothing is asked of the output, and inputs may share samples
    measure = afgpu.loudness_params(16000, apply=False)
    afgpu.loudness_check_groups(bad(in_off=(1, 0), out_off=(1, top - 5)), counts, measure, floats, 0, False)
    afgpu.loudness_check_groups(bad(out_off=(0, 1)), counts, prm, floats + 1, floats + 1, False)      # shifted, in two planes
    # the kernel entry's own checks come before any device call
    d = lambda a: C.c_void_p(a)
    cb = C.byref(counts)
    for args, message in (((1, d(0x1000), None, C.byref(prm), d(0x20000), 1000, d(0x30000), 1000, d(0x4000), d(0x5000), d(0x6000), None), "NULL counts"),
                          ((1, None, cb, C.byref(prm), d(0x20000), 1000, d(0x30000), 1000, d(0x4000), d(0x5000), d(0x6000), None), "NULL device pointer"),
                          ((1, d(0x1000), cb, C.byref(prm), d(0x20000), 1000, None, 1000, d(0x4000), d(0x5000), d(0x6000), None), "NULL device pointer"),
                          ((1, d(0x1000), cb, C.byref(prm), d(0x20002), 1000, d(0x30000), 1000, d(0x4000), d(0x5000), d(0x6000), None), "aligned"),
                          ((1, d(0x1000), cb, C.byref(prm), d(0x20000), 1000, d(0x30000), 1000, d(0x4004), d(0x5000), d(0x6000), None), "aligned"),
                          ((1 << 31, d(0x1000), cb, C.byref(prm), d(0x20000), 1000, d(0x30000), 1000, d(0x4000), d(0x5000), d(0x6000), None), "2^31 - 1 groups"),
                          ((1, d(0x1000), cb, C.byref(prm), d(0x20000), 1 << 61, d(0x30000), 1000, d(0x4000), d(0x5000), d(0x6000), None), "2^61"),
                          ((1, d(0x1000), cb, C.byref(prm), d(0x20000), 1000, d(0x20000 + 3996), 1000, d(0x4000), d(0x5000), d(0x6000), None), "overlaps the input plane")):
        assert lib.afg_loudness_hip(*args) == INVALID and message in lib.afg_last_error().decode(), (message, lib.afg_last_error())


def test_the_batch_entry_refuses_before_any_device_call():
    lib = afgpu.lib()
    prm = afgpu.loudness_params(16000)
    opts = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0)
    data = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    out = C.c_void_p(0x1000)

    def call(o=opts, p=prm, d_out=out, r=res, n=1):
        return lib.afg_batch_decode_loudnorm(data, lens, n, C.byref(o) if o is not None else None, C.byref(p) if p is not None else None, d_out, None,
                                             C.byref(r) if r is not None else None)
    for kw, message in ((dict(o=None), "NULL opts"), (dict(p=None), "NULL loudness"), (dict(d_out=None), "NULL d_out"), (dict(r=None), "NULL out"),
                        (dict(p=afgpu.loudness_params(8000)), "is not the tensor's"), (dict(p=afgpu.loudness_params(16000, max_gain=-1.0)), "max_gain"),
                        (dict(n=-1), "")):
        assert call(**kw) == INVALID and message in lib.afg_last_error().decode(), (kw, lib.afg_last_error())
    nine = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 9, 16000, None, 16000, 0, 0, 0, 0)
    assert call(o=nine) == INVALID and b"at most 8 rows" in lib.afg_last_error()
    low = afgpu.ResampleOpts(C.sizeof(afgpu.ResampleOpts), 1, 1, 4000, None, 4000, 1, 0, 0, 0)
    assert call(o=low, p=afgpu.loudness_params(4000)) == INVALID and b"samplerate" in lib.afg_last_error()
    assert call(n=0) == 0 and res.n_files == 0
    for kw in (dict(frames=0), dict(channels=0), dict(channels=9), dict(samplerate=0), dict(samplerate=4000), dict(channels=2, mono=True),
               dict(target_lufs=float("nan")), dict(max_peak=-1.0), dict(weights=[1.0] * 9), dict(weights=[-1.0])):
        args = dict(frames=16000, channels=1, samplerate=16000)
        args.update(kw)
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_loudnorm([b"x"], **args)
