"""The host half of the convolution stage (include/afg.h: afg_convolve_*), without a device: the symbols and record sizes, the
two layouts, and every refusal of afg_convolve_bank_check and afg_convolve_check_rows with its status and a message of its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import convolve_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["afg_convolve_bank_layout", "afg_convolve_bank_check", "afg_convolve_bank_hip", "afg_convolve_layout", "afg_convolve_bound",
       "afg_convolve_check_rows", "afg_convolve_hip"]
B, SPEC, TABLE, TILE = 1024, 2050, 4096, 4096


def status_of(name):
    header = open(os.path.join(ROOT, "include", "afg.h")).read()
    return int(re.search(rf"\b{name}\s*=\s*(-?\d+)", header).group(1))


def test_the_symbols_and_the_record_sizes():
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
    assert code.index("afg_pvoc_hip(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    assert C.sizeof(afgpu.ConvolveParams) == 32 and afgpu.CONV_KERNEL_DTYPE.itemsize == 24 and afgpu.CONV_ROW_DTYPE.itemsize == 48
    assert [afgpu.CONV_KERNEL_DTYPE.fields[n][1] for n in afgpu.CONV_KERNEL_DTYPE.names] == [0, 8, 16, 20]
    assert [afgpu.CONV_ROW_DTYPE.fields[n][1] for n in afgpu.CONV_ROW_DTYPE.names] == [0, 8, 16, 24, 32, 36, 40, 44]
    src = ("#include <stdio.h>\n#include \"afg.h\"\nint main(void){printf(\"%zu %zu %zu %d %d %d %d %d %d\", sizeof(afg_convolve_params), "
           "sizeof(afg_convolve_kernel), sizeof(afg_convolve_row), AFG_CONV_BLOCK, AFG_CONV_MAX_TAPS, AFG_CONV_DIRECT_MAX, AFG_CONV_DIRECT_TILE, "
           "AFG_CONV_TABLE_FLOATS, AFG_CONV_SPEC_FLOATS);return 0;}")
    exe = os.path.join(ROOT, "audio-formats_amd", "build", "convolve_sizes")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["cc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    assert subprocess.check_output([exe], text=True).split() == ["32", "24", "48", "1024", "65536", "128", "4096", "4096", "2050"]
    assert (afgpu.CONV_BLOCK, afgpu.CONV_MAX_TAPS, afgpu.CONV_DIRECT_MAX, afgpu.CONV_DIRECT_TILE, afgpu.CONV_TABLE_FLOATS, afgpu.CONV_SPEC_FLOATS) == \
        (cm.B, cm.MAX_TAPS, cm.DIRECT_MAX, cm.DIRECT_TILE, cm.TABLE_FLOATS, cm.SPEC_FLOATS) == (B, 65536, 128, TILE, TABLE, SPEC)
    for name in ("convolve_params", "convolve_bank_layout", "convolve_bank_check", "convolve_bank", "convolve_layout", "convolve_bound",
                 "convolve_check_rows", "convolve", "ConvolveBank", "convolve_tensor"):
        assert callable(getattr(afgpu, name))


def bank_of(taps):
    """kernels of these taps packed one behind the other; returns (records, bank floats, spectrum floats)"""
    k = np.zeros(len(taps), afgpu.CONV_KERNEL_DTYPE)
    k["taps"] = taps
    k["bank_off"] = np.concatenate([[0], np.cumsum(taps)[:-1]])
    return k, int(np.sum(taps)), afgpu.convolve_bank_layout(k)


def rows_of(specs):
    """(frames, kernel, out_first, out_frames) packed one behind the other; returns (rows, in floats, out floats)"""
    r = np.zeros(len(specs), afgpu.CONV_ROW_DTYPE)
    a = b = 0
    for i, (frames, kernel, first, count) in enumerate(specs):
        r[i] = (a, b, 0, 0, frames, kernel, first, count)
        a += frames
        b += count
    return r, a, b


def test_the_bank_layout():
    taps = [1, 1024, 1025, 65536, 128, 129]
    k, bank, spec = bank_of(taps)
    parts = [1, 1, 2, 64, 1, 1]
    assert [cm.partitions(t) for t in taps] == parts
    assert list(k["spec_off"]) == [TABLE + SPEC * s for s in np.cumsum([0] + parts)[:-1]]
    assert spec == TABLE + SPEC * sum(parts) and bank == sum(taps)
    afgpu.convolve_bank_check(k, bank, spec)
    afgpu.convolve_bank_check(k, bank + 5, spec + 5)


def test_the_row_layout():
    taps = [1, 1024, 1025, 65536, 128, 129]
    k, _, _ = bank_of(taps)
    prm = afgpu.convolve_params()
    # direct rows: tiles of 4096 delivered samples, no work
    r, _, _ = rows_of([(10000, 0, 0, c) for c in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)] + [(5000, 4, 3, 5000)])
    tiles, work = afgpu.convolve_layout(r, k, prm)
    counts = [0, 1, 1, 1, 2, 3, 2]
    assert tiles == sum(counts) and work == 0
    assert list(r["first_tile"]) == list(np.cumsum([0] + counts)[:-1]) and not r["work_off"].any()
    # FFT rows: one tile per block the range meets; the pairs j_lo .. j_hi
    cases = [
        ((3000, 1, 0, 3000 + 1023), 4, 4),            # taps 1024, full: blocks 0 .. 3; pairs 0 .. 3 (pair 3 is the last that meets the row)
        ((3000, 1, 1000, 100), 2, 2),                 # blocks 0 .. 1, pairs 0 .. 1
        ((3000, 2, 2048, 1), 1, 2),                   # taps 1025, P = 2: block 2, pairs 1 .. 2
        ((1500, 3, 0, 1500 + 65535), 66, 3),          # taps 65536, full: 67035 samples are blocks 0 .. 65; pairs 0 .. 2
        ((1500, 3, 66000, 1000), 2, 2),               # blocks 64 .. 65; pairs max(0, 64 - 63) .. min(65, 2): 1 .. 2
        ((1, 5, 0, 129), 1, 1),                       # taps 129: block 0, pair 0
        ((5000, 5, 64, 0), 0, 0),                     # no output: nothing
        ((5000, 0, 0, 5000), 2, 0),                   # a direct row among them
    ]
    r, _, _ = rows_of([c[0] for c in cases])
    tiles, work = afgpu.convolve_layout(r, k, prm)
    assert list(r["first_tile"]) == list(np.cumsum([0] + [c[1] for c in cases])[:-1]) and tiles == sum(c[1] for c in cases)
    assert list(r["work_off"]) == [SPEC * v for v in np.cumsum([0] + [c[2] for c in cases])[:-1]] and work == SPEC * sum(c[2] for c in cases)
    # direct_max = 0: the short kernels take the FFT path too
    r, _, _ = rows_of([(5000, 0, 0, 5000), (5000, 4, 100, 5000)])
    tiles, work = afgpu.convolve_layout(r, k, afgpu.convolve_params(0))
    assert tiles == 5 + 5 and work == SPEC * (5 + 5)
    # the work plane: about twice the input plus one block per row
    r, _, _ = rows_of([(480000, 2, 0, 480000)])
    _, work = afgpu.convolve_layout(r, k, prm)
    assert work == SPEC * 469 and 2.0 < work / 480000 < 2.01


PRM = afgpu.convolve_params()


def refused(message, status=-1, **kw):
    """one change to a launch that passes, and what check_rows says"""
    taps = kw.pop("taps", [64, 2000])
    k, bank, spec = bank_of(taps)
    specs = kw.pop("rows", [(3000, 0, 0, 3063), (3000, 1, 10, 3000), (0, 1, 0, 0)])
    r, a, b = rows_of(specs)
    prm = kw.pop("prm", PRM)
    tiles, work = afgpu.convolve_layout(r, k, prm)
    sizes = dict(in_floats=a, bank_floats=bank, spec_floats=spec, work_floats=work, out_floats=b)
    edit = kw.pop("edit", None)
    if edit:
        edit(r, k)
    tiles += kw.pop("tiles", 0)
    plane_at = kw.pop("plane_at", None)
    for name, v in kw.items():
        sizes[name] += v
    if message is None:
        afgpu.convolve_check_rows(r, tiles, k, prm, plane_at=plane_at, **sizes)
        return
    with pytest.raises(afgpu.AfgError, match=message) as e:
        afgpu.convolve_check_rows(r, tiles, k, prm, plane_at=plane_at, **sizes)
    assert f"({status})" in str(e.value), str(e.value)


def test_a_launch_that_passes():
    refused(None)
    refused(None, prm=afgpu.convolve_params(0))
    refused(None, plane_at=[0, 10 ** 6, 2 * 10 ** 6, 3 * 10 ** 6, 4 * 10 ** 6])
    afgpu.convolve_check_rows(np.zeros(0, afgpu.CONV_ROW_DTYPE), 0, np.zeros(0, afgpu.CONV_KERNEL_DTYPE), PRM, 0, 0, TABLE, 0, 0)


def test_every_refusal_with_its_message():
    unsupported = status_of("AFG_ERR_UNSUPPORTED")
    assert unsupported != -1
    def set_(field, i, v, kernels=False):
        def edit(r, k):
            (k if kernels else r)[field][i] = v
        return edit
    refused("taps 0", edit=set_("taps", 0, 0, True))
    refused("taps 65537: at most 65536", status=unsupported, edit=set_("taps", 1, 65537, True))
    refused(r"direct_max 129: 0 \.\. 128", prm=afgpu.convolve_params(129), rows=[(0, 0, 0, 0)])
    bad = afgpu.convolve_params()
    bad.reserved[3] = 1
    refused("reserved: must be 0", prm=bad, rows=[(0, 0, 0, 0)])
    refused("afg_convolve_kernel 1: reserved must be 0", edit=set_("reserved", 1, 7, True))
    refused("afg_convolve_row 1: kernel 2 outside the bank of 2", edit=set_("kernel", 1, 2))
    refused("afg_convolve_row 0: samples 0 .. 3064, but 3000 frames and 64 taps make a line of 3063", rows=[(3000, 0, 0, 3064)])
    refused("afg_convolve_row 0: samples 4999 .. 5000, but 3000 frames and 2000 taps make a line of 4999", rows=[(3000, 1, 4999, 1)])
    refused("afg_convolve_row 1: 5 samples of a row without frames", rows=[(3000, 0, 0, 3063), (0, 1, 0, 5)])
    refused("afg_convolve_row 0: frames 2147483648: at most", rows=[(1 << 31, 0, 0, 5)])
    refused("afg_convolve_row 1: the row's 3000 samples leave the input", in_floats=-1)
    refused("afg_convolve_row 0: the row's 3000 samples leave the input", edit=set_("in_off", 0, (1 << 64) - 100))
    refused("afg_convolve_row 1: the 3000 delivered samples leave the output", out_floats=-1)
    refused("afg_convolve_kernel 1: its 2000 taps leave the bank", bank_floats=-1)
    refused("afg_convolve_kernel 1: its 2000 taps leave the bank", edit=set_("bank_off", 1, (1 << 64) - 10, True))
    refused("spec_floats 10245: afg_convolve_bank_layout gives 10246", spec_floats=-1)
    refused("work_floats 6149: afg_convolve_layout gives 6150", work_floats=-1)
    refused("afg_convolve_kernel 1: spec_off 6148, afg_convolve_bank_layout gives 6146", edit=set_("spec_off", 1, TABLE + SPEC + 2, True))
    refused("afg_convolve_row 1: first_tile 2, afg_convolve_layout gives 1", edit=set_("first_tile", 1, 2))
    refused("afg_convolve_row 2: work_off 0, afg_convolve_layout gives 6150", edit=set_("work_off", 2, 0))
    refused("n_tiles 5, afg_convolve_layout gives 4", tiles=1)
    # planes that share an allocation: in, bank, spectra, work, out
    at = [0, 10 ** 6, 2 * 10 ** 6, 3 * 10 ** 6, 4 * 10 ** 6]
    def moved(q, v):
        return at[:q] + [v] + at[q + 1:]
    refused("afg_convolve_row 0: its output overlaps the bank", plane_at=moved(4, 10 ** 6 + 2063))
    refused("its output overlaps the spectra", plane_at=moved(4, 2 * 10 ** 6 - 1))
    refused("its output overlaps the work plane", plane_at=moved(4, 3 * 10 ** 6 + 6149))
    refused(None, plane_at=moved(4, 3 * 10 ** 6 + 6150))
    refused("output overlaps a row of record", plane_at=moved(4, 2999))
    refused(None, plane_at=moved(4, 6000))
    refused("output overlaps a row of record", plane_at=at, edit=set_("out_off", 1, 3062))
    refused("the work plane overlaps the input plane", plane_at=moved(3, 5999))
    refused("the work plane overlaps the bank", plane_at=moved(3, 10 ** 6 - 6149))
    refused("the work plane overlaps the spectra", plane_at=moved(3, 2 * 10 ** 6 + 10245))


def test_the_bank_refusals_and_the_layouts_own():
    k, bank, spec = bank_of([64, 2000])
    with pytest.raises(afgpu.AfgError, match="spec_floats"):
        afgpu.convolve_bank_check(k, bank, spec - 1)
    with pytest.raises(afgpu.AfgError, match="leave the bank"):
        afgpu.convolve_bank_check(k, bank - 1, spec)
    for taps, msg in ((0, "taps 0"), (65537, "taps 65537")):
        z = np.zeros(1, afgpu.CONV_KERNEL_DTYPE)
        z["taps"] = taps
        with pytest.raises(afgpu.AfgError, match=msg):
            afgpu.convolve_bank_layout(z)
    r, _, _ = rows_of([(100, 2, 0, 100)])
    with pytest.raises(afgpu.AfgError, match="kernel 2 outside the bank"):
        afgpu.convolve_layout(r, k, PRM)
    r, _, _ = rows_of([(100, 0, 0, 100)])
    with pytest.raises(afgpu.AfgError, match="direct_max"):
        afgpu.convolve_layout(r, k, afgpu.convolve_params(200))


def test_the_caps():
    # 2^31 tiles from few records: direct rows of 2^31 - 65536 frames make 2^19 - 16 tiles each
    k, bank, spec = bank_of([1])
    n = 4200
    r = np.zeros(n, afgpu.CONV_ROW_DTYPE)
    r["frames"] = r["out_frames"] = (1 << 31) - 65536
    r["in_off"] = r["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64((1 << 31) - 65536)
    tiles, work = afgpu.convolve_layout(r, k, PRM)
    assert tiles == n * ((1 << 19) - 16) > (1 << 31) - 1 and work == 0
    with pytest.raises(afgpu.AfgError, match=r"2\^31 - 1 tiles"):
        afgpu.convolve_check_rows(r, tiles, k, PRM, n << 31, bank, spec, 0, n << 31)
    m = 4090
    assert m * ((1 << 19) - 16) <= (1 << 31) - 1
    tiles, _ = afgpu.convolve_layout(r[:m], k, PRM)
    afgpu.convolve_check_rows(r[:m].copy(), tiles, k, PRM, n << 31, bank, spec, 0, n << 31)
