"""The host half of the inverse STFT stage (include/afg.h: afg_istft_*), without a device: the symbols and struct sizes, the
tile and the layout, the envelope against tests/istft_model.py, and every refusal of afg_istft_check_rows with its status and a
message of its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import afgpu
import istft_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["afg_istft_tile_samples", "afg_istft_layout", "afg_istft_envelope_min", "afg_istft_check_rows", "afg_istft_hip"]
INVALID, UNSUPPORTED = -1, None                                 # (UNSUPPORTED is read from the header below)


def status_of(name):
    header = open(os.path.join(ROOT, "include", "afg.h")).read()
    return int(re.search(rf"\b{name}\s*=\s*(-?\d+)", header).group(1))


def test_the_symbols_and_the_struct_sizes():
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
    assert code.index("afg_batch_decode_loudnorm(") < min(code.index(n + "(") for n in NEW)      # appended; the ABI version is unchanged
    assert lib.afg_abi_version() == 2
    assert C.sizeof(afgpu.IstftParams) == 32 and afgpu.ISTFT_ROW_DTYPE.itemsize == 40
    assert [afgpu.ISTFT_ROW_DTYPE.fields[n][1] for n in afgpu.ISTFT_ROW_DTYPE.names] == [0, 8, 16, 24, 28, 32, 36]
    src = "#include <stdio.h>\n#include \"afg.h\"\nint main(void){printf(\"%zu %zu\", sizeof(afg_istft_params), sizeof(afg_istft_row));return 0;}"
    exe = os.path.join(ROOT, "audio-formats_amd", "build", "istft_sizes")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["cc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    assert subprocess.check_output([exe], text=True).split() == ["32", "40"]
    for name in ("istft_params", "istft_tile_samples", "istft_layout", "istft_envelope_min", "istft_check_rows", "istft", "istft_tensor"):
        assert callable(getattr(afgpu, name))


def records(prm, specs):
    """rows of (n_frames, out_first, out_frames[, in_pitch]) packed one behind the other; returns (rows, in_floats, out_floats)"""
    rows = np.zeros(len(specs), afgpu.ISTFT_ROW_DTYPE)
    n_bins = prm.n_fft // 2 + 1
    a = b = 0
    for k, s in enumerate(specs):
        f, first, count = s[:3]
        pitch = s[3] if len(s) > 3 else f
        rows[k] = (a, b, 0, f, pitch, first, count)
        a += 2 * n_bins * pitch
        b += count
    return rows, a, b


def test_tile_and_layout():
    for shape, tile in (((400, 160, 400, True), 10240), ((1024, 256, 1024, True), 16384), ((16, 4, 16, True), 256), ((16, 1, 16, True), 256),
                        ((2048, 512, 2048, True), 16384), ((75, 20, 60, True), 1280)):
        prm = afgpu.istft_params(*shape)
        assert afgpu.istft_tile_samples(prm) == tile and tile % 256 == 0
        counts = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5, 0, 2 * tile]
        rows, _, _ = records(prm, [(1 + (c + prm.hop - 1) // prm.hop, 0, c) for c in counts])
        tiles = afgpu.istft_layout(rows, prm)
        assert tiles == sum(-(-c // tile) for c in counts)
        assert list(rows["first_tile"]) == list(np.cumsum([0] + [-(-c // tile) for c in counts])[:-1])


@pytest.mark.parametrize("shape", [(400, 400, 160, True), (400, 300, 100, True), (75, 60, 20, True), (30, 30, 15, True), (16, 16, 4, True), (16, 16, 1, True),
                                   (1024, 1024, 256, False), (2048, 2048, 512, True)], ids=lambda s: "-".join(map(str, s)))
def test_the_envelope_against_the_model(shape):
    n_fft, win, hop, center = shape
    prm = afgpu.istft_params(n_fft, hop, win, center)
    n_lo, pad = (n_fft - win) // 2, (n_fft // 2 if center else 0)
    for frames in (1, 2, 5, 40):
        D = im.envelope(n_fft, win, hop, frames)
        line = len(D)
        ranges = [(0 if center else n_lo + 1, None), (n_lo + 1, 7), (max(0, line - pad - 9), 9)]
        if center and frames > 1:
            ranges.append((0, hop * (frames - 1)))                # torch.istft's default length
        for first, count in ranges:
            count = line - pad - first if count is None else count
            if count < 1 or pad + first + count > line:
                continue
            want = D[pad + first:pad + first + count].min()
            if want < 1e-9:
                continue                                         # (refusals have their own test)
            got = afgpu.istft_envelope_min(prm, frames, first, count)
            assert abs(got - want) <= 1e-6 * want, (frames, first, count, got, want)
    # a long row costs no pass over its samples: 2^32 - 1 samples of 2^26 frames, at once
    many = min((1 << 32) // hop, (1 << 32) - 1)
    count = min((1 << 32) - 1, n_fft + hop * (many - 1) - pad - n_lo - 1)
    got = afgpu.istft_envelope_min(prm, many, n_lo + 1, count)
    few = im.envelope(n_fft, win, hop, 40)
    short = n_fft + hop * (many - 1) - (pad + n_lo + 1 + count)                   # what the range leaves of the line's end
    want = few[pad + n_lo + 1:len(few) - short].min()                              # (the two lines agree counted from either end)
    assert abs(got - want) <= 1e-6 * want


def test_every_refusal_has_its_status_and_a_message_of_its_own():
    lib = afgpu.lib()
    unsupported = status_of("AFG_ERR_UNSUPPORTED")
    prm = afgpu.istft_params(400, 160, 400, True)
    tile = afgpu.istft_tile_samples(prm)
    table = 400 + 2 * 400
    rows, a, b = records(prm, [(11, 0, 1600), (5, 3, 600, 9), (0, 0, 0), (200, 0, 2 * tile + 7)])
    tiles = afgpu.istft_layout(rows, prm)
    afgpu.istft_check_rows(rows, tiles, prm, a, table, b)
    seen = set()

    def refused(change=None, status=INVALID, **kw):
        bad = rows.copy()
        if change:
            change(bad)
        p = kw.get("prm", prm)
        rc = lib.afg_istft_check_rows(bad.ctypes.data, len(bad), kw.get("tiles", tiles), C.byref(p), kw.get("in_floats", a), kw.get("table_floats", table),
                                      kw.get("out_floats", b))
        msg = lib.afg_last_error().decode()
        assert rc == status and msg, (rc, msg)
        assert msg not in seen, msg
        seen.add(msg)

    refused(prm=afgpu.IstftParams(14 * 3 * 5, 16, 16, 1), status=unsupported)
    refused(prm=afgpu.IstftParams(2049, 16, 16, 1), status=unsupported)
    refused(prm=afgpu.IstftParams(400, 0, 160, 1))
    refused(prm=afgpu.IstftParams(400, 401, 160, 1))
    refused(prm=afgpu.IstftParams(400, 400, 0, 1))
    refused(prm=afgpu.IstftParams(400, 400, 401, 1))
    refused(prm=afgpu.IstftParams(400, 400, 160, 2))
    refused(prm=afgpu.IstftParams(400, 400, 160, 1, (0, 0, 0, 1)))
    refused(table_floats=table - 1)
    refused(lambda r: r["first_tile"].__setitem__(1, 0))
    refused(tiles=tiles + 1)
    refused(in_floats=a - 1)                                     # the last slab's last float
    refused(lambda r: r["in_off"].__setitem__(0, 1 << 63))
    refused(out_floats=b - 1)
    refused(lambda r: r["out_off"].__setitem__(1, (1 << 64) - 8))
    refused(lambda r: r["n_frames"].__setitem__(0, 0))
    refused(lambda r: r["in_pitch"].__setitem__(1, 4))
    refused(lambda r: r["out_frames"].__setitem__(0, 1801))      # one past the line: 11 frames make 2000 samples, 200 of them the pad
    assert len(seen) == 18
    # a slab that ends exactly at in_floats and a row that ends exactly at L pass
    ok, a2, b2 = records(prm, [(11, 0, 1800)])
    afgpu.istft_check_rows(ok, afgpu.istft_layout(ok, prm), prm, a2, table, b2)
    ok["out_frames"][0] = 1801
    with pytest.raises(afgpu.AfgError, match="line"):
        afgpu.istft_check_rows(ok, afgpu.istft_layout(ok, prm), prm, a2, table, b2 + 1)
    assert lib.afg_istft_check_rows(None, 0, 0, C.byref(prm), 0, 0, 0) == 0
    assert lib.afg_istft_check_rows(None, 3, 0, C.byref(prm), 0, 0, 0) == INVALID
    assert lib.afg_istft_tile_samples(None) == 0 and lib.afg_istft_layout(None, 0, None) == 0
    assert lib.afg_istft_envelope_min(None, 1, 0, 1) < 0 and lib.afg_last_error()
    assert lib.afg_istft_envelope_min(C.byref(prm), 0, 0, 1) < 0 and lib.afg_istft_envelope_min(C.byref(prm), 3, 0, 0) < 0
    assert lib.afg_istft_envelope_min(C.byref(prm), 3, 0, 2 * 160 + 400 - 200 + 1) < 0
    # the kernel entry stops at the parameters and the arguments before it touches a device
    assert lib.afg_istft_hip(1, 0x1000, 1, C.byref(afgpu.IstftParams(400, 400, 160, 3)), 0x2000, 8, 0x3000, table, 0x4000, 8, None) == INVALID
    assert lib.afg_istft_hip(1, None, 1, C.byref(prm), 0x2000, 8, 0x3000, table, 0x4000, 8, None) == INVALID
    assert lib.afg_istft_hip(0, None, 0, C.byref(prm), None, 0, None, 0, None, 0, None) == 0


def test_the_envelope_refuses_what_torch_refuses():
    table = lambda p: p.win_length + 2 * p.n_fft

    def check(prm, frames, first, count):
        rows, a, b = records(prm, [(frames, first, count)])
        afgpu.istft_check_rows(rows, afgpu.istft_layout(rows, prm), prm, a, table(prm), b)

    # without centring the line starts on the window's zero
    prm = afgpu.istft_params(400, 160, 400, False)
    with pytest.raises(afgpu.AfgError, match="envelope"):
        check(prm, 10, 0, 500)
    check(prm, 10, 1, 500)
    prm = afgpu.istft_params(400, 100, 300, False)               # n_lo = 50
    with pytest.raises(afgpu.AfgError, match="envelope"):
        check(prm, 10, 50, 500)
    check(prm, 10, 51, 500)
    assert afgpu.istft_envelope_min(prm, 10, 50, 500) == 0.0 and afgpu.istft_envelope_min(prm, 10, 51, 500) > 1e-11
    # a hop above the window leaves samples under no window
    prm = afgpu.istft_params(400, 320, 300, True)
    with pytest.raises(afgpu.AfgError, match="envelope"):
        check(prm, 10, 0, 1000)
    check(prm, 10, 0, 100)                                       # (inside the first frame's window it is fine)
    # centred, the default range is fine down to hop = win_length / 2
    for shape in ((30, 15, 30), (16, 1, 16), (2048, 2048, 2048)):
        prm = afgpu.istft_params(*shape, True)
        if shape[1] == shape[2]:                                 # hop = win_length: Hann's zero comes round every hop
            with pytest.raises(afgpu.AfgError, match="envelope"):
                check(prm, 4, 0, 3 * shape[1])
        else:
            check(prm, 40, 0, 39 * shape[1])
            assert afgpu.istft_envelope_min(prm, 40, 0, 39 * shape[1]) >= 0.4999
