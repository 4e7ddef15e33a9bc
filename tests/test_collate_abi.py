"""afg_collate_hip / afg_batch_decode_to_device without a GPU: the symbols, the record layouts, the argument checks that
come before any device call, and the numpy model the GPU tests compare with (tests/collate_model.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import afgpu
import collate_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afg_collate_layout", "afg_collate_hip", "afg_batch_decode_to_device")
INVALID = -1


def header():
    return open(os.path.join(ROOT, "include", "afg.h")).read()


def test_symbols_are_exported_and_declared():
    lib = afgpu.lib()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "audio-formats_amd", "lib", "libafg_hip.so")], text=True)
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    d = open(os.path.join(ROOT, "bindings", "d", "afgpu.d")).read()
    d = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", d, flags=re.S))
    for name in NEW:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", exported), name
        assert re.search(rf"\b{name}\s*\(", code), name
        assert re.search(rf"\b{name}\s*\(", d), name
        assert name in afgpu.ABI_SYMBOLS
    assert "stream.d:429-637" in header().split("afg_batch_decode_to_device")[0].rsplit("typedef struct afg_collate_opts", 1)[0][-3000:]
    assert lib.afg_status_string(INVALID) == b"invalid argument"


def c_layout(struct, fields):
    """sizeof and the offsets of `fields` of a struct of afg.h, from a C compiler"""
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"afg.h\"\nint main(void){printf(\"%zu\", sizeof(" + struct + "));" + \
          "".join(f"printf(\" %zu\", offsetof({struct}, {f}));" for f in fields) + "return 0;}"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.c"), "w").write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")])
        out = subprocess.check_output([os.path.join(tmp, "t")], text=True).split()
    return int(out[0]), [int(v) for v in out[1:]]


def test_record_layouts_match_the_header():
    names = list(afgpu.COLLATE_SPAN_DTYPE.names)
    size, offs = c_layout("afg_collate_span", names)
    assert size == afgpu.COLLATE_SPAN_DTYPE.itemsize == 56
    assert offs == [afgpu.COLLATE_SPAN_DTYPE.fields[n][1] for n in names]
    assert afgpu.COLLATE_SPAN_DTYPE["first_frame"] == np.int64 and afgpu.COLLATE_SPAN_DTYPE["channels"] == np.uint16
    names = [f[0] for f in afgpu.CollateOpts._fields_]
    size, offs = c_layout("afg_collate_opts", names)
    assert size == C.sizeof(afgpu.CollateOpts)
    assert offs == [getattr(afgpu.CollateOpts, n).offset for n in names]
    assert afgpu.WAV_TILE_SAMPLES == 4096


def test_layout_gives_every_span_its_tiles():
    sp = np.zeros(5, afgpu.COLLATE_SPAN_DTYPE)
    sp["count"] = [1, 0, 4096, 4097, 3 * 4096]
    assert afgpu.collate_layout(sp) == 1 + 0 + 1 + 2 + 3
    assert list(sp["first_tile"]) == [0, 1, 1, 2, 4]


def call(n_files, opts, d_out=0x1000, out=True, files=(b"x",)):
    """afg_batch_decode_to_device with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    bufs = [bytes(f) for f in files]
    ptrs = (C.c_char_p * max(len(bufs), 1))(*bufs)
    lens = (C.c_size_t * max(len(bufs), 1))(*[len(b) for b in bufs])
    res = afgpu.BatchResult()
    rc = lib.afg_batch_decode_to_device(ptrs, lens, n_files, None if opts is None else C.byref(opts), d_out, C.byref(res) if out else None)
    return rc, lib.afg_last_error().decode(), res


def good_opts(**kw):
    o = afgpu.CollateOpts(C.sizeof(afgpu.CollateOpts), 1, 2, 16, None)
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
        "short struct": call(1, good_opts(struct_size=afgpu.CollateOpts.first_frame.offset)),
        "no channels": call(1, good_opts(channels=0)),
        "no frames": call(1, good_opts(frames=0)),
        "negative first_frame": call(1, good_opts(first_frame=neg)),
        "negative n_files": call(-1, good_opts()),
    }
    seen = set()
    for what, (rc, msg, res) in cases.items():
        assert rc == INVALID, (what, rc)
        assert msg and msg not in seen, (what, msg)
        seen.add(msg)
        assert res.n_files == 0 and not res.items
    # no file at all: ok, and nothing is touched (the address is made up)
    rc, _, res = call(0, good_opts())
    assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entry_checks_its_arguments():
    import pytest
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor([b"x"], 0, 2)
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor([b"x"], 16, 0)


def test_model_on_a_hand_written_stereo_example():
    """frames 0..4 of a stereo file as L0 R0 L1 R1 ...; the run starts at R1 (sample 3) and ends with L4 (sample 8)"""
    L, R = [10, 11, 12, 13, 14], [20, 21, 22, 23, 24]
    inter = np.array([v for lr in zip(L, R) for v in lr], np.float32)
    d_in = np.concatenate([np.float32([99]), inter[3:9]])                       # the run lies at float 1 of the plane
    out = np.full(2 + 2 * 4, 77, np.float32)
    sp = cm.span(in_off=1, count=6, sample0=3, out_off=2, first_frame=1, frames=4, channels=2, out_channels=2)
    got = cm.apply_spans([sp], d_in, out).view(np.float32)
    #            foreign   row 0: t = 0..3 is frames 1..4: L1 not in the run     row 1: R1 R2 R3, R4 not in the run
    assert list(got) == [77, 77, 77, 12, 13, 14, 21, 22, 23, 77]
    # one output channel: row 1 is dropped; a row longer than the file is left as it was; first_frame past the end: nothing
    got = cm.apply_spans([dict(sp, out_channels=1, frames=8)], d_in, np.full(12, 77, np.float32)).view(np.float32)
    assert list(got) == [77, 77, 77, 12, 13, 14] + [77] * 6
    assert (cm.apply_spans([dict(sp, first_frame=5)], d_in, out).view(np.float32) == 77).all()
    # zero run
    got = cm.apply_spans([cm.zero_run(3, 4)], d_in, out).view(np.float32)
    assert list(got) == [77] * 3 + [0] * 4 + [77] * 3
    # a slab: 3 output channels of a stereo file from frame 3 on, 4 frames long
    s = cm.slab(inter, 2, 3, 4, first_frame=3)
    assert s.tolist() == [[13, 14, 0, 0], [23, 24, 0, 0], [0, 0, 0, 0]]
    assert (cm.slab(None, 0, 2, 3) == 0).all() and (cm.slab(inter, 2, 1, 2, first_frame=9) == 0).all()


def test_model_one_span_equals_the_same_run_cut_anywhere():
    rng = np.random.default_rng(5)
    for ch in (1, 2, 3, 6, 8):
        n = 997
        d_in = rng.integers(0, 1 << 32, 64 + n, dtype=np.uint64).astype(np.uint32)
        for _ in range(8):
            T, C = int(rng.integers(1, 300)), int(rng.integers(1, 10))
            base = rng.integers(0, 1 << 32, 5 + C * T, dtype=np.uint64).astype(np.uint32)
            whole = cm.span(in_off=17, count=n, sample0=int(rng.integers(0, 50)), out_off=5, first_frame=int(rng.integers(0, 40)),
                            frames=T, channels=ch, out_channels=C)
            cut = int(rng.integers(1, n))
            a = dict(whole, count=cut)
            b = dict(whole, in_off=17 + cut, count=n - cut, sample0=whole["sample0"] + cut)
            one = cm.apply_spans([whole], d_in, base)
            assert (one == cm.apply_spans([a, b], d_in, base)).all() and (one == cm.apply_spans([b, a], d_in, base)).all()
            assert (one != base).any() or whole["first_frame"] * ch >= whole["sample0"] + n
