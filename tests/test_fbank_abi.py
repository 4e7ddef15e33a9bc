"""The host half of the Kaldi-compatible filter-bank stage (include/afg.h: afg_fbank_*): the helpers' return values, every
refusal with its message, the record checks on hostile records, struct_size handling of the batch options.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import afgpu

INVALID = -1


def status_of(word):
    """the status code whose afg_status_string is `word`"""
    lib = afgpu.lib()
    return next(rc for rc in range(-1, -16, -1) if lib.afg_status_string(rc).decode() == word)


def good_params(**kw):
    p = afgpu.fbank_params(400, 160, 512, 23)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [(dict(win_length=1), "win_length"), (dict(win_length=2049, n_fft=2048), "win_length"), (dict(hop=0), "hop"), (dict(hop=65536), "hop"),
              (dict(n_fft=399), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(n_mels=0), "n_mels"), (dict(n_mels=257), "n_mels"),
              (dict(snip_edges=2), "snip_edges"), (dict(remove_dc=2), "remove_dc"), (dict(use_power=2), "use_power"), (dict(use_log=7), "use_log"),
              (dict(use_energy=2), "use_energy"), (dict(raw_energy=2), "raw_energy"), (dict(htk_compat=2), "htk_compat"), (dict(layout=2), "layout"),
              (dict(preemph=-0.1), "preemph"), (dict(preemph=1.5), "preemph"), (dict(preemph=float("nan")), "preemph"),
              (dict(energy_floor=-1.0), "energy_floor"), (dict(energy_floor=float("inf")), "energy_floor"), (dict(scale=-1.0), "scale"),
              (dict(scale=float("nan")), "scale"), (dict(reserved=1), "reserved")]


def test_helpers():
    lib = afgpu.lib()
    assert [afgpu.fbank_n_fft(w) for w in (2, 3, 400, 512, 513, 1102, 2048)] == [2, 4, 512, 512, 1024, 2048, 2048]
    assert [afgpu.fbank_n_fft(w, False) for w in (2, 400, 1102)] == [2, 400, 1102]
    for w in (0, 1, 2049):
        assert lib.afg_fbank_n_fft(w, 1) == 0 and "win_length" in lib.afg_last_error().decode()
    p = good_params()
    assert [afgpu.fbank_frames(p, n) for n in (0, 399, 400, 559, 560, 16000)] == [0, 0, 1, 1, 2, 98]
    q = good_params(snip_edges=0)
    assert [afgpu.fbank_frames(q, n) for n in (0, 1, 79, 80, 240, 16000, 2 ** 32 - 1)] == [0, 0, 0, 1, 2, 100, (2 ** 32 - 1 + 80) // 160]
    assert afgpu.fbank_frames(good_params(hop=0), 16000) == 0 and "hop" in lib.afg_last_error().decode()
    assert lib.afg_fbank_frames(None, 16000) == 0
    assert lib.afg_fbank_tables(0, 400, 512, 0.42, None, 0) == 400 + 1024
    few = np.full(8, 7.0, np.float32)
    assert lib.afg_fbank_tables(0, 400, 512, 0.42, few.ctypes.data, 8) == 1424 and (few == 7.0).all()      # too small a buffer is left alone
    assert lib.afg_fbank_filters(16000, 512, 23, 20.0, 0.0, None, 0) == 23 * 257
    assert lib.afg_fbank_filters(16000, 512, 23, 20.0, 0.0, few.ctypes.data, 8) == 23 * 257 and (few == 7.0).all()
    rows = np.zeros(4, afgpu.MEL_ROW_DTYPE)
    rows["out_frames"] = [0, 16, 17, 1]
    assert afgpu.fbank_layout(rows, p) == 4 and list(rows["first_tile"]) == [0, 0, 1, 3]
    assert afgpu.fbank_layout(rows, good_params(n_mels=0)) == 0
    assert C.sizeof(afgpu.FbankParams) == 64 and C.sizeof(afgpu.FbankOpts) == 152 and afgpu.FbankOpts.fbank.offset == 48
    assert afgpu.FbankOpts.low_freq.offset == 120 and afgpu.FbankOpts.reserved.offset == 144


def test_tables_and_bank_refusals():
    lib = afgpu.lib()
    for args, word in (((5, 400, 512, 0.42), "window_type"), ((0, 1, 512, 0.42), "win_length"), ((0, 2049, 2048, 0.42), "win_length"),
                       ((0, 400, 399, 0.42), "n_fft"), ((0, 400, 4096, 0.42), "n_fft"), ((3, 400, 512, float("nan")), "blackman_coeff"),
                       ((0, 1102, 1102, 0.42), "prime factors"), ((0, 8, 8, 0.42), "prime factors")):
        assert lib.afg_fbank_tables(*args, None, 0) == 0 and word in lib.afg_last_error().decode(), args
        with pytest.raises(afgpu.AfgError, match=word):
            afgpu.fbank_tables(*args)
    with pytest.raises(ValueError, match="window_type"):
        afgpu.fbank_tables("kaiser", 400, 512)
    for args, word in (((0, 512, 23, 20.0, 0.0), "sample rate"), ((16000, 1, 23, 20.0, 0.0), "n_fft"), ((16000, 4096, 23, 20.0, 0.0), "n_fft"),
                       ((16000, 512, 0, 20.0, 0.0), "n_mels"), ((16000, 512, 257, 20.0, 0.0), "n_mels"), ((16000, 512, 23, -1.0, 0.0), "low_freq"),
                       ((16000, 512, 23, 20.0, 8000.5), "low_freq"), ((16000, 512, 23, 4000.0, 4000.0), "low_freq"),
                       ((16000, 512, 23, 20.0, -7990.0), "low_freq"), ((16000, 512, 23, float("nan"), 0.0), "low_freq")):
        assert lib.afg_fbank_filters(*args, None, 0) == 0 and word in lib.afg_last_error().decode(), args
        with pytest.raises(afgpu.AfgError, match=word):
            afgpu.fbank_filters(*args)
    assert afgpu.fbank_filters(16000, 512, 23, 20.0, 8000.0).shape == (23, 257)        # Nyquist itself is allowed


def records(p, lengths, frames=None):
    cols = p.n_mels + p.use_energy
    rows = np.zeros(len(lengths), afgpu.MEL_ROW_DTYPE)
    at_in = at_out = 0
    for k, n in enumerate(lengths):
        f = afgpu.fbank_frames(p, n) if frames is None else frames[k]
        rows[k]["in_off"], rows[k]["out_off"], rows[k]["in_frames"], rows[k]["out_frames"] = at_in, at_out, n, f
        at_in += n
        at_out += cols * f
    return rows, afgpu.fbank_layout(rows, p), at_in, at_out


@pytest.mark.parametrize("snip_edges", [1, 0])
def test_check_rows(snip_edges):
    lib = afgpu.lib()
    unsupported = status_of("unsupported")
    p = good_params(snip_edges=snip_edges, use_energy=1)
    table, bank = 400 + 1024, 23 * 257
    rows, tiles, nin, nout = records(p, [3000, 0, 700, 399, 16000])
    afgpu.fbank_check_rows(rows, tiles, p, nin, table, bank, nout)
    seen = set()

    def refused(change=None, want=INVALID, word=None, prm=None, **kw):
        bad = rows.copy()
        if change:
            change(bad)
        rc = lib.afg_fbank_check_rows(bad.ctypes.data, len(bad), kw.get("tiles", tiles), C.byref(p if prm is None else prm), kw.get("nin", nin),
                                      kw.get("table", table), kw.get("bank", bank), kw.get("nout", nout))
        msg = lib.afg_last_error().decode()
        assert rc == want and msg.startswith(("afg_fbank_check_rows:", "afg_fbank_hip:")) and (word is None or word in msg), (rc, msg)
        seen.add(msg)

    for kw, word in BAD_PARAMS:
        refused(prm=good_params(**kw), word=word)
    refused(prm=good_params(win_length=1102, hop=441, n_fft=1102), want=unsupported, word="prime factors")    # 44.1 kHz, 25 ms, no rounding
    refused(prm=good_params(win_length=8, n_fft=8), want=unsupported, word="prime factors")
    assert lib.afg_fbank_check_rows(None, 0, 0, C.byref(good_params(win_length=1102, n_fft=2048)), 0, 0, 0, 0) == 0   # ... rounded up it runs
    refused(lambda b: b["out_frames"].__setitem__(2, afgpu.fbank_frames(p, 700) + 1), word="out_frames")
    refused(lambda b: b["out_frames"].__setitem__(1, 1), word="out_frames")          # no samples, no frames, whatever the edge mode
    refused(nin=nin - 1, word="leaves the input")
    refused(nout=nout - 1, word="leave the output")
    refused(lambda b: b["in_off"].__setitem__(0, 1 << 63))
    refused(lambda b: b["out_off"].__setitem__(4, (1 << 64) - 8))
    refused(table=table - 1, word="table_floats")
    refused(bank=bank - 1, word="filters_floats")
    refused(tiles=tiles + 1, word="n_tiles")
    refused(lambda b: b["first_tile"].__setitem__(2, 0), word="first_tile")
    assert len(seen) >= len(BAD_PARAMS) + 10
    assert lib.afg_fbank_check_rows(None, 1, 0, C.byref(p), 0, table, bank, 0) == INVALID and "NULL rows" in lib.afg_last_error().decode()
    rows2, tiles2, nin2, nout2 = records(p, [480000], [2000])                       # fewer frames than the row has is fine
    afgpu.fbank_check_rows(rows2, tiles2, p, nin2, table, bank, nout2)


def test_kernel_entry_checks_what_it_can_without_a_device():
    lib = afgpu.lib()
    p = good_params()
    assert lib.afg_fbank_hip(0, None, 0, C.byref(p), None, 0, None, 0, None, 0, None, 0, None) == 0
    assert lib.afg_fbank_hip(0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None) == INVALID
    for kw, word in BAD_PARAMS:
        assert lib.afg_fbank_hip(1, 0x1000, 1, C.byref(good_params(**kw)), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None) == INVALID
        assert lib.afg_last_error().decode().startswith(f"afg_fbank_hip: {word}")
    for args in ((1, None, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, None, 8, 0x4000, 8, 0x5000, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, None, 8, 0x5000, 8, None), (1, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, None, 8, None),
                 (1, 0x1000, 1, C.byref(p), 0x2002, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None), (1 << 32, 0x1000, 1, C.byref(p), 0x2000, 8, 0x3000, 8, 0x4000, 8, 0x5000, 8, None)):
        assert lib.afg_fbank_hip(*args) == INVALID and lib.afg_last_error().decode().startswith("afg_fbank_hip:")


def call(n_files, opts, d_out=0x1000):
    """the batch entry with a made-up device address: an argument error comes back before anything touches it"""
    lib = afgpu.lib()
    ptrs = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    res = afgpu.BatchResult()
    counts = np.full(1, 77, np.uint32)
    rc = lib.afg_batch_decode_fbank(ptrs, lens, n_files, C.byref(opts) if opts is not None else None, d_out, counts.ctypes.data, C.byref(res))
    assert counts[0] == 77
    return rc, lib.afg_last_error().decode(), res


def good_opts(fbank=None, **kw):
    o = afgpu.FbankOpts(C.sizeof(afgpu.FbankOpts), 1, 1, 16000, None, 16000, 1, 0, 0, 0, 0, good_params(**(fbank or {})), 0, 20.0, 0.0, 0.42, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_batch_entry_refuses_before_any_device_call():
    unsupported = status_of("unsupported")
    cases = {
        "no opts": (call(1, None), INVALID, "NULL opts"),
        "no d_out": (call(1, good_opts(), d_out=None), INVALID, "NULL d_out"),
        "short struct": (call(1, good_opts(struct_size=C.sizeof(afgpu.FbankOpts) - 8)), INVALID, "struct_size"),
        "resample's struct": (call(1, good_opts(struct_size=C.sizeof(afgpu.ResampleOpts))), INVALID, "struct_size"),
        "reserved": (call(1, good_opts(reserved=1)), INVALID, "reserved"),
        "channels": (call(1, good_opts(channels=0)), INVALID, "channels"),
        "bad hop": (call(1, good_opts(fbank=dict(hop=0))), INVALID, "hop"),
        "params' reserved": (call(1, good_opts(fbank=dict(reserved=3))), INVALID, "reserved"),
        "n_fft below the window": (call(1, good_opts(fbank=dict(n_fft=256))), INVALID, "n_fft"),
        "1102": (call(1, good_opts(fbank=dict(win_length=1102, hop=441, n_fft=1102), samplerate=44100)), unsupported, "n_fft 1102"),
        "window": (call(1, good_opts(window_type=9)), INVALID, "window_type"),
        "blackman": (call(1, good_opts(window_type=3, blackman_coeff=float("inf"))), INVALID, "blackman_coeff"),
        "low above high": (call(1, good_opts(low_freq=5000.0, high_freq=4000.0)), INVALID, "low_freq"),
        "high above nyquist": (call(1, good_opts(high_freq=8001.0)), INVALID, "low_freq"),
        "no frame": (call(1, good_opts(frames=399)), INVALID, "no frame"),
        "n_out": (call(1, good_opts(n_out=99)), INVALID, "n_out"),
    }
    for what, ((rc, msg, res), want, word) in cases.items():
        assert rc == want and word in msg, (what, rc, msg)
        assert res.n_files == 0 and not res.items
    for o in (good_opts(), good_opts(n_out=98), good_opts(struct_size=C.sizeof(afgpu.FbankOpts) + 64), good_opts(fbank=dict(snip_edges=0), frames=80)):
        rc, _, res = call(0, o)                                  # no file at all touches nothing
        assert rc == 0 and res.n_files == 0 and not res.items


def test_python_entries_check_their_arguments():
    with pytest.raises(ValueError, match="window_type"):
        afgpu.batch_decode_fbank([b"x"], 16000, window_type="kaiser")
    with pytest.raises(ValueError, match="no frame"):
        afgpu.batch_decode_fbank([b"x"], 399)
    with pytest.raises(ValueError, match="n_out"):
        afgpu.batch_decode_fbank([b"x"], 16000, n_out=99)
    with pytest.raises(afgpu.AfgError, match="n_mels"):
        afgpu.batch_decode_fbank([b"x"], 16000, num_mel_bins=300)
    with pytest.raises(afgpu.AfgError, match="unsupported"):
        afgpu.batch_decode_fbank([b"x"], 44100, samplerate=44100, round_to_power_of_two=False)      # 1102 = 2 * 19 * 29
