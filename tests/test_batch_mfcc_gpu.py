"""afgpu.batch_decode_mfcc (afg_batch_decode_mfcc) on the small generated corpus of tests/test_batch_mel_gpu.py -- one short file
of every format, files at 8 and 44.1 kHz, a damaged file and one that is no audio: the result is, bit for bit,
tests/cepstra_model.py applied to afgpu.batch_decode_mel_normalized of the same list with the library's table, for both mel
algorithms and whatever the sublists; with cmvn, tests/normalize_model.py applied to every row of that."""
import math

import numpy as np
import pytest
import torch

import afgpu
import cepstra_model as cm
import f64_model as fm
import melspec_model as mm
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T, N_MELS, N_OUT = 16000, 4000, 80, 26
N_MFCC, ORDER, WIN = 13, 2, 2
IN_CHANNELS = 3                                                  # two of the generated files have three channels


def logmel_of(files, **kw):
    kw.setdefault("in_channels", IN_CHANNELS)
    got, meta = afgpu.batch_decode_mel_normalized(files, T, RATE, n_threads=4, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


def model_of(logmel, D, order=ORDER, N=WIN):
    """[files, channels, n_mels, n_out] -> [files, channels, (1 + order) * n_ceps, n_out]"""
    return np.stack([np.stack([cm.cepstra32(D, s, order, N) for s in f]) for f in logmel])


def cmvn_of(feats, mode="standard", **kw):
    prm = nm.params(getattr(nm, mode.upper()), **kw)
    rows = feats.reshape(-1, feats.shape[-1])
    return np.stack([nm.apply(r, nm.group_stats(r.reshape(1, -1), prm), prm) for r in rows]).reshape(feats.shape)


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()                                        # one file per format
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 3001), (44100, 2, 9000)):
        files.append(wb.wav_file(fm.KIND_S16, ch, rate, wb.random_samples(rng, fm.KIND_S16, ch * frames)))
    files.append(files[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    at = {"r8000": base, "r44100": base + 1, "damaged": base + 2, "junk": base + 3}
    D = afgpu.cep_dct(N_MFCC, N_MELS, "ortho")
    ref = {}
    with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for algorithm in ("direct", "fft"):                      # made once, never changed
            logmel, meta = logmel_of(files, algorithm=algorithm)
            want = model_of(logmel, D)
            want.setflags(write=False)
            ref[algorithm] = {"logmel": logmel, "meta": meta, "want": want}
    assert ref["direct"]["logmel"].shape == (len(files), 1, N_MELS, N_OUT)
    assert [i for i, m in enumerate(ref["direct"]["meta"]) if m["status"] != 0] == [at["damaged"], at["junk"]]
    assert mm.same_bits(ref["direct"]["logmel"], ref["fft"]["logmel"]).size > 0       # two algorithms: two references
    return {"files": files, "at": at, "D": D, "ref": ref}


def decode(files, shape=None, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    shape = shape or (len(files), 1, (1 + kw.get("delta_order", ORDER)) * kw.get("n_mfcc", N_MFCC), N_OUT)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    kw.setdefault("in_channels", IN_CHANNELS)
    kw.setdefault("delta_order", ORDER)
    kw.setdefault("delta_win", WIN)
    got, meta = afgpu.batch_decode_mfcc(files, T, out=out, n_threads=4, **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("algorithm", ["direct", "fft"])
def test_the_cepstra_are_the_models_of_the_log_mel_tensor(corpus, algorithm):
    ref = corpus["ref"][algorithm]
    got, meta = decode(corpus["files"], algorithm=algorithm)
    same(got, ref["want"])
    assert meta == ref["meta"]
    assert not np.isnan(got).any() and np.abs(got[:, :, N_MFCC:]).max() > 0.01       # deltas that say something
    # a failed file keeps its status and message; its slab is the all-floor slab's: c0 of 80 floors, the other statics what
    # the table's rows sum to, every delta nothing
    floor = np.full((N_MELS, N_OUT), ref["logmel"][corpus["at"]["junk"], 0, 0, 0], np.float32)
    assert abs(float(floor[0, 0]) + 10.0) < 1e-5
    for bad in (corpus["at"]["damaged"], corpus["at"]["junk"]):
        assert meta[bad]["status"] != 0 and meta[bad]["message"]
        same(got[bad, 0], cm.cepstra32(corpus["D"], floor, ORDER, WIN))
        assert abs(float(got[bad, 0, 0, 0]) + 10.0 * math.sqrt(N_MELS)) < 1e-3 and (got[bad, 0, N_MFCC:] == 0).all()


def test_cmvn_is_the_normalisation_model_row_by_row(corpus):
    ref = corpus["ref"]["direct"]
    got, meta = decode(corpus["files"], cmvn="standard")
    want = cmvn_of(ref["want"])
    bad = nm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    assert meta == ref["meta"]
    live = got[corpus["at"]["r8000"], 0]                         # zero mean and unit variance per coefficient over time
    assert np.abs(live.mean(axis=1)).max() < 1e-4 and np.abs(live.std(axis=1) - 1.0).max() < 1e-3
    peak, _ = decode(corpus["files"][:3], cmvn=afgpu.norm_params("peak", target=0.5))           # the other modes work too
    assert nm.same_bits(peak, cmvn_of(ref["want"][:3], "peak", target=0.5)).size == 0
    assert np.abs(np.abs(peak[0]).max(axis=-1) - 0.5).max() < 1e-6


def test_wave_norm_and_cmvn_together(corpus):
    files = corpus["files"][:4]
    logmel, meta0 = logmel_of(files, wave_norm="standard")
    got, meta = decode(files, wave_norm="standard", cmvn="standard")
    want = cmvn_of(model_of(logmel, corpus["D"]))
    assert nm.same_bits(got, want).size == 0 and meta == meta0
    assert mm.same_bits(logmel, corpus["ref"]["direct"]["logmel"][:4]).size > 0            # the gain shows in the features


def test_the_result_does_not_depend_on_the_sublists(corpus):
    files, ref = corpus["files"], corpus["ref"]["direct"]
    L = afgpu.lib()
    want = cmvn_of(ref["want"])
    try:
        for value in (1, 3 * N_MELS * N_OUT * 4 + 8):           # every file its own sublist; three files
            assert L.afg_dev_option(b"mel_scratch_bytes", value) == 0
            got, meta = decode(files)
            same(got, ref["want"])
            assert meta == ref["meta"]
            got, meta = decode(files, cmvn="standard")
            assert nm.same_bits(got, want).size == 0 and meta == ref["meta"]
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0


def test_n_out_crops_the_frames(corpus):
    files = corpus["files"][:4]
    logmel, _ = logmel_of(files, n_out=25)                       # 25 of 26, as Whisper takes 3000 of 3001
    got, meta = decode(files, shape=(4, 1, 39, 25), n_out=25)
    same(got, model_of(logmel, corpus["D"]))                     # (the deltas replicate frame 24: not a crop of the uncropped result)
    assert mm.same_bits(got[:, :, :N_MFCC], corpus["ref"]["direct"]["want"][:4, :, :N_MFCC, :25]).size == 0


def test_two_channels_other_tables_and_first_frame(corpus):
    at = corpus["at"]
    files = corpus["files"][:3] + [corpus["files"][at["r44100"]], corpus["files"][at["junk"]]]
    first = [0, 100, 7, 2000, 0]
    kw = dict(mono=False, channels=2, first_frame=first, n_mels=40, in_channels=IN_CHANNELS)
    logmel, meta0 = logmel_of(files, **kw)
    assert logmel.shape == (5, 2, 40, N_OUT)
    D = afgpu.cep_dct(40, 40, "none", 22.0, math.log(10.0))      # every coefficient, liftered, natural-log cepstra, N = 8
    got, meta = decode(files, shape=(5, 2, 80, N_OUT), n_mfcc=40, delta_order=1, delta_win=8, dct_norm="none", lifter=22,
                       log_scale=math.log(10.0), **kw)
    same(got, model_of(logmel, D, 1, 8))
    assert meta == meta0 and meta[4]["status"] != 0
    unshifted, _ = logmel_of(files, **dict(kw, first_frame=None))
    assert mm.same_bits(logmel[1], unshifted[1]).size > 0       # first_frame shows
    statics, _ = decode(files, shape=(5, 2, 40, N_OUT), n_mfcc=40, delta_order=0, dct_norm="none", lifter=22, log_scale=math.log(10.0), **kw)
    same(statics, got[:, :, :40])


def test_an_empty_list_and_a_wrong_out(corpus):
    empty, meta = afgpu.batch_decode_mfcc([], T, delta_order=2)
    assert tuple(empty.shape) == (0, 1, 39, N_OUT) and empty.is_cuda and meta == []
    for out in (torch.empty((2, 1, 39, N_OUT), dtype=torch.float64, device="cuda"), torch.empty((2, 1, 13, N_OUT), device="cuda"),
                torch.empty((2, 1, 39, N_OUT))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mfcc(corpus["files"][:2], T, delta_order=2, out=out)
