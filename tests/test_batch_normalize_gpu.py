"""afgpu.batch_decode_tensor_normalized (afg_batch_decode_resampled_norm) and afgpu.batch_decode_mel_normalized
(afg_batch_decode_mel_norm) on the corpus of tests/test_batch_mel_gpu.py -- one short generated file of every format, files
at 8 and 44.1 kHz, a damaged file and one that is no audio, to 16 kHz: the library's own tensor (or its own log-mel) put
through tests/normalize_model.py, bit for bit, whatever the sublists."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as fm
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T, N_FFT, HOP, N_MELS = 16000, 4000, 400, 160, 80
N_OUT = 26
IN_CHANNELS = 3                                                  # two of the generated files have three channels
MODES = {"peak": dict(target=0.9), "rms": dict(target=0.1), "standard": {}, "dynamic_range": dict(range=0.5, shift=0.25, gain=2.0)}


def groups_of(meta, C, mono):
    """one group per file, as include/afg.h describes them, with valid computed here from what the call reported"""
    g = np.zeros(len(meta), nm.GROUP_DTYPE)
    for i, m in enumerate(meta):
        g[i]["in_off"] = g[i]["out_off"] = i * C * T
        g[i]["stride"], g[i]["rows"] = T, 1
        if m["status"] == 0:
            g[i]["rows"] = 1 if mono else min(C, m["channels"])
            g[i]["valid"] = nm.valid_length(m["frames"], 0, round(m["samplerate"]), RATE, T)
    return g


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
    ref = {}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for C, mono in ((1, True), (2, False)):
            tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, C, RATE, mono=mono, in_channels=IN_CHANNELS, n_threads=4)
            torch.cuda.synchronize()
            plane = tensor.cpu().numpy().reshape(-1)
            plane.setflags(write=False)
            ref[mono] = {"plane": plane, "meta": meta, "groups": groups_of(meta, C, mono), "C": C}
        logmel, mel_meta = afgpu.batch_decode_mel(files, T, RATE, in_channels=IN_CHANNELS, n_threads=4)
        torch.cuda.synchronize()
    meta = ref[True]["meta"]
    assert mel_meta == meta and tuple(logmel.shape) == (len(files), 1, N_MELS, N_OUT)
    assert [i for i, m in enumerate(meta) if m["status"] != 0] == [at["damaged"], at["junk"]]
    assert {8000, 44100} <= {int(m["samplerate"]) for m in meta if m["status"] == 0}
    valid = ref[True]["groups"]["valid"]
    assert valid[at["r8000"]] == T and valid[at["r44100"]] == -(-9000 * 160 // 441) and valid[at["damaged"]] == 0 and 0 < valid.min(initial=T, where=valid > 0) < T
    return {"files": files, "at": at, "ref": ref, "logmel": logmel.cpu().numpy().reshape(len(files), -1), "model": {}}


def tensor_model(corpus, mono, mode):
    key = (mono, mode)
    if key not in corpus["model"]:
        r = corpus["ref"][mono]
        corpus["model"][key] = nm.normalize(r["plane"], r["plane"], r["groups"], nm.params(getattr(nm, mode.upper()), **MODES[mode]))
    return corpus["model"][key]


def decode(corpus, mono, mode, files=None, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    files = corpus["files"] if files is None else files
    C = corpus["ref"][mono]["C"]
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")
    got, meta, stats = afgpu.batch_decode_tensor_normalized(files, T, C, RATE, mode, mono=mono, in_channels=IN_CHANNELS, out=out, n_threads=4,
                                                            return_stats=True, **MODES[mode], **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta, stats


def same(got, want):
    bad = nm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("mono", [True, False], ids=["mono", "two-channels"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_tensor_is_the_resampled_one_through_the_model(corpus, mono, mode):
    got, meta, stats = decode(corpus, mono, mode)
    want, want_stats = tensor_model(corpus, mono, mode)
    r, at = corpus["ref"][mono], corpus["at"]
    same(got.reshape(-1), want)
    assert meta == r["meta"]
    assert nm.same_stats(stats.view(nm.STATS_DTYPE), want_stats) == []
    for bad in (at["damaged"], at["junk"]):                      # a zero slab, a zero record, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad].view(np.uint32) == 0).all()
        assert stats[bad].tobytes() == bytes(40)
    assert stats["count"][at["damaged"] - 1] > 0 and np.abs(got[at["damaged"] - 1]).max() > 0
    ref = r["plane"].reshape(got.shape)
    for i, g in enumerate(r["groups"]):                          # what lies behind a file's samples, and the rows it has no channel for
        rows, valid = int(g["rows"]), int(g["valid"])
        assert (got[i, rows:].view(np.uint32) == 0).all()
        assert (got[i, :, valid:].view(np.uint32) == ref[i, :, valid:].view(np.uint32)).all()
        assert (got[i, :, min(valid + 64, T):].view(np.uint32) == 0).all()            # +0.0f behind the filter's tail
    moved = [i for i, g in enumerate(r["groups"]) if g["valid"] and (got[i].view(np.uint32) != ref[i].view(np.uint32)).any()]
    assert len(moved) >= 10                                      # the mode did something


def whisper_of(logmel):
    """[slabs, n_mels * n_out] through the model: every slab one group of a single row"""
    prm = nm.params(nm.DYNAMIC_RANGE, **nm.WHISPER)
    return np.stack([nm.apply(s, nm.group_stats(s.reshape(1, -1), prm), prm) for s in logmel])


def decode_mel(files, **kw):
    out = torch.full((len(files), 1, N_MELS, N_OUT), float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_mel_normalized(files, T, RATE, in_channels=IN_CHANNELS, out=out, n_threads=4, **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(len(files), -1), meta


def test_whisper_features_are_the_librarys_log_mel_through_the_model(corpus):
    got, meta = decode_mel(corpus["files"], feat_norm="whisper")
    want = corpus.setdefault("whisper", whisper_of(corpus["logmel"]))
    same(got, want)
    assert meta == corpus["ref"][True]["meta"]
    for bad in (corpus["at"]["damaged"], corpus["at"]["junk"]):  # the all-floor slab: (floor + 4) / 4 throughout
        assert (got[bad].view(np.uint32) == got[bad].view(np.uint32)[0]).all() and abs(float(got[bad][0]) - (-10.0 + 4.0) / 4.0) < 1e-6


def test_wave_and_feature_normalisation_together(corpus):
    """the reference: batch_decode_tensor_normalized, afgpu.melspec with the library's tables, then the model"""
    files = corpus["files"]
    got, meta = decode_mel(files, wave_norm="standard", feat_norm="whisper")
    tensor, meta0 = afgpu.batch_decode_tensor_normalized(files, T, 1, RATE, "standard", mono=True, in_channels=IN_CHANNELS, n_threads=4)
    rows = np.zeros(len(files), afgpu.MEL_ROW_DTYPE)
    rows["in_off"], rows["in_frames"] = np.arange(len(files)) * T, T
    rows["out_off"], rows["out_frames"] = np.arange(len(files)) * N_MELS * N_OUT, N_OUT
    prm = afgpu.mel_params(N_FFT, HOP, N_MELS)
    tiles = afgpu.mel_layout(rows, prm)
    basis, bank = afgpu.mel_basis(N_FFT), afgpu.mel_filters(RATE, N_FFT, N_MELS)
    d_mel = torch.full((len(files), N_MELS * N_OUT), float("nan"), dtype=torch.float32, device="cuda")
    afgpu.melspec(len(rows), torch.from_numpy(rows.view(np.uint8).copy()).cuda(), tiles, prm, tensor, tensor.numel(),
                  torch.from_numpy(basis.reshape(-1).copy()).cuda(), basis.size, torch.from_numpy(bank.reshape(-1).copy()).cuda(), bank.size,
                  d_mel, d_mel.numel())
    torch.cuda.synchronize()
    same(got, whisper_of(d_mel.cpu().numpy()))
    assert meta == meta0 == corpus["ref"][True]["meta"]
    only_wave, _ = decode_mel(files, wave_norm="standard")       # either one alone
    same(only_wave, d_mel.cpu().numpy())
    assert nm.same_bits(got, corpus.setdefault("whisper", whisper_of(corpus["logmel"]))).size > 0      # the gain shows in the features


def test_neither_entry_depends_on_the_sublists(corpus):
    files = corpus["files"]
    L = afgpu.lib()
    want, want_stats = tensor_model(corpus, True, "standard")
    whisper = corpus.setdefault("whisper", whisper_of(corpus["logmel"]))
    slab = IN_CHANNELS * (T * 48000 // RATE + 2 * 19 + 1) * 4    # the resampler's scratch: R_s * T_s floats, H = W(48000 -> 16000) = 19
    for option, three in ((b"resample_scratch_bytes", 3 * slab + slab // 2), (b"mel_scratch_bytes", 3 * T * 4 + 8)):
        try:
            for value in (1, three):                             # every file its own sublist; three files
                assert L.afg_dev_option(option, value) == 0
                if option == b"resample_scratch_bytes":
                    got, meta, stats = decode(corpus, True, "standard")
                    same(got.reshape(-1), want)
                    assert nm.same_stats(stats.view(nm.STATS_DTYPE), want_stats) == [] and meta == corpus["ref"][True]["meta"]
                else:
                    got, meta = decode_mel(files, feat_norm="whisper")
                    same(got, whisper)
                    assert meta == corpus["ref"][True]["meta"]
        finally:
            assert L.afg_dev_option(option, -1) == 0


def test_python_refusals_and_empty_lists(corpus):
    part = corpus["files"][:3]
    for out in (torch.empty((3, 1, T), dtype=torch.float64, device="cuda"), torch.empty((3, 1, T + 1), device="cuda"), torch.empty((3, 1, T))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor_normalized(part, T, 1, RATE, "peak", mono=True, out=out)
    for out in (torch.empty((3, 1, N_MELS, N_OUT), dtype=torch.float64, device="cuda"), torch.empty((3, 1, N_MELS, N_OUT + 1), device="cuda"),
                torch.empty((3, 1, N_MELS, N_OUT))):
        with pytest.raises(ValueError):
            afgpu.batch_decode_mel_normalized(part, T, out=out, feat_norm="whisper")
    with pytest.raises(ValueError):
        afgpu.batch_decode_tensor_normalized(part, T, 1, RATE, "loudness", mono=True)
    with pytest.raises(ValueError):
        afgpu.batch_decode_mel_normalized(part, T, feat_norm="wisper")
    with pytest.raises(afgpu.AfgError):
        afgpu.batch_decode_tensor_normalized(part, T, 1, RATE, "peak", target=-1.0, mono=True)
    empty, meta, stats = afgpu.batch_decode_tensor_normalized([], T, 2, RATE, "rms", return_stats=True)
    assert tuple(empty.shape) == (0, 2, T) and empty.is_cuda and meta == [] and stats.shape == (0,)
    empty, meta = afgpu.batch_decode_mel_normalized([], T, wave_norm="peak", feat_norm="whisper")
    assert tuple(empty.shape) == (0, 1, N_MELS, N_OUT) and empty.is_cuda and meta == []
