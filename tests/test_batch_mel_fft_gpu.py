"""afgpu.batch_decode_mel(..., algorithm="fft") on the corpus of tests/test_batch_mel_gpu.py -- one short generated file of every
format, files at 8 and 44.1 kHz, a damaged file and one that is no audio, to 16 kHz mono: the features are afgpu.melspec_fft
applied to afgpu.batch_decode_tensor_resampled of the same list, bit for bit, whatever the sublists; they lie inside the
interval of the float64 model; the normalised entry is tests/normalize_model.py applied to them; and the default is still
the direct path."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64m
import melspec_fft_model as fm
import melspec_model as mm
import normalize_model as nm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T, N_FFT, HOP, N_MELS = 16000, 4000, 400, 160, 80
N_OUT = 26
IN_CHANNELS = 3                                                  # two of the generated files have three channels


def kernel(tensor, out_kind):
    """afgpu.melspec_fft over the rows of a [files, 1, T] device tensor: [files, N_MELS, N_OUT] on the host"""
    n = tensor.shape[0]
    rows = np.zeros(n, afgpu.MEL_ROW_DTYPE)
    rows["in_off"], rows["in_frames"] = np.arange(n) * T, T
    rows["out_off"], rows["out_frames"] = np.arange(n) * N_MELS * N_OUT, N_OUT
    prm = afgpu.mel_params(N_FFT, HOP, N_MELS, out_kind=out_kind)
    tiles = afgpu.mel_fft_layout(rows, prm)
    table, bank = afgpu.mel_fft_tables(N_FFT), afgpu.mel_filters(RATE, N_FFT, N_MELS)
    d_mel = torch.full((n, N_MELS, N_OUT), float("nan"), dtype=torch.float32, device="cuda")
    afgpu.melspec_fft(n, torch.from_numpy(rows.view(np.uint8).copy()).cuda(), tiles, prm, tensor, tensor.numel(), torch.from_numpy(table).cuda(),
                      table.size, torch.from_numpy(bank.reshape(-1).copy()).cuda(), bank.size, d_mel, d_mel.numel())
    torch.cuda.synchronize()
    return d_mel.cpu().numpy()


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()                                        # one file per format
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 3001), (44100, 2, 9000)):
        files.append(wb.wav_file(f64m.KIND_S16, ch, rate, wb.random_samples(rng, f64m.KIND_S16, ch * frames)))
    files.append(files[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    at = {"r8000": base, "r44100": base + 1, "damaged": base + 2, "junk": base + 3}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, 1, RATE, mono=True, in_channels=IN_CHANNELS, n_threads=4)
        torch.cuda.synchronize()
    assert [i for i, m in enumerate(meta) if m["status"] != 0] == [at["damaged"], at["junk"]]
    assert mm.max_frames(T, N_FFT, HOP, True) == N_OUT
    want = {kind: kernel(tensor, kind) for kind in (afgpu.MEL_POWER, afgpu.MEL_LOG10)}     # made once, never changed
    for v in want.values():
        v.setflags(write=False)
    return {"files": files, "meta": meta, "at": at, "rows": tensor.cpu().numpy()[:, 0], "want": want}


def decode(files, normalized=False, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    out = torch.full((len(files), 1, N_MELS, N_OUT), float("nan"), dtype=torch.float32, device="cuda")
    fn = afgpu.batch_decode_mel_normalized if normalized else afgpu.batch_decode_mel
    got, meta = fn(files, T, RATE, in_channels=IN_CHANNELS, out=out, n_threads=4, **kw)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()[:, 0], meta


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("out_kind", [afgpu.MEL_POWER, afgpu.MEL_LOG10], ids=["power", "log10"])
def test_the_features_are_the_kernels_of_the_resampled_tensor_and_inside_the_interval(corpus, out_kind):
    got, meta = decode(corpus["files"], out_kind=out_kind, algorithm="fft")
    same(got, corpus["want"][out_kind])
    assert meta == corpus["meta"]
    bank = afgpu.mel_filters(RATE, N_FFT, N_MELS)
    for i, x in enumerate(corpus["rows"]):
        lo, hi, _ = fm.power_interval(x, bank, N_FFT, N_FFT, HOP, True, mm.PAD_REFLECT, N_OUT)
        if out_kind == afgpu.MEL_LOG10:
            lo, hi = fm.log_interval(lo, hi)
        hit = np.isnan(mm.frames_of(x, N_FFT, N_FFT, HOP, True, mm.PAD_REFLECT, N_OUT)).any(axis=1)     # (a generated file may hold a NaN sample)
        assert fm.outside(got[i][:, ~hit], lo[:, ~hit], hi[:, ~hit]).size == 0, i
        if out_kind == afgpu.MEL_POWER:
            assert np.isnan(got[i][:, hit]).all(), i
        else:
            assert (np.abs(got[i][:, hit] + 10.0) < 1e-5).all(), i
    for bad in (corpus["at"]["damaged"], corpus["at"]["junk"]):  # what an all-zero row gives, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and (got[bad].view(np.uint32) == got[bad].view(np.uint32)[0, 0]).all()
        assert got[bad][0, 0] == 0 if out_kind == afgpu.MEL_POWER else abs(float(got[bad][0, 0]) + 10.0) < 1e-5
    assert got[corpus["at"]["r8000"]].max() > (1.0 if out_kind == afgpu.MEL_POWER else 0.0)


def test_the_features_do_not_depend_on_the_sublists(corpus):
    L = afgpu.lib()
    assert L.afg_dev_option(b"mel_scratch_bytes", 1) == 0        # every file its own sublist
    try:
        got, meta = decode(corpus["files"], out_kind=afgpu.MEL_POWER, algorithm="fft")
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0
    same(got, corpus["want"][afgpu.MEL_POWER])
    assert meta == corpus["meta"]


def test_the_normalised_entry_is_the_model_over_the_fft_slabs(corpus):
    got, meta = decode(corpus["files"], normalized=True, feat_norm="whisper", algorithm="fft")
    prm = nm.params(nm.DYNAMIC_RANGE, **nm.WHISPER)
    slabs = corpus["want"][afgpu.MEL_LOG10].reshape(len(corpus["files"]), -1)
    want = np.stack([nm.apply(s, nm.group_stats(s.reshape(1, -1), prm), prm) for s in slabs])
    same(got.reshape(len(slabs), -1), want)
    assert meta == corpus["meta"]


def test_direct_is_the_default_and_the_keyword_changes_nothing_else(corpus):
    files = corpus["files"]
    plain, meta = decode(files)
    direct, meta_d = decode(files, algorithm="direct")
    same(direct, plain)
    assert meta == meta_d == corpus["meta"]
    plain_n, _ = decode(files, normalized=True, feat_norm="whisper")
    direct_n, _ = decode(files, normalized=True, feat_norm="whisper", algorithm="direct")
    same(direct_n, plain_n)
    assert mm.same_bits(plain, corpus["want"][afgpu.MEL_LOG10]).size > 0          # the two algorithms round differently
    with pytest.raises(afgpu.AfgError, match="n_fft 401"):                       # a size the direct path alone takes
        afgpu.batch_decode_mel(files[:2], T, RATE, n_fft=401, win_length=400, in_channels=IN_CHANNELS, algorithm="fft")
    ok, _ = afgpu.batch_decode_mel(files[:2], T, RATE, n_fft=401, win_length=400, in_channels=IN_CHANNELS)
    torch.cuda.synchronize()
    assert tuple(ok.shape) == (2, 1, N_MELS, mm.max_frames(T, 401, HOP, True)) and np.isfinite(ok.cpu().numpy()).any()
