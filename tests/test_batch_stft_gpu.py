"""afgpu.batch_decode_stft on the corpus of tests/test_batch_mel_fft_gpu.py -- one short generated file of every format, files
at 8 and 44.1 kHz, a damaged file and one that is no audio, to 16 kHz: every slab is afgpu.stft applied to the matching row of
afgpu.batch_decode_tensor_resampled of the same list, bit for bit, for power and complex output, one channel (mono mix) and
two, whatever the sublists; a failed file keeps its status and message and gets the zero row's slab."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64m
import melspec_model as mm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T, N_FFT, HOP = 16000, 4000, 400, 160
N_BINS, N_OUT = N_FFT // 2 + 1, 26
IN_CHANNELS = 3                                                  # two of the generated files have three channels
KINDS = {"power": afgpu.STFT_POWER, "complex": afgpu.STFT_COMPLEX}


def kernel(tensor, out_kind):
    """afgpu.stft over the rows of a [files, channels, T] device tensor: [files, channels, N_BINS, N_OUT (, 2)] on the host"""
    n = tensor.shape[0] * tensor.shape[1]
    comps = 2 if out_kind == afgpu.STFT_COMPLEX else 1
    rows = np.zeros(n, afgpu.MEL_ROW_DTYPE)
    rows["in_off"], rows["in_frames"] = np.arange(n) * T, T
    rows["out_off"], rows["out_frames"] = np.arange(n) * comps * N_BINS * N_OUT, N_OUT
    prm = afgpu.stft_params(N_FFT, HOP, out_kind=out_kind)
    tiles = afgpu.stft_layout(rows, prm)
    table = afgpu.mel_fft_tables(N_FFT)
    d_out = torch.full((n, N_BINS, N_OUT * comps), float("nan"), dtype=torch.float32, device="cuda")
    afgpu.stft(n, torch.from_numpy(rows.view(np.uint8).copy()).cuda(), tiles, prm, tensor, tensor.numel(), torch.from_numpy(table).cuda(), table.size,
               d_out, d_out.numel())
    torch.cuda.synchronize()
    shape = tuple(tensor.shape[:2]) + (N_BINS, N_OUT) + ((2,) if comps == 2 else ())
    return d_out.cpu().numpy().reshape(shape)


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
    assert mm.max_frames(T, N_FFT, HOP, True) == N_OUT
    made = {"files": files, "at": at}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for channels in (1, 2):
            tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, channels, RATE, mono=channels == 1, in_channels=IN_CHANNELS, n_threads=4)
            torch.cuda.synchronize()
            assert [i for i, m in enumerate(meta) if m["status"] != 0] == [at["damaged"], at["junk"]]
            want = {name: kernel(tensor, kind) for name, kind in KINDS.items()}      # made once, never changed
            for v in want.values():
                v.setflags(write=False)
            made[channels] = {"meta": meta, "want": want}
    return made


def decode(files, channels, name, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    shape = (len(files), channels, N_BINS, N_OUT) + ((2,) if name == "complex" else ())
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_stft(files, T, RATE, N_FFT, HOP, out_kind=KINDS[name], mono=channels == 1, channels=channels,
                                        in_channels=IN_CHANNELS, out=out, n_threads=4, **kw)
    torch.cuda.synchronize()
    if name == "complex":
        assert got.dtype == torch.complex64 and tuple(got.shape) == shape[:-1] and got.data_ptr() == out.data_ptr()
        return torch.view_as_real(got).cpu().numpy(), meta
    assert got is out
    return got.cpu().numpy(), meta


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(KINDS))
def test_every_slab_is_the_kernels_of_the_resampled_row(corpus, name, channels):
    got, meta = decode(corpus["files"], channels, name)
    want = corpus[channels]["want"][name]
    same(got, want)
    assert meta == corpus[channels]["meta"]
    at = corpus["at"]
    for bad in (at["damaged"], at["junk"]):                      # what an all-zero row gives, status and message kept, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"]
        assert ((got[bad].view(np.uint32) & 0x7fffffff) == 0).all()
    assert np.nanmax(np.abs(got[at["r44100"]])) > 1.0 and np.nanmax(np.abs(got[at["r8000"]])) > 1.0     # the file in front of them, too


@pytest.mark.parametrize("name", list(KINDS))
def test_the_slabs_do_not_depend_on_the_sublists(corpus, name):
    L = afgpu.lib()
    assert L.afg_dev_option(b"mel_scratch_bytes", 1) == 0        # every file its own sublist
    try:
        got, meta = decode(corpus["files"], 2, name)
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0   # restored
    same(got, corpus[2]["want"][name])
    assert meta == corpus[2]["meta"]
    again, _ = decode(corpus["files"], 2, name)
    same(again, got)


def test_the_complex_tensor_and_the_defaults(corpus):
    files = corpus["files"][:3]
    z, meta = afgpu.batch_decode_stft(files, T, RATE, N_FFT, HOP, out_kind=afgpu.STFT_COMPLEX, in_channels=IN_CHANNELS)
    p, _ = afgpu.batch_decode_stft(files, T, RATE, N_FFT, HOP, in_channels=IN_CHANNELS)
    m, _ = afgpu.batch_decode_stft(files, T, RATE, N_FFT, HOP, out_kind=afgpu.STFT_MAGNITUDE, in_channels=IN_CHANNELS, n_out=20)
    torch.cuda.synchronize()
    assert z.dtype == torch.complex64 and tuple(z.shape) == (3, 1, N_BINS, N_OUT) and z.is_contiguous()
    assert p.dtype == torch.float32 and tuple(p.shape) == (3, 1, N_BINS, N_OUT)
    assert tuple(m.shape) == (3, 1, N_BINS, 20) and (np.nan_to_num(m.cpu().numpy()) >= 0).all()
    same(torch.view_as_real(z).cpu().numpy(), corpus[1]["want"]["complex"][:3])
    same(p.cpu().numpy(), corpus[1]["want"]["power"][:3])
    empty, none = afgpu.batch_decode_stft([], T, RATE, N_FFT, HOP, out_kind=afgpu.STFT_COMPLEX)
    assert none == [] and empty.dtype == torch.complex64 and tuple(empty.shape) == (0, 1, N_BINS, N_OUT)
    assert [x["status"] for x in meta] == [0, 0, 0]
