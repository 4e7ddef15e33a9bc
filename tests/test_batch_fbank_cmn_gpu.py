"""afgpu.batch_decode_fbank_cmn on the corpus of test_batch_fbank_gpu.py -- a few generated files of different formats, files
at 8 and 44.1 kHz (the first shorter than T, so that its own frames end in front of n_out), a damaged file and one that is no
audio: the one-call entry gives the bits of afgpu.batch_decode_fbank followed by afgpu.sliding_cmn_tensor in place with
valid_frames set to the returned counts, with one channel and two, in both layouts, whatever the sublists; the frames behind a
file's count and the slabs of the failed files are batch_decode_fbank's."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64m
import melspec_model as mm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T = 16000, 4000
IN_CHANNELS = 3
KW = dict(num_mel_bins=23, use_energy=True, energy_floor=0.0, scale=32768.0, snip_edges=False)
N_OUT, COLS = 25, 24
LAYOUTS = {"frames-major": (afgpu.FBANK_FRAMES_MAJOR, "frames"), "mel-major": (afgpu.FBANK_MEL_MAJOR, "cols")}
WINDOWS = {"centred-10-vars": dict(cmn_window=10, min_cmn_window=100, center=True, norm_vars=True),
           "causal-600-100": dict(cmn_window=600, min_cmn_window=100, center=False, norm_vars=False)}


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()[:4]
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 1001), (44100, 2, 12000)):
        files.append(wb.wav_file(f64m.KIND_S16, ch, rate, wb.random_samples(rng, f64m.KIND_S16, ch * frames)))
    files.append(files[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    return {"files": files, "at": {"r8000": base, "r44100": base + 1, "damaged": base + 2, "junk": base + 3}}


def shape_of(n, channels, name):
    return (n, channels) + ((N_OUT, COLS) if name == "frames-major" else (COLS, N_OUT))


def two_calls(files, channels, name, window):
    """batch_decode_fbank's tensor, then the tensor call over every slab's own frames, in place; and the plain features"""
    layout, word = LAYOUTS[name]
    feats, meta, lengths = afgpu.batch_decode_fbank(files, T, RATE, layout=layout, mono=channels == 1, channels=channels, in_channels=IN_CHANNELS,
                                                    n_threads=4, **KW)
    torch.cuda.synchronize()
    plain = feats.cpu().numpy()
    out = afgpu.sliding_cmn_tensor(feats, layout=word, valid_frames=np.repeat(lengths, channels), out=feats, **WINDOWS[window])
    torch.cuda.synchronize()
    assert out is feats
    return out.cpu().numpy(), plain, meta, lengths


def one_call(files, channels, name, window):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    out = torch.full(shape_of(len(files), channels, name), float("nan"), dtype=torch.float32, device="cuda")
    got, meta, lengths = afgpu.batch_decode_fbank_cmn(files, T, samplerate=RATE, layout=LAYOUTS[name][0], mono=channels == 1, channels=channels,
                                                      in_channels=IN_CHANNELS, out=out, n_threads=4, **WINDOWS[window], **KW)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy(), meta, lengths


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def frames_of(a, name, lo, hi):
    return a[..., lo:hi, :] if name == "frames-major" else a[..., lo:hi]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("window", list(WINDOWS))
def test_one_call_gives_the_two_calls_bits(corpus, window, name, channels):
    files, at = corpus["files"], corpus["at"]
    want, plain, meta0, lengths0 = two_calls(files, channels, name, window)
    got, meta, lengths = one_call(files, channels, name, window)
    same(got, want)
    assert meta == meta0 and list(lengths) == list(lengths0)
    assert lengths[at["damaged"]] == 0 and lengths[at["junk"]] == 0 and 0 < lengths[at["r8000"]] < N_OUT == lengths[at["r44100"]]
    for bad in (at["damaged"], at["junk"]):                      # status and message kept, the slab batch_decode_fbank's
        assert meta[bad]["status"] != 0 and meta[bad]["message"]
        same(got[bad], plain[bad])
    short = at["r8000"]                                          # the tail frames are the fbank call's, the own frames are not
    n = int(lengths[short])
    same(frames_of(got[short], name, n, N_OUT), frames_of(plain[short], name, n, N_OUT))
    assert (frames_of(got[short], name, 0, n) != frames_of(plain[short], name, 0, n)).any()
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_slabs_do_not_depend_on_the_sublists(corpus, name):
    want, _, meta0, lengths0 = two_calls(corpus["files"], 2, name, "centred-10-vars")
    L = afgpu.lib()
    assert L.afg_dev_option(b"mel_scratch_bytes", 1) == 0        # every file its own sublist
    try:
        got, meta, lengths = one_call(corpus["files"], 2, name, "centred-10-vars")
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0   # restored
    same(got, want)
    assert meta == meta0 and list(lengths) == list(lengths0)


def test_refusals_and_the_empty_list(corpus):
    files = corpus["files"][:2]
    with pytest.raises(afgpu.AfgError):
        afgpu.batch_decode_fbank_cmn(files, T, cmn_window=0, samplerate=RATE, in_channels=IN_CHANNELS, **KW)
    with pytest.raises(afgpu.AfgError):
        afgpu.batch_decode_fbank_cmn(files, T, min_cmn_window=0, samplerate=RATE, in_channels=IN_CHANNELS, **KW)
    empty, none, no_lengths = afgpu.batch_decode_fbank_cmn([], T, samplerate=RATE, **KW)
    assert none == [] and tuple(empty.shape) == (0, 1, N_OUT, COLS) and len(no_lengths) == 0
