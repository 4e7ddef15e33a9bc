"""afgpu.batch_decode_fbank on a small corpus -- a few generated files of different formats, files at 8 and 44.1 kHz, a
damaged file and one that is no audio, to 16 kHz: every slab is afgpu.fbank_tensor applied to the matching row of
afgpu.batch_decode_tensor_resampled of the same list, bit for bit, in both layouts, with one channel (mono mix) and two,
whatever the sublists; a failed file keeps its status and message and gets the zero row's slab; the returned lengths are the
frames each file's own resampled samples give."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64m
import fbank_model as fm
import melspec_model as mm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T = 16000, 4000
IN_CHANNELS = 3                                                  # some of the generated files have three channels
KW = dict(num_mel_bins=23, use_energy=True, energy_floor=0.0, scale=32768.0)
LAYOUTS = {"frames-major": afgpu.FBANK_FRAMES_MAJOR, "mel-major": afgpu.FBANK_MEL_MAJOR}
EDGES = {"snip": True, "mirror": False}
N_OUT = {"snip": 23, "mirror": 25}


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()[:4]                                    # a few formats
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 1001), (44100, 2, 12000)):
        files.append(wb.wav_file(f64m.KIND_S16, ch, rate, wb.random_samples(rng, f64m.KIND_S16, ch * frames)))
    files.append(files[2][:-100])                                # a file cut short
    files.append(b"RIFF" + b"\x00" * 40)
    at = {"r8000": base, "r44100": base + 1, "damaged": base + 2, "junk": base + 3}
    made = {"files": files, "at": at}
    with pytest.MonkeyPatch.context() as mp:                     # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        for channels in (1, 2):
            tensor, meta = afgpu.batch_decode_tensor_resampled(files, T, channels, RATE, mono=channels == 1, in_channels=IN_CHANNELS, n_threads=4)
            torch.cuda.synchronize()
            assert [i for i, m in enumerate(meta) if m["status"] != 0] == [at["damaged"], at["junk"]]
            want = {}
            for edge, snip in EDGES.items():
                for name, layout in LAYOUTS.items():             # made once, never changed
                    want[edge, name] = afgpu.fbank_tensor(tensor, RATE, snip_edges=snip, layout=layout, **KW).cpu().numpy()
                    want[edge, name].setflags(write=False)
            made[channels] = {"meta": meta, "want": want}
    return made


def lengths_of(meta, edge):
    """the frames of ceil(frames * 16000 / rate) samples, at most T of them; 0 for a file that failed"""
    prm = fm.params(snip_edges=EDGES[edge])
    out = []
    for m in meta:
        valid = min(T, -(-int(m["frames"]) * RATE // int(m["samplerate"]))) if m["status"] == 0 else 0
        out.append(min(N_OUT[edge], fm.n_frames(valid, prm.win_length, prm.hop, prm.snip_edges)))
    return out


def decode(files, channels, edge, name, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    F, cols = N_OUT[edge], 24
    shape = (len(files), channels) + ((F, cols) if name == "frames-major" else (cols, F))
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    got, meta, lengths = afgpu.batch_decode_fbank(files, T, RATE, snip_edges=EDGES[edge], layout=LAYOUTS[name], mono=channels == 1, channels=channels,
                                                  in_channels=IN_CHANNELS, out=out, n_threads=4, **KW, **kw)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy(), meta, lengths


def same(got, want):
    bad = mm.same_bits(got, want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("edge", list(EDGES))
def test_every_slab_is_the_kernels_of_the_resampled_row(corpus, edge, name, channels):
    got, meta, lengths = decode(corpus["files"], channels, edge, name)
    same(got, corpus[channels]["want"][edge, name])
    assert meta == corpus[channels]["meta"]
    assert list(lengths) == lengths_of(meta, edge)
    at = corpus["at"]
    assert lengths[at["damaged"]] == 0 and lengths[at["junk"]] == 0 and 0 < lengths[at["r8000"]] < N_OUT[edge] == lengths[at["r44100"]]
    zero = afgpu.fbank_tensor(torch.zeros(1, T, device="cuda"), RATE, snip_edges=EDGES[edge], layout=LAYOUTS[name], **KW).cpu().numpy()
    for bad in (at["damaged"], at["junk"]):                      # what an all-zero row gives, status and message kept, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"]
        for c in range(channels):
            same(got[bad, c], zero[0])
    assert np.isfinite(got).all() and got[at["r44100"]].max() > 0.0 and got[at["r8000"]].max() > 0.0


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_slabs_do_not_depend_on_the_sublists(corpus, name):
    L = afgpu.lib()
    assert L.afg_dev_option(b"mel_scratch_bytes", 1) == 0        # every file its own sublist
    try:
        got, meta, lengths = decode(corpus["files"], 2, "mirror", name)
    finally:
        assert L.afg_dev_option(b"mel_scratch_bytes", -1) == 0   # restored
    same(got, corpus[2]["want"]["mirror", name])
    assert meta == corpus[2]["meta"] and list(lengths) == lengths_of(meta, "mirror")


def test_n_out_first_frame_and_the_defaults(corpus):
    files = corpus["files"][:3]
    y, meta, lengths = afgpu.batch_decode_fbank(files, T, RATE, in_channels=IN_CHANNELS, n_out=20, **KW)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (3, 1, 20, 24) and [m["status"] for m in meta] == [0, 0, 0] and (lengths <= 20).all()
    same(y.cpu().numpy(), corpus[1]["want"]["snip", "frames-major"][:3, :, :20])
    d, _, _ = afgpu.batch_decode_fbank(files, T, in_channels=IN_CHANNELS)         # torchaudio's defaults: 23 mels, no energy column
    assert tuple(d.shape) == (3, 1, 23, 23)
    empty, none, no_lengths = afgpu.batch_decode_fbank([], T, RATE, **KW)
    assert none == [] and tuple(empty.shape) == (0, 1, 23, 24) and len(no_lengths) == 0
