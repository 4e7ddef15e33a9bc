"""afgpu.batch_decode_pitch on a small corpus -- every fixture format build_files makes, files at 8 and 44.1 kHz, a damaged
file and one that is no audio, to 16 kHz: over each file's own frames both planes are afgpu.yin_tensor applied to the matching
row of afgpu.batch_decode_tensor_resampled of the same list, bit for bit, with one channel (mono mix) and two, whatever the
sublists; the frames past a file's own are +0.0f; a failed file keeps its status and message and has no frames; the returned
lengths are the frames each file's own resampled samples give."""
import numpy as np
import pytest
import torch

import afgpu
import f64_model as f64m
import wav_bitstream as wb
import yin_model as ym
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

RATE, T = 16000, 6000
IN_CHANNELS = 3                                                  # some of the generated files have three channels
KW = dict(fmin=50, fmax=500, frame_length=1024)                  # W 512, hop 256, lags 32 .. 320
MODEL = {"zero": ym.params(RATE, 1024, 512, 256, 32, 320), "reflect": ym.params(RATE, 1024, 512, 256, 32, 320, pad_mode=ym.PAD_REFLECT)}
PADS = {"zero": afgpu.MEL_PAD_ZERO, "reflect": afgpu.MEL_PAD_REFLECT}
N_OUT = 24


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()                                        # every format
    base = len(files)
    rng = np.random.default_rng(72)
    for rate, ch, frames in ((8000, 1, 1001), (44100, 2, 30000)):
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
            failed = [i for i, m in enumerate(meta) if m["status"] != 0]
            assert at["damaged"] in failed and at["junk"] in failed
            want = {}
            for pad, mode in PADS.items():                       # made once, never changed
                want[pad] = afgpu.yin_tensor(tensor, RATE, pad_mode=mode, **KW).cpu().numpy()
                want[pad].setflags(write=False)
            made[channels] = {"meta": meta, "want": want}
    return made


def lengths_of(meta, pad):
    """the frames of ceil(frames * 16000 / rate) samples, at most T of them; 0 for a file that failed"""
    out = []
    for m in meta:
        valid = min(T, -(-int(m["frames"]) * RATE // int(m["samplerate"]))) if m["status"] == 0 else 0
        out.append(min(N_OUT, ym.n_frames(valid, MODEL[pad])) if valid else 0)
    return out


def decode(files, channels, pad, **kw):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    out = torch.full((len(files), channels, 2, N_OUT), float("nan"), dtype=torch.float32, device="cuda")
    got, meta, lengths = afgpu.batch_decode_pitch(files, T, RATE, pad_mode=PADS[pad], mono=channels == 1, channels=channels, in_channels=IN_CHANNELS,
                                                  out=out, n_threads=4, **KW, **kw)
    torch.cuda.synchronize()
    assert got is out
    return got.cpu().numpy(), meta, lengths


def check(got, lengths, want):
    """the kernel's bits over each file's own frames, +0.0f past them"""
    for i, n in enumerate(lengths):
        assert (got[i, :, :, :n].view(np.uint32) == want[i, :, :, :n].view(np.uint32)).all(), i
        assert (got[i, :, :, n:].view(np.uint32) == 0).all(), i


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("pad", list(PADS))
def test_every_plane_is_the_kernels_of_the_resampled_row(corpus, pad, channels):
    got, meta, lengths = decode(corpus["files"], channels, pad)
    assert meta == corpus[channels]["meta"]
    assert list(lengths) == lengths_of(meta, pad)
    check(got, lengths, corpus[channels]["want"][pad])
    at = corpus["at"]
    assert lengths[at["damaged"]] == 0 and lengths[at["junk"]] == 0 and 0 < lengths[at["r8000"]] < N_OUT == lengths[at["r44100"]]
    for bad in (at["damaged"], at["junk"]):                      # status and message kept, no frames, the neighbours undisturbed
        assert meta[bad]["status"] != 0 and meta[bad]["message"] and (got[bad] == 0).all()
    own = got[at["r44100"]]                                      # 16-bit noise: finite, and |shift| < 1 round a lag of 32 .. 320
    assert np.isfinite(own).all() and own[:, 0].min() >= RATE / 321 and own[:, 0].max() <= RATE / 31 and own[:, 1].min() > 0.0


def test_the_planes_do_not_depend_on_the_sublists(corpus):
    L = afgpu.lib()
    try:
        assert L.afg_dev_option(b"resample_scratch_bytes", 1) == 0                 # every file its own sublist
        got, meta, lengths = decode(corpus["files"], 2, "reflect")
        assert L.afg_dev_option(b"resample_scratch_bytes", 3 * 2 * T * 4 + 8) == 0   # three files' slabs of this stage's scratch
        got3, meta3, lengths3 = decode(corpus["files"], 2, "reflect")
    finally:
        assert L.afg_dev_option(b"resample_scratch_bytes", -1) == 0                # restored
    for g, m, n in ((got, meta, lengths), (got3, meta3, lengths3)):
        assert m == corpus[2]["meta"] and list(n) == lengths_of(m, "reflect")
        check(g, n, corpus[2]["want"]["reflect"])


def test_n_out_and_the_defaults(corpus):
    files = corpus["files"][:3]
    y, meta, lengths = afgpu.batch_decode_pitch(files, T, RATE, in_channels=IN_CHANNELS, n_out=10, **KW)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (3, 1, 2, 10) and [m["status"] for m in meta] == [0, 0, 0] and (lengths <= 10).all()
    check(y.cpu().numpy(), lengths, corpus[1]["want"]["zero"][:3, :, :, :10])
    d, _, _ = afgpu.batch_decode_pitch(files, 16000, RATE, 50, 500, in_channels=IN_CHANNELS)      # librosa's defaults: 2048 / 1024 / 512
    assert tuple(d.shape) == (3, 1, 2, 32)
    empty, none, no_lengths = afgpu.batch_decode_pitch([], T, RATE, **KW)
    assert none == [] and tuple(empty.shape) == (0, 1, 2, N_OUT) and len(no_lengths) == 0
