"""afgpu.batch_decode_tensor (afg_batch_decode_to_device) on one file of every format, a damaged file and one that is no
audio: the tensor is what afgpu.batch_decode returns for the same list, collated by tests/collate_model.py, bit for bit --
whatever the stages' chunks, the file's neighbours or its place in the batch."""
import numpy as np
import pytest
import torch

import afgpu
import collate_model as cm
import f64_model as fm
import wav_bitstream as wb
from test_batch_transcode_gpu import build_files

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 4000), (8, 100000), (72, 256)]          # (the last: more rows than the 70-channel file has, a row longer than it)
DAMAGED, JUNK = 3, 7           # where the two bad files sit in the batch
LOUD, WIDE = 13, 14            # the float WAV that leaves [-1, 1] and holds NaNs; a WAV file of 70 channels (the kernel's path for more than 64)
WIDE_CHANNELS, WIDE_FRAMES = 70, 201


@pytest.fixture(scope="module")
def corpus(gpu):
    files = build_files()
    damaged = files[2][:-100]                                                    # a WAV file whose data chunk is cut short
    junk = b"RIFF" + b"\x00" * 40
    files = files[:DAMAGED] + [damaged] + files[DAMAGED:JUNK - 1] + [junk] + files[JUNK - 1:]
    files.append(wb.wav_file(fm.KIND_S16, WIDE_CHANNELS, 48000, wb.random_samples(np.random.default_rng(70), fm.KIND_S16, WIDE_CHANNELS * WIDE_FRAMES)))
    assert len(files) == WIDE + 1
    with pytest.MonkeyPatch.context() as mp:                 # (the tests run in the exact numeric mode: so does their reference)
        mp.setenv("AFG_NUMERIC", "exact")
        floats = afgpu.batch_decode(files, n_threads=4)
    assert [i for i, f in enumerate(floats) if f["status"] != 0] == [DAMAGED, JUNK]
    assert sorted({f["format"] for f in floats if f["status"] == 0}) == list(range(8))        # WAV, MP3, FLAC, OGG, OPUS, QOA, MOD, XM
    assert floats[WIDE]["channels"] == WIDE_CHANNELS and floats[WIDE]["frames"] == WIDE_FRAMES
    return {"files": files, "floats": floats}


def first_frames(floats, varied):
    if not varied:
        return None
    ff = [(37 * (i + 1)) % max(f["frames"], 1) for i, f in enumerate(floats)]
    ff[0] = floats[0]["frames"] - 1                                              # the last frame alone
    ff[1] = floats[1]["frames"] + 5                                              # past the end: an all-zero slab
    ff[4] = floats[4]["frames"]                                                  # exactly at the end
    return ff


def decode(files, C, T, ff=None):
    """through out=, prefilled with NaN: an element nobody wrote shows"""
    out = torch.full((len(files), C, T), float("nan"), dtype=torch.float32, device="cuda")
    got, meta = afgpu.batch_decode_tensor(files, T, C, first_frame=ff, out=out, n_threads=4)
    assert got is out
    torch.cuda.synchronize()
    return got.cpu().numpy(), meta


def same(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def meta_of(floats):
    return [{k: v for k, v in f.items() if k != "pcm"} for f in floats]


@pytest.mark.parametrize("varied", [False, True], ids=["from-0", "varied-first-frame"])
@pytest.mark.parametrize("C,T", SHAPES)
def test_the_tensor_is_the_collated_float_batch(corpus, C, T, varied):
    files, floats = corpus["files"], corpus["floats"]
    ff = first_frames(floats, varied)
    got, meta = decode(files, C, T, ff)
    want = cm.tensor(floats, C, T, ff)
    same(got, want)
    assert meta == meta_of(floats)
    for bad in (DAMAGED, JUNK):
        assert meta[bad]["status"] != 0 and (got[bad].view(np.uint32) == 0).all()
    if varied:
        assert (got[1] == 0).all() and (got[4] == 0).all()
        assert (got[0, :, 1:] == 0).all() if T > 1 else True
    assert np.isnan(floats[LOUD]["pcm"]).any()                                   # (the float WAV's NaNs come through: compared above)
    if C >= WIDE_CHANNELS and not varied:
        assert (got[WIDE, :WIDE_CHANNELS, :WIDE_FRAMES] == floats[WIDE]["pcm"].T).all() and (got[WIDE, WIDE_CHANNELS:] == 0).all()


def test_a_new_tensor_is_made_on_the_current_device(corpus):
    files, floats = corpus["files"], corpus["floats"]
    got, meta = afgpu.batch_decode_tensor(files[:3], 700, 2)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3, 2, 700) and got.is_contiguous()
    torch.cuda.synchronize()
    same(got.cpu().numpy(), cm.tensor(floats[:3], 2, 700))
    empty, meta = afgpu.batch_decode_tensor([], 700, 2)
    assert tuple(empty.shape) == (0, 2, 700) and empty.is_cuda and meta == []
    for out in (torch.empty((3, 2, 700), dtype=torch.float64, device="cuda"), torch.empty((3, 2, 701), device="cuda"),
                torch.empty((3, 2, 700)), torch.empty((3, 700, 2), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError):
            afgpu.batch_decode_tensor(files[:3], 700, 2, out=out)


def chunk_counts(floats, value):
    """how many chunks of `value` samples a file's delivered samples make: what stage_chunk_samples does to the stages that
    cut inside a file (the others cut between files: with each file twice they have something to cut between)"""
    return [-(-f["frames"] * f["channels"] // value) if f["status"] == 0 else 0 for f in floats]


@pytest.mark.parametrize("value", [4096, 1000])
def test_the_tensor_does_not_depend_on_the_chunks(corpus, value):
    files, floats = corpus["files"], corpus["floats"]
    order = list(range(len(files))) * 2
    C, T = 3, 30000
    ff = [(11 * i) % 500 for i in range(len(order))]
    plain, _ = decode([files[k] for k in order], C, T, ff)
    L = afgpu.lib()
    assert L.afg_dev_option(b"stage_chunk_samples", value) == 0
    try:
        got, meta = decode([files[k] for k in order], C, T, ff)
        chunked = afgpu.batch_decode([files[k] for k in order], n_threads=4)
    finally:
        assert L.afg_dev_option(b"stage_chunk_samples", -1) == 0
    same(got, plain)
    same(got, cm.tensor([floats[k] for k in order], C, T, ff))
    assert meta == meta_of([floats[k] for k in order])
    for item, k in zip(chunked, order):                                         # (the option leaves the float call as it was)
        assert item["frames"] == floats[k]["frames"]
    # the option did cut: at least one file is longer than a chunk, so its samples reached the tensor from several chunks
    assert max(chunk_counts(floats, value)) > 1
    wav = [k for k, f in enumerate(floats) if f["status"] == 0 and f["format"] == afgpu.FORMAT_WAV]
    assert any(chunk_counts(floats, (value + 4095) // 4096 * 4096)[k] > 1 for k in wav)       # (the WAV stage cuts files at tile borders)


def test_a_files_slab_does_not_depend_on_its_neighbours(corpus):
    files, floats = corpus["files"], corpus["floats"]
    C, T = 2, 9000
    whole, _ = decode(files, C, T)
    for k in (0, 2, 5, 6, 12, WIDE):
        twice, meta = decode([files[k], files[DAMAGED], files[k]], C, T)
        alone, _ = decode([files[k]], C, T)
        same(twice[0], whole[k])
        same(twice[2], whole[k])
        same(alone[0], whole[k])
        assert (twice[1].view(np.uint32) == 0).all() and meta[1]["status"] != 0 and meta[0] == meta[2] == meta_of(floats)[k]
