"""FastTracker II XM on the device: the mixer (afg_xm_render_hip), the stream's reads, the module functions and the batch
path, compared as uint32 with tests/libxm_model.py driven by the same reads; no frame is left out."""
import os

import numpy as np
import pytest

import afgpu
import libxm_model as xm
import xm_bitstream as xb
from test_mod_gpu import mixed_files

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def claimed_by_mp3(data):
    try:
        afgpu.mp3_parse(data)
        return True
    except afgpu.AfgError:
        return False


def songs(seed, n=6):
    rng = np.random.default_rng(seed)
    return [xb.random_song(rng, channels=[4, 1, 8, 2, 32, 6][i % 6]) for i in range(n)]


@pytest.mark.parametrize("align", [16, 1])
def test_render_hip_batch(gpu, align):
    """align 1 puts songs on odd output frames: the mixer's 8-byte store path."""
    import torch
    files = songs(1, 6)
    parsed = [afgpu.xm_parse(f) for f in files]
    sng, ticks, segs, data, aux, frames = afgpu.xm_layout(parsed, align)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(gpu)
    d_out = torch.full((frames * 2 + 64,), float("nan"), dtype=torch.float32, device=gpu)
    d_aux = torch.from_numpy(aux).to(gpu)
    afgpu.xm_render(len(files), dev(sng), dev(segs), dev(ticks), dev(data), d_aux, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()[:frames * 2].reshape(-1, 2)
    written = np.zeros(frames, bool)
    for i, f in enumerate(files):
        want = xm.decode_batch(f)
        o = int(sng[i]["out_frame"])
        assert len(want) == parsed[i]["frames"] and not parsed[i]["capped"]
        assert np.array_equal(bits(got[o:o + len(want)]), bits(want)), i
        written[o:o + len(want)] = True
    assert np.isnan(got[~written]).all() and np.isnan(d_out.cpu().numpy()[frames * 2:]).all()   # nothing outside the songs


@pytest.mark.parametrize("reads", [[1], [7], [1000], [4096], [400000], [1, 7, 1000, 4096, 33]])
def test_stream_reads(gpu, reads):
    if reads == [1]:
        # a song of a few ticks, so that 1-frame reads cross ramps, cross-fades and the tick that raises the loop count
        data = xb.random_song(np.random.default_rng(3), channels=4, rows=5, n_patterns=1)
    else:
        data = xb.random_song(np.random.default_rng(2 + len(reads)), channels=4)
    total = len(xm.decode_batch(data))
    plan = []
    while sum(plan) <= total:                                 # the read that crosses the song's end is the last with frames
        plan.append(reads[len(plan) % len(reads)])
    if reads == [1]:
        plan += [1] * 40                                      # zeros: the reads inside the tick that raised the loop count ...
    plan = plan + [5]
    want, _ = xm.decode_stream(data, plan)
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    assert not s.isError(), s.errorMessage()
    assert s.getFormat() == afgpu.FORMAT_XM and s.getNumChannels() == 2 and s.getSamplerate() == 44100.0
    assert s.getLengthInFrames() == afgpu.UNKNOWN_LENGTH and s.isModule() and s.canSeek()
    assert not s.seekPosition(0)                              # a module seeks by pattern and row
    for n, w in zip(plan, want):
        buf = np.full((n, 2), np.nan, np.float32)
        got = s.readSamplesFloat(buf)
        assert got == len(w)                                  # all the frames asked for, or 0 once the loop count is 1
        assert np.array_equal(bits(buf[:got]), bits(w))
    # the read that was under way when the loop count was raised is filled with zeros, and every read after it returns 0
    filled = [i for i, w in enumerate(want) if len(w)]
    last = filled[-1]
    assert sum(plan[:last + 1]) > total and all(len(w) == 0 for w in want[last + 1:]) and len(want[-1]) == 0
    tail = want[last][total - sum(plan[:last]):]
    assert len(tail) and not tail.any()


def test_module_queries_and_seek(gpu):
    data = xb.random_song(np.random.default_rng(31), channels=3, rows=16, n_patterns=3)
    m = xm.load(data)
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    assert s.countModulePatterns() == m.num_patterns and s.getModuleLength() == m.length
    for p in range(-1, m.num_patterns + 2):
        assert s.rowsInPattern(p) == (m.patterns[p][0] if 0 <= p < m.num_patterns else -1)
    pl = xm.Player(m)
    for n in (3000, 1234):
        buf = np.full((n, 2), np.nan, np.float32)
        assert s.readSamplesFloat(buf) == n
        assert np.array_equal(bits(buf), bits(pl.generate(n)))
        assert (s.tellModulePattern(), s.tellModuleRow()) == (pl.index, pl.row)
    assert s.seekPosition(1, 5) and pl.seek(1, 5)
    assert (s.tellModulePattern(), s.tellModuleRow()) == (1, 5)
    assert not s.seekPosition(m.length, 0) and not s.seekPosition(0, 256)
    buf = np.full((5000, 2), np.nan, np.float32)
    assert s.readSamplesFloat(buf) == 5000
    assert np.array_equal(bits(buf), bits(pl.generate(5000)))


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
def test_batch_mixes_xm_with_other_formats(gpu, mode, monkeypatch):
    """XM has one numeric mode.  The other files (MOD, MP3, FLAC, QOA, junk) decode as they do without the XMs beside them."""
    if mode == "tolerance":
        monkeypatch.delenv("AFG_NUMERIC", raising=False)
    else:
        monkeypatch.setenv("AFG_NUMERIC", "exact")
    others, _ = mixed_files()
    # MP3 is probed before XM (stream.d:1706-1750), here as in the reference: an XM whose sample bytes pass for MPEG frames is an
    # MP3 to both.  Such a generated file is no case of this test.
    xms = [f for f in songs(9, 8) if not claimed_by_mp3(f)][:3]
    assert len(xms) == 3
    files = [xms[0]] + others[:3] + [xms[1]] + others[3:] + [xms[2]]
    is_xm = [True] + [False] * 3 + [True] + [False] * (len(others) - 3) + [True]
    out = afgpu.batch_decode(files, n_threads=3)
    alone = iter(afgpu.batch_decode(others, n_threads=3))
    k = 0
    for item, x in zip(out, is_xm):
        if x:
            want = xm.decode_batch(xms[k])
            k += 1
            assert item["status"] == 0 and item["message"] is None and item["format"] == afgpu.FORMAT_XM
            assert item["channels"] == 2 and item["samplerate"] == 44100.0 and item["frames"] == len(want)
            assert np.array_equal(bits(item["pcm"]), bits(want))
            continue
        ref = next(alone)
        assert item["status"] == ref["status"] and item["message"] == ref["message"] and item["format"] == ref["format"]
        if ref["status"] == 0:
            assert item["frames"] == ref["frames"] and np.array_equal(bits(item["pcm"]), bits(ref["pcm"]))
        else:
            assert item["pcm"] is None and item["message"] == "Cannot decode stream: unrecognized encoding."
    # an XM-headed file the loader refuses stays refused
    bad = bytearray(xms[0])
    bad[64] = 0
    bad[65] = 0                                                # song length 0
    item = afgpu.batch_decode([bytes(bad)])[0]
    assert item["status"] != 0 and item["message"] == "Cannot decode stream: unrecognized encoding."


def test_capped_endless_song(gpu):
    """The 30-minute cap.  The model steps frame by frame in Python, so it covers the first 200000 frames; the song's only
    tick never ends and its one looped note is periodic from then on."""
    data = xb.endless_song()
    out = afgpu.batch_decode([data])[0]
    assert out["status"] == 0 and out["format"] == afgpu.FORMAT_XM
    assert out["frames"] == afgpu.MOD_MAX_FRAMES and "cut at AFG_MOD_MAX_FRAMES" in out["message"]
    want = xm.decode_batch(data, limit=200000)
    assert len(want) == 200000
    assert np.array_equal(bits(out["pcm"][:200000]), bits(want))
    assert not np.isnan(out["pcm"]).any()


def test_transcode_writes_the_models_samples(gpu, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = songs(12, 1)[0]
    src, dst = tmp_path / "song.xm", tmp_path / "song.wav"
    src.write_bytes(data)
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "transcode.py"), "--format", "f32", str(src), str(dst)])
    wav = dst.read_bytes()
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    body = np.frombuffer(wav[wav.index(b"data") + 8:], np.float32).reshape(-1, 2)
    total = len(xm.decode_batch(data))
    want, _ = xm.decode_stream(data, [len(body)])
    assert len(body) >= total and np.array_equal(bits(body), bits(want[0]))
