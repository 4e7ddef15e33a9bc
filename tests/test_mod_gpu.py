"""ProTracker MOD on the device: the mixer (afg_mod_render_hip), the stream's reads, the module functions and the batch path,
compared as uint32 with tests/pocketmod_model.py driven by the same reads."""
import os

import numpy as np
import pytest

import afgpu
import flac_bitstream as fb
import mod_bitstream as mb
import pocketmod_model as pm
from test_flac_frontend import make_pcm
from test_stream_gpu import MP3_FIXTURE, flac_expected, qoa_file

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def songs(seed, n=6):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ch = [4, 1, 8, 2, 16, 32, 6, 4][i % 8]
        out.append(mb.random_song(rng, channels=ch, n_patterns=2 if ch <= 8 else 1, instruments=15 if i == 7 else 31,
                                  last_cut=(i % 3 == 2), max_sample=3000))
    return out


def test_render_hip_batch(gpu):
    import torch
    files = songs(1, 8)
    parsed = [afgpu.mod_parse(f) for f in files]
    sng, ticks, segs, plane, frames = afgpu.mod_layout(parsed)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(gpu)
    d_out = torch.full((frames * 2,), float("nan"), dtype=torch.float32, device=gpu)
    afgpu.mod_render(len(files), dev(sng), dev(segs), dev(ticks), dev(plane), d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().reshape(-1, 2)
    for i, f in enumerate(files):
        want, capped, _, _ = pm.decode_batch(f)
        o = int(sng[i]["out_frame"])
        assert not capped and len(want) == parsed[i]["frames"]
        assert np.array_equal(bits(got[o:o + len(want)]), bits(want)), i


@pytest.mark.parametrize("reads", [[1], [7], [1000], [4096], [882 * 6 * 64], [1, 7, 1000, 4096, 33]])
def test_stream_reads(gpu, reads):
    rng = np.random.default_rng(2 + len(reads))
    data = mb.random_song(rng, channels=4, n_patterns=2, max_sample=2000)
    limit = 60000 if reads == [1] else None
    want = pm.decode_stream(data, reads, max_frames=limit)
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    assert not s.isError(), s.errorMessage()
    assert s.getFormat() == afgpu.FORMAT_MOD and s.getNumChannels() == 2 and s.getSamplerate() == 44100.0
    assert s.getLengthInFrames() == afgpu.UNKNOWN_LENGTH
    parts, total, k = [], 0, 0
    while True:
        n = reads[k % len(reads)]
        if limit is not None:
            n = min(n, limit - total)
            if n <= 0:
                break
        buf = np.full(n * 2, np.nan, np.float32)
        got = s.readSamplesFloat(buf)
        k += 1
        if got == 0:
            break
        parts.append(buf[:got * 2].reshape(-1, 2))
        total += got
    got = np.concatenate(parts)
    assert np.array_equal(bits(got), bits(want))
    if limit is None:
        assert s.readSamplesFloat(np.zeros(64, np.float32)) == 0            # after the song has looped
    assert s.tellPosition() == total


def test_module_queries_and_seek(gpu):
    rng = np.random.default_rng(9)
    data = mb.random_song(rng, channels=4, n_patterns=3, jumps=False, max_sample=2000)
    s = afgpu.AudioStream()
    s.openFromMemory(data)
    m = pm.Mod.init(data)
    assert s.isModule() and s.canSeek()
    assert s.countModulePatterns() == m.num_patterns == 3 and s.getModuleLength() == m.length == 3
    assert s.rowsInPattern(0) == 64
    assert (s.tellModulePattern(), s.tellModuleRow()) == (m.pattern, m.line) == (0, 0)
    assert not s.seekPosition(10)                                             # frame seeks are refused on a module
    buf = np.zeros(2 * 5000, np.float32)
    assert s.readSamplesFloat(buf) == len(pm.read(m, 5000))
    assert (s.tellModulePattern(), s.tellModuleRow()) == (m.pattern, m.line)
    assert s.seekPosition(2, 17)                                              # pocketmod_seek
    m.seek(2, 17)
    for n in (3000, 1, 70000, 882):
        want = pm.read(m, n)
        got = np.full(2 * n, np.nan, np.float32)
        k = s.readSamplesFloat(got)
        assert k == len(want) and np.array_equal(bits(got[:2 * k].reshape(-1, 2)), bits(want))
        assert (s.tellModulePattern(), s.tellModuleRow()) == (m.pattern, m.line)
    other = afgpu.AudioStream()
    d, _ = qoa_file(3000, 1, 44100, 3)
    other.openFromMemory(d)
    assert not other.isModule() and other.countModulePatterns() == -1


def mixed_files():
    files, wants = [], []
    for i in range(3):
        pcm = make_pcm(3000 + 517 * i, 1 + i % 2, 16, 30 + i)
        d, _ = fb.encode_file(pcm, 16, 1024, sample_rate=44100)
        files.append(d)
        wants.append(("flac", flac_expected(d)[1]))
    d, w = qoa_file(7000, 2, 44100, 44)
    files.append(d)
    wants.append(("qoa", w))
    mp3 = open(MP3_FIXTURE, "rb").read()
    files.append(mp3)
    wants.append(("mp3", None))
    for f in songs(5, 5):
        files.append(f)
        wants.append(("mod", pm.decode_batch(f)[0]))
    files.insert(3, b"\x00" * 100)
    wants.insert(3, ("junk", None))
    files.insert(6, bytes(np.random.default_rng(3).integers(0, 256, 3000, dtype=np.uint8)))
    wants.insert(6, ("junk", None))
    return files, wants


@pytest.mark.parametrize("mode", ["exact", "tolerance"])
def test_batch_mixes_mod_with_other_formats(gpu, mode, monkeypatch):
    """MOD has one numeric mode: both AFG_NUMERIC settings give the same bits.  The other files of the batch decode as they do
    without the MODs beside them; junk stays refused."""
    if mode == "tolerance":
        monkeypatch.delenv("AFG_NUMERIC", raising=False)
    files, wants = mixed_files()
    out = afgpu.batch_decode(files, n_threads=3)
    alone = afgpu.batch_decode([f for f, (k, _) in zip(files, wants) if k != "mod"], n_threads=3)
    others = iter(alone)
    for item, (kind, want) in zip(out, wants):
        if kind == "junk":
            assert item["status"] != 0 and item["pcm"] is None
            assert item["message"] == "Cannot decode stream: unrecognized encoding."
            next(others)
            continue
        if kind == "mod":
            assert item["status"] == 0 and item["message"] is None and item["format"] == afgpu.FORMAT_MOD
            assert item["channels"] == 2 and item["samplerate"] == 44100.0 and item["frames"] == len(want)
            assert np.array_equal(bits(item["pcm"]), bits(want))
            continue
        ref = next(others)
        assert item["status"] == 0 == ref["status"] and item["frames"] == ref["frames"]
        assert np.array_equal(bits(item["pcm"]), bits(ref["pcm"]))
        if want is not None:
            assert np.array_equal(bits(item["pcm"]), bits(want))


def test_capped_endless_song(gpu):
    data = mb.endless_song(np.random.default_rng(7))
    out = afgpu.batch_decode([data])[0]
    assert out["status"] == 0 and out["format"] == afgpu.FORMAT_MOD
    assert out["frames"] == afgpu.MOD_MAX_FRAMES and "cut at AFG_MOD_MAX_FRAMES" in out["message"]
    # the batch's one read of AFG_MOD_MAX_FRAMES never reaches a pattern boundary: its first frames are the model's
    m = pm.Mod.init(data)
    want = m.render(300000)
    assert len(want) == 300000
    assert np.array_equal(bits(out["pcm"][:300000]), bits(want))


def test_transcode_writes_the_models_samples(gpu, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = songs(12, 1)[0]
    src, dst = tmp_path / "song.mod", tmp_path / "song.wav"
    src.write_bytes(data)
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "transcode.py"), "--format", "f32", str(src), str(dst)])
    wav = dst.read_bytes()
    want = pm.decode_stream(data, [1024])
    assert wav[:4] == b"RIFF" and wav[8:12] == b"WAVE"
    body = wav[wav.index(b"data") + 8:]
    got = np.frombuffer(body, np.float32) if len(body) == want.size * 4 else None
    assert got is not None, "the WAV holds 32-bit float samples"
    assert np.array_equal(got.view(np.uint32), bits(want).ravel())


def test_sharding_over_devices(gpu):
    n = afgpu.device_count()
    files = songs(21, 6)
    one = afgpu.batch_decode(files)
    if n < 2:
        many = afgpu.batch_decode(files, devices=[0, 0])
    else:
        many = afgpu.batch_decode(files, devices="all")
    for a, b in zip(one, many):
        assert a["frames"] == b["frames"] and np.array_equal(bits(a["pcm"]), bits(b["pcm"]))
