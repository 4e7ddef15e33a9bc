"""afg_batch_encode: every item of a batch is byte-equal to the single-file writers (afg_wav_encode[_dithered] for WAV,
the write stream -- itself pinned to afg_qoa_encode_hip by test_write_stream_gpu.py -- for QOA), whatever its neighbours,
the thread count or the chunking are."""
import numpy as np
import pytest

import afgpu

pytestmark = pytest.mark.gpu

A, INC, M = 1103515245, 12345, 1 << 31


def lcg(seed):
    state = [seed % M]

    def rng():
        state[0] = (state[0] * A + INC) % M
        return state[0]
    return rng


def noise(rng, frames, ch):
    return rng.uniform(-1, 1, (frames, ch)).astype(np.float32)


def wav_single(x, rate, fmt, dither, seed):
    if dither == afgpu.DITHER_LCG31 and fmt <= afgpu.WAV_S24LE:
        return afgpu.wav_encode(x, rate, fmt, dither=lcg(seed), rng_max=0x7fffffff)
    return afgpu.wav_encode(x, rate, fmt)


def qoa_single(x, rate):
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_QOA, rate, x.shape[1])
    assert st.writeSamplesFloat(x) == len(x)
    return st.finalizeAndGetEncodedResult()


def wav_inputs(rng, n):
    lengths = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193]
    out = []
    for k in range(n):
        ch = (1, 2, 6, 1024)[k % 4] if k % 16 != 15 else 1024
        if ch == 1024:
            frames = int(rng.integers(0, 6))
        else:
            frames = lengths[k % len(lengths)] if k % 3 == 0 else int(rng.integers(0, 700))
        out.append((noise(rng, frames, ch), (8000, 44100, 48000, 96000)[k % 4]))
    return out


@pytest.mark.parametrize("fmt,dither", [(afgpu.WAV_S8, afgpu.DITHER_OFF), (afgpu.WAV_S16LE, afgpu.DITHER_LCG31), (afgpu.WAV_S24LE, afgpu.DITHER_LCG31),
                                        (afgpu.WAV_S24LE, afgpu.DITHER_OFF), (afgpu.WAV_FP32LE, afgpu.DITHER_LIBC), (afgpu.WAV_FP64LE, afgpu.DITHER_OFF)],
                         ids=["s8", "s16-lcg31", "s24-lcg31", "s24", "fp32", "fp64"])
def test_wav_batch_items_are_the_single_file_writers(gpu, fmt, dither):
    rng = np.random.default_rng(10 + fmt)
    inputs = wav_inputs(rng, 320)
    opts = afgpu.encoding_options(fmt, dither, 4242)
    got = afgpu.batch_encode(inputs, afgpu.FORMAT_WAV, opts)
    assert len(got) == 320
    for k, ((x, rate), it) in enumerate(zip(inputs, got)):
        assert it["status"] == 0 and it["message"] is None, (k, it["message"])
        assert it["bytes"] == wav_single(x, rate, fmt, dither, 4242), (k, x.shape)
    # neither the thread count nor the order of the inputs changes a file
    assert afgpu.batch_encode(inputs, afgpu.FORMAT_WAV, opts, n_threads=1) == got
    assert afgpu.batch_encode(inputs, afgpu.FORMAT_WAV, opts, n_threads=5) == got
    order = rng.permutation(len(inputs))
    shuffled = afgpu.batch_encode([inputs[i] for i in order], afgpu.FORMAT_WAV, opts)
    assert [s["bytes"] for s in shuffled] == [got[i]["bytes"] for i in order]


def test_qoa_batch_items_are_the_stream_writers(gpu):
    rng = np.random.default_rng(20)
    lengths = [0, 1, 19, 20, 21, 5119, 5120, 5121, 10240, 12001]
    inputs = []
    for k in range(304):
        ch = 1 + k % 8
        frames = lengths[(k // 8) % len(lengths)] if k % 5 == 0 else int(rng.integers(0, 900))
        inputs.append((noise(rng, frames, ch) * 0.5, (8000, 44100, 48000)[k % 3]))
    got = afgpu.batch_encode(inputs, afgpu.FORMAT_QOA)
    for k, ((x, rate), it) in enumerate(zip(inputs, got)):
        assert it["status"] == 0, (k, it["message"])
        assert it["bytes"] == qoa_single(x, rate), (k, x.shape)
    assert afgpu.batch_encode(inputs, afgpu.FORMAT_QOA, n_threads=3) == got
    order = rng.permutation(len(inputs))
    shuffled = afgpu.batch_encode([inputs[i] for i in order], afgpu.FORMAT_QOA)
    assert [s["bytes"] for s in shuffled] == [got[i]["bytes"] for i in order]


def test_qoa_batch_items_at_the_encoder_edges(gpu):
    """Floats beyond full scale, a 3-channel item beside a narrow one and an item of no frames (the inputs of
    test_qoa_encode_edges_gpu.py): the stream writer's bytes, which are the oracle's on the int16 that afg.h defines."""
    import oraclelib
    from test_qoa_encode_edges_gpu import c1_streams, float_to_s16, make_pcm
    over, short = c1_streams()
    wide = (make_pcm(np.random.default_rng(404), 50, 3) / 32767.0).astype(np.float32)
    inputs = [(over, 48000), (wide, 44100), (np.zeros((0, 2), np.float32), 8000), (short, 48000)]
    got = afgpu.batch_encode(inputs, afgpu.FORMAT_QOA)
    for k, ((x, rate), it) in enumerate(zip(inputs, got)):
        assert it["status"] == 0, (k, it["message"])
        assert it["bytes"] == qoa_single(x, rate), (k, x.shape)
        assert it["bytes"] == oraclelib.qoa_encode(float_to_s16(x), rate)[0].tobytes(), (k, x.shape)
    assert got[2]["bytes"] == b"qoaf" + bytes(4)


def test_bad_items_keep_to_themselves(gpu):
    rng = np.random.default_rng(30)
    good = (noise(rng, 500, 2), 44100)
    x = noise(rng, 10, 2)
    bad = [dict(pcm=x, frames=10, channels=0, samplerate=44100), dict(pcm=x[:, :1].repeat(1025, 1), frames=10, channels=1025, samplerate=44100),
           dict(pcm=None, frames=10, channels=2, samplerate=44100), dict(pcm=x, frames=10, channels=2, samplerate=-5.0),
           dict(pcm=x, frames=10, channels=2, samplerate=float("nan")), dict(pcm=x, frames=10, channels=2, samplerate=3e9)]
    batch = [good, bad[0], good, bad[1], bad[2], good, bad[3], bad[4], bad[5], good, dict(pcm=None, frames=0, channels=2, samplerate=8000)]
    opts = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LCG31, 1)
    got = afgpu.batch_encode(batch, afgpu.FORMAT_WAV, opts)
    want = wav_single(good[0], 44100, afgpu.WAV_S16LE, afgpu.DITHER_LCG31, 1)
    for k, it in enumerate(got):
        if k in (0, 2, 5, 9):
            assert it["status"] == 0 and it["bytes"] == want
        elif k == 10:                                                             # NULL pcm is fine for no frames
            assert it["status"] == 0 and it["bytes"] == afgpu.wav_encode(np.zeros((0, 2), np.float32), 8000, afgpu.WAV_S16LE)
        else:
            assert it["status"] == -1 and it["message"] and it["bytes"] is None, k
    qbad = [dict(pcm=x, frames=10, channels=9, samplerate=44100), dict(pcm=x, frames=10, channels=2, samplerate=0.2),
            dict(pcm=x, frames=10, channels=2, samplerate=float(1 << 24)), dict(pcm=x, frames=1 << 32, channels=1, samplerate=44100)]
    got = afgpu.batch_encode([good] + qbad + [good], afgpu.FORMAT_QOA)
    assert [it["status"] for it in got] == [0, -1, -1, -1, -1, 0]
    assert got[0]["bytes"] == got[5]["bytes"] == qoa_single(good[0], 44100)
    assert afgpu.batch_encode([], afgpu.FORMAT_WAV, opts) == []


def test_libc_dither_is_refused_for_integer_formats(gpu):
    rng = np.random.default_rng(31)
    with pytest.raises(afgpu.AfgError, match="unsupported"):
        afgpu.batch_encode([(noise(rng, 10, 2), 44100)], afgpu.FORMAT_WAV, afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LIBC))
    with pytest.raises(afgpu.AfgError, match="unsupported"):
        afgpu.batch_encode([(noise(rng, 10, 2), 44100)], afgpu.FORMAT_MP3)


@pytest.mark.parametrize("fmt", [afgpu.WAV_S16LE, afgpu.WAV_S24LE], ids=["s16", "s24"])
def test_a_file_longer_than_a_chunk_keeps_its_dither_position(gpu, fmt):
    """A chunk is 2^23 samples: this file is cut twice, between neighbours that move the cuts off its start.  The expected
    bytes come from the float64 model of test_wav_encode_gpu.py (the host writer's callback is too slow for 2 x 10^7 draws);
    the head of the file is also checked against the host writer."""
    from test_wav_encode_gpu import model
    rng = np.random.default_rng(32)
    big = noise(rng, (1 << 23) + 70001, 2)
    inputs = [(noise(rng, 3001, 1), 8000), (big, 44100), (noise(rng, 77, 2), 8000)]
    opts = afgpu.encoding_options(fmt, afgpu.DITHER_LCG31, 77)
    got = afgpu.batch_encode(inputs, afgpu.FORMAT_WAV, opts)
    alone = afgpu.batch_encode([inputs[1]], afgpu.FORMAT_WAV, opts)[0]["bytes"]
    assert got[1]["bytes"] == alone
    body = np.frombuffer(alone, np.uint8)[44:]
    want = model(big.reshape(-1), fmt, True, seed=77)
    assert body.size == want.size and np.array_equal(body, want)
    head = 1 << 15
    assert alone[:44] == afgpu.wav_encode(big, 44100, fmt)[:44]
    b = afgpu.WAV_FORMAT_BYTES[fmt]
    assert alone[44:44 + head * 2 * b] == wav_single(big[:head], 44100, fmt, afgpu.DITHER_LCG31, 77)[44:]
    for k in (0, 2):
        assert got[k]["bytes"] == wav_single(inputs[k][0], 8000, fmt, afgpu.DITHER_LCG31, 77)


def test_flac_to_wav_round_trip_returns_the_first_decode(gpu):
    import flac_bitstream
    rng = np.random.default_rng(33)
    files = []
    for k in range(12):
        ch = 1 + k % 2
        pcm = (rng.standard_normal((2000 + 517 * k, ch)) * 3000).astype(np.int64).clip(-32768, 32767)
        files.append(flac_bitstream.encode_file(pcm, 16, 1152, sample_rate=(44100, 48000)[k % 2])[0])
    first = afgpu.batch_decode(files)
    assert all(it["status"] == 0 and it["format"] == afgpu.FORMAT_FLAC for it in first)
    enc = afgpu.batch_encode([(it["pcm"], it["samplerate"]) for it in first], afgpu.FORMAT_WAV,
                             afgpu.encoding_options(afgpu.WAV_FP32LE, afgpu.DITHER_OFF))
    assert all(it["status"] == 0 for it in enc)
    second = afgpu.batch_decode([it["bytes"] for it in enc])
    for a, b in zip(first, second):
        assert b["status"] == 0 and b["format"] == afgpu.FORMAT_WAV
        assert b["channels"] == a["channels"] and b["samplerate"] == a["samplerate"] and b["frames"] == a["frames"]
        assert np.array_equal(a["pcm"].view(np.uint32), b["pcm"].view(np.uint32))
