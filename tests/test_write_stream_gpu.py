"""The writing half of AudioStream (afg_open_to_buffer / afg_open_to_memory, afg_write_samples_*, afg_finalize_*): the
bytes do not depend on how the signal is cut into writes, and they are the single-call writers' bytes -- afg_wav_encode /
afg_wav_encode_dithered for WAV, afg_qoa_encode_hip through its existing binding for QOA."""
import numpy as np
import pytest

import afgpu

pytestmark = pytest.mark.gpu

A, INC, M = 1103515245, 12345, 1 << 31
CHUNKS = [1, 7, 1024, 5119, 5120, 5121, 300001]
FRAMES, CH, RATE = 41000, 2, 48000
WAV_CASES = [(fmt, dither) for fmt in range(5) for dither in (afgpu.DITHER_OFF, afgpu.DITHER_LCG31)]


def signal(frames=FRAMES, ch=CH, seed=1):
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None]
    x = 0.6 * np.sin(0.013 * (1 + np.arange(ch))[None, :] * t) + 0.2 * rng.uniform(-1, 1, (frames, ch))
    return np.clip(x, -1, 1).astype(np.float32)


def lcg(seed):
    state = [seed % M]

    def rng():
        state[0] = (state[0] * A + INC) % M
        return state[0]
    return rng


def wav_whole(x, rate, fmt, dither, seed):
    if dither == afgpu.DITHER_LCG31 and fmt <= afgpu.WAV_S24LE:
        return afgpu.wav_encode(x, rate, fmt, dither=lcg(seed), rng_max=0x7fffffff)
    return afgpu.wav_encode(x, rate, fmt)


def qoa_whole(gpu, x, rate):
    import torch
    recs, n_in, n_out = afgpu.qoa_encode_layout([x.shape], rate)
    d_out = torch.zeros(max(n_out, 8), dtype=torch.uint8, device=gpu)
    afgpu.qoa_encode(1, torch.from_numpy(recs.view(np.uint8).copy()).to(gpu), d_out,
                     d_pcm_f32=torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(gpu))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:afgpu.qoa_encoded_size(x.shape[0], x.shape[1])].tobytes()


def write_in_chunks(fmt, x, rate, chunk, options=None, double=False):
    st = afgpu.AudioStream()
    st.openToBuffer(fmt, rate, x.shape[1], options)
    assert not st.isError(), st.errorMessage()
    assert st.isOpenForWriting() and not st.isOpenForReading()
    assert st.getFormat() == fmt and st.getNumChannels() == x.shape[1]
    for at in range(0, len(x), chunk):
        part = x[at:at + chunk]
        n = st.writeSamplesDouble(part.astype(np.float64)) if double else st.writeSamplesFloat(part)
        assert n == len(part) and not st.isError()
    assert st.finalizeEncoding() is True                                          # a complete WAV reports success here
    data = st.finalizeAndGetEncodedResult()
    assert data is not None and data == st.finalizeAndGetEncodedResult()          # repeatable
    assert st.writeSamplesFloat(x[:1]) == 0 and st.isError()                      # a write after finalize
    assert st.errorMessage() == "Encoder encountered an error"
    st.cleanUp()
    return data


def reopen(data):
    st = afgpu.AudioStream()
    st.openFromMemory(data)
    assert not st.isError(), st.errorMessage()
    out = np.zeros(max(1, st.getLengthInFrames()) * st.getNumChannels(), np.float32)
    got = st.readSamplesFloat(out)
    return st, out.reshape(-1, st.getNumChannels())[:got]


@pytest.mark.parametrize("fmt,dither", WAV_CASES, ids=[f"{'s8 s16 s24 fp32 fp64'.split()[f]}-{'off' if d == 0 else 'lcg31'}" for f, d in WAV_CASES])
def test_wav_stream_bytes_are_the_single_call_writers(gpu, fmt, dither):
    x = signal()
    seed = 99
    opts = afgpu.encoding_options(fmt, dither, seed)
    want = wav_whole(x, RATE, fmt, dither, seed)
    one = write_in_chunks(afgpu.FORMAT_WAV, x, RATE, len(x), opts)
    assert one == want
    for chunk in CHUNKS:
        assert write_in_chunks(afgpu.FORMAT_WAV, x, RATE, chunk, opts) == want, chunk
    assert write_in_chunks(afgpu.FORMAT_WAV, x, RATE, 5121, opts, double=True) == want      # doubles that are floats
    st, pcm = reopen(one)
    assert st.getFormat() == afgpu.FORMAT_WAV and st.getNumChannels() == CH and st.getSamplerate() == RATE
    assert st.getLengthInFrames() == FRAMES and len(pcm) == FRAMES
    if fmt == afgpu.WAV_S16LE and dither == afgpu.DITHER_OFF:
        s = (32768.5 + x.astype(np.float64) * 32767.0).astype(np.int64) - 32768
        assert np.array_equal(pcm, (s / 32767.0).astype(np.float32))
    if fmt in (afgpu.WAV_FP32LE, afgpu.WAV_FP64LE):
        assert np.array_equal(pcm.view(np.uint32), x.view(np.uint32))


def test_wav_stream_longer_than_its_queue(gpu):
    """More than 2^18 samples: several flushes, the dither position carried across them."""
    x = signal(300001, 2, seed=3)
    opts = afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LCG31, 5)
    one = write_in_chunks(afgpu.FORMAT_WAV, x, 44100, len(x), opts)
    for chunk in (5121, 100000):
        assert write_in_chunks(afgpu.FORMAT_WAV, x, 44100, chunk, opts) == one
    head = 1 << 16                                                                # the host writer's callback is slow: its first 2^17 samples
    want = afgpu.wav_encode(x[:head], 44100, afgpu.WAV_S16LE, dither=lcg(5), rng_max=0x7fffffff)
    assert one[44:44 + head * 4] == want[44:]
    plain = write_in_chunks(afgpu.FORMAT_WAV, x, 44100, 77777, afgpu.encoding_options(afgpu.WAV_S24LE, afgpu.DITHER_OFF))
    assert plain == afgpu.wav_encode(x, 44100, afgpu.WAV_S24LE)


def test_default_options_are_fp32(gpu):
    x = signal(3000, 3)
    assert write_in_chunks(afgpu.FORMAT_WAV, x, 22050, 1000) == afgpu.wav_encode(x, 22050, afgpu.WAV_FP32LE)


def test_libc_dither_stays_on_the_host_writer(gpu):
    """AFG_DITHER_LIBC draws from rand(): the bytes are not reproducible, but every sample is within the dither's reach of
    the undithered one."""
    x = signal(5000, 2)
    data = write_in_chunks(afgpu.FORMAT_WAV, x, 44100, 1999, afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_LIBC))
    plain = afgpu.wav_encode(x, 44100, afgpu.WAV_S16LE)
    assert len(data) == len(plain) and data[:44] == plain[:44]
    a = np.frombuffer(data[44:], "<i2").astype(int)
    b = np.frombuffer(plain[44:], "<i2").astype(int)
    assert np.abs(a - b).max() <= 1


def test_doubles_to_fp64_keep_their_bits(gpu):
    rng = np.random.default_rng(8)
    d = rng.uniform(-1, 1, (9000, 2))                                             # not representable as floats
    f = signal(700, 2)
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_WAV, 96000, 2, afgpu.encoding_options(afgpu.WAV_FP64LE, afgpu.DITHER_OFF))
    assert st.writeSamplesDouble(d[:4000]) == 4000
    assert st.writeSamplesFloat(f) == 700                                         # floats in between are widened, in order
    assert st.writeSamplesDouble(d[4000:]) == 5000
    data = st.finalizeAndGetEncodedResult()
    body = np.frombuffer(data[44:], "<f8").reshape(-1, 2)
    want = np.concatenate([d[:4000], f.astype(np.float64), d[4000:]])
    assert np.array_equal(body.view(np.uint64), want.view(np.uint64))
    assert int.from_bytes(data[40:44], "little") == want.size * 8
    # to any other target the doubles are narrowed first (stream.d:886-894)
    got = write_in_chunks(afgpu.FORMAT_WAV, d.astype(np.float32), 96000, 1234, afgpu.encoding_options(afgpu.WAV_S24LE, 0), double=False)
    st2 = afgpu.AudioStream()
    st2.openToBuffer(afgpu.FORMAT_WAV, 96000, 2, afgpu.encoding_options(afgpu.WAV_S24LE, afgpu.DITHER_OFF))
    assert st2.writeSamplesDouble(d) == len(d)
    assert st2.finalizeAndGetEncodedResult() == got


@pytest.mark.parametrize("ch", [1, 2, 5, 8])
def test_qoa_stream_bytes_are_the_encoder_entrys(gpu, ch):
    x = signal(5120 * 3 + 777, ch, seed=ch)
    want = qoa_whole(gpu, x, 44100)
    for chunk in [len(x)] + CHUNKS:
        assert write_in_chunks(afgpu.FORMAT_QOA, x, 44100, chunk) == want, chunk
    # doubles: converted in double, no narrowing (qoa.d:632-634)
    d = x.astype(np.float64) * 0.999999999
    s = ((32768.5 + d * 32767.0).astype(np.int64) - 32768).astype(np.int16)
    import torch
    recs, _, n_out = afgpu.qoa_encode_layout([s.shape], 44100)
    d_out = torch.zeros(n_out, dtype=torch.uint8, device=gpu)
    afgpu.qoa_encode(1, torch.from_numpy(recs.view(np.uint8).copy()).to(gpu), d_out, d_pcm_i16=torch.from_numpy(s.reshape(-1)).to(gpu))
    torch.cuda.synchronize()
    assert write_in_chunks(afgpu.FORMAT_QOA, d, 44100, 5121, double=True) == d_out.cpu().numpy()[:afgpu.qoa_encoded_size(*s.shape)].tobytes()
    st, pcm = reopen(want)
    assert st.getFormat() == afgpu.FORMAT_QOA and st.getNumChannels() == ch and st.getSamplerate() == 44100
    assert st.getLengthInFrames() == len(x) and len(pcm) == len(x)
    import oraclelib
    s16 = ((32768.5 + x.astype(np.float64) * 32767.0).astype(np.int64) - 32768).astype(np.int16)
    ref_bytes, recon = oraclelib.qoa_encode(s16, 44100)
    assert bytes(ref_bytes) == want
    assert np.array_equal(pcm, recon.astype(np.float32) * np.float32(1.0 / 32767.0))


def test_open_to_memory_exact_fit_and_one_byte_less(gpu):
    x = signal(6000, 2)
    for fmt, opts, want in [(afgpu.FORMAT_WAV, afgpu.encoding_options(afgpu.WAV_S24LE, afgpu.DITHER_LCG31, 3),
                             afgpu.wav_encode(x, 44100, afgpu.WAV_S24LE, dither=lcg(3), rng_max=0x7fffffff)),
                            (afgpu.FORMAT_QOA, None, qoa_whole(gpu, x, 44100))]:
        size = len(want)
        buf = np.full(size + 64, 0xCD, np.uint8)
        st = afgpu.AudioStream()
        st.openToMemory(buf[:size], fmt, 44100, 2, opts)
        assert not st.isError()
        for at in range(0, len(x), 2500):
            assert st.writeSamplesFloat(x[at:at + 2500]) == len(x[at:at + 2500])
        assert st.finalizeEncoding() and not st.isError()
        assert buf[:size].tobytes() == want and (buf[size:] == 0xCD).all()
        assert st.finalizeAndGetEncodedResult() is None                           # buffer streams only
        st.cleanUp()
        buf[:] = 0xCD
        st = afgpu.AudioStream()
        st.openToMemory(buf[:size - 1], fmt, 44100, 2, opts)
        assert not st.isError()
        wrote = [st.writeSamplesFloat(x[at:at + 2500]) for at in range(0, len(x), 2500)]
        done = st.finalizeEncoding()
        assert st.isError() and st.errorMessage() == "Encoder encountered an error" and not done
        if fmt == afgpu.FORMAT_WAV:
            assert wrote == [2500, 2500, 0]                                       # the write that would pass the end
        assert (buf[size - 1:] == 0xCD).all()
        st.cleanUp()
    tiny = np.zeros(43, np.uint8)
    st = afgpu.AudioStream()
    st.openToMemory(tiny, afgpu.FORMAT_WAV, 44100, 2)                             # not even the header fits
    assert st.isError() and st.errorMessage() == "Encoder encountered an error"


def test_stream_state(gpu):
    for rate, want in [(44100.4, 44100), (44100.5, 44101), (7999.5, 8000)]:
        st = afgpu.AudioStream()
        st.openToBuffer(afgpu.FORMAT_WAV, np.float32(rate), 1, afgpu.encoding_options(afgpu.WAV_S8, afgpu.DITHER_OFF))
        assert not st.isError() and st.getSamplerate() == float(np.float32(rate))
        data = st.finalizeAndGetEncodedResult()
        assert len(data) == 44 and int.from_bytes(data[24:28], "little") == want  # stream.d:1852
        assert data == afgpu.wav_encode(np.zeros((0, 1), np.float32), want, afgpu.WAV_S8)
        st2 = afgpu.AudioStream()
        st2.openToBuffer(afgpu.FORMAT_QOA, np.float32(rate), 1)
        st2.writeSamplesFloat(np.zeros((30, 1), np.float32))
        q = st2.finalizeAndGetEncodedResult()
        assert int.from_bytes(q[9:12], "big") == want
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_WAV, 8000, 0)                                    # wav.d:400 lets no channels through
    assert not st.isError() and len(st.finalizeAndGetEncodedResult()) == 44
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_WAV, 8000, 1024, afgpu.encoding_options(afgpu.WAV_S16LE, afgpu.DITHER_OFF))
    x = signal(10, 1024)
    assert st.writeSamplesFloat(x) == 10
    assert st.finalizeAndGetEncodedResult() == afgpu.wav_encode(x, 8000, afgpu.WAV_S16LE)
    # a write stream does not read or seek
    st = afgpu.AudioStream()
    st.openToBuffer(afgpu.FORMAT_WAV, 8000, 2)
    assert st.readSamplesFloat(np.zeros(8, np.float32)) == 0 and not st.seekPosition(0) and not st.canSeek() and not st.isError()
    rd = afgpu.AudioStream()
    rd.openFromMemory(afgpu.wav_encode(signal(10, 2), 8000, afgpu.WAV_S16LE))
    assert rd.isOpenForReading() and not rd.isOpenForWriting()
    assert rd.writeSamplesFloat(np.zeros((1, 2), np.float32)) == 0 and not rd.finalizeEncoding()
