"""afg_pcm_pack_hip (csrc/pcm_pack.hip), the packer of the batch decode stages: spans at any float and any byte.  Expected
bytes come from the host writer (afgpu.wav_encode, with the 31-bit generator as its callback for dither) over the test's
own clamp of the samples: NaN to 0, then [-1, 1].  Everything compares bit for bit; 0xA5 guard bytes around every span must
come back unchanged."""
import numpy as np
import pytest
import torch

import afgpu
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

A, INC, M = 1103515245, 12345, 1 << 31
BYTES = {afgpu.WAV_S8: 1, afgpu.WAV_S16LE: 2, afgpu.WAV_S24LE: 3}
FORMATS = [afgpu.WAV_S8, afgpu.WAV_S16LE, afgpu.WAV_S24LE]
NAMES = {afgpu.WAV_S8: "s8", afgpu.WAV_S16LE: "s16", afgpu.WAV_S24LE: "s24"}
COUNTS = [0, 1, 2, 3, 15, 16, 17, 4095, 4096, 4097, 8193]
IN_MODS = [0, 1, 2, 3]
OUT_MODS = [0, 1, 2, 3, 5, 15]
GUARD = 0xA5


def lcg_from(state):
    st = [state % M]

    def rng():
        st[0] = (st[0] * A + INC) % M
        return st[0]
    return rng


def clamp(x):
    x = np.asarray(x, np.float32)
    return np.clip(np.where(np.isnan(x), np.float32(0), x), -1, 1).astype(np.float32)


def expected(x, fmt, dither, seed=0, draw0=0):
    """the host writer's sample bytes for a run of a file that starts draw0 draws into the file's generator"""
    x = clamp(x)
    if dither:
        data = afgpu.wav_encode(x, 8000, fmt, dither=lcg_from(afgpu.lcg31_jump(seed, draw0)), rng_max=0x7fffffff)
    else:
        data = afgpu.wav_encode(x, 8000, fmt)
    body = np.frombuffer(data, np.uint8)[44:]
    assert body.size == x.size * BYTES[fmt]
    return body


def signal(n, seed):
    rng = np.random.default_rng(seed)
    return (0.7 * np.sin(0.05 * np.arange(n)) + 0.29 * rng.uniform(-1, 1, n)).astype(np.float32)


def launch(dev, spans, plane, out_bytes, in_floats=None, out_limit=None):
    """one launch over `spans` (any order); returns the output plane, which started as guard bytes"""
    spans = np.ascontiguousarray(spans)
    tiles = afgpu.pcm_pack_layout(spans)
    d_spans = torch.from_numpy(spans.view(np.uint8).copy()).to(dev)
    d_in = torch.from_numpy(np.ascontiguousarray(plane, np.float32)).to(dev)
    d_out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device=dev)
    afgpu.pcm_pack(len(spans), d_spans, tiles, d_in, plane.size if in_floats is None else in_floats, d_out,
                   out_bytes if out_limit is None else out_limit)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def span(in_off, out_off, count, fmt, dither=0, seed=0, draw0=0):
    sp = np.zeros(1, afgpu.PCM_PACK_SPAN_DTYPE)
    sp["in_off"], sp["out_off"], sp["count"], sp["draw0"] = in_off, out_off, count, draw0
    sp["seed"], sp["format"], sp["dither"] = seed, fmt, dither
    return sp


def check(got, pieces):
    """pieces: (out_off, expected bytes); every byte outside them is a guard byte"""
    want = np.full(got.size, GUARD, np.uint8)
    for off, body in pieces:
        want[off:off + body.size] = body
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("dither", [0, 1], ids=["off", "lcg31"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_single_spans(gpu, fmt, dither):
    """every count twice, walking through the input and output alignments"""
    B = BYTES[fmt]
    spans, pieces, planes = [], [], []
    in_at, out_at, k = 0, 32, fmt * 5 + dither * 3
    for count in COUNTS:
        for _ in range(2):
            im, om = IN_MODS[k % 4], OUT_MODS[(k // 4 + k) % 6]
            k += 1
            in_off = ((in_at + 3) & ~3) + im
            out_off = ((out_at + 15) & ~15) + 16 + om                # at least 16 guard bytes in front
            x = signal(count, 100 + k)
            seed = 1000 + k
            planes.append((in_off, x))
            spans.append(span(in_off, out_off, count, fmt, dither, seed))
            pieces.append((out_off, expected(x, fmt, dither, seed)))
            in_at, out_at = in_off + count + 1, out_off + count * B
    plane = np.full(in_at + 8, np.nan, np.float32)                   # (a float read from outside a span would show)
    for off, x in planes:
        plane[off:off + x.size] = x
    got = launch(gpu, np.concatenate(spans), plane, out_at + 64)
    check(got, pieces)


def test_spans_that_abut_byte_to_byte(gpu):
    """a dozen spans in mixed formats, outputs back to back from an odd byte on, records in shuffled order"""
    rng = np.random.default_rng(11)
    counts = [5, 4097, 1, 17, 300, 4096, 33, 7, 2, 1000, 4099, 3, 0, 21]
    spans, pieces, planes = [], [], []
    in_at, out_at = 3, 37
    for k, count in enumerate(counts):
        fmt, dither = FORMATS[(k * 2 + k // 3) % 3], k % 2
        x = signal(count, 200 + k)
        planes.append((in_at, x))
        spans.append(span(in_at, out_at, count, fmt, dither, 77 + k))
        pieces.append((out_at, expected(x, fmt, dither, 77 + k)))
        in_at += count + int(rng.integers(0, 3))
        out_at += count * BYTES[fmt]                                 # no gap
        if k == 8:
            out_at += 5                                              # one gap: guard bytes between two spans
    plane = np.full(in_at + 4, np.nan, np.float32)
    for off, x in planes:
        plane[off:off + x.size] = x
    order = rng.permutation(len(spans))
    got = launch(gpu, np.concatenate([spans[i] for i in order]), plane, out_at + 41)
    check(got, pieces)


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_dither_position(gpu, fmt):
    B = BYTES[fmt]
    n, seed = 9001, 0x2545F491
    x = signal(n, 31)
    plane = np.concatenate([np.full(1, np.nan, np.float32), x])
    far = 2 * ((1 << 32) + 1)                                        # an odd multiple of 2 near 2^33
    for draw0 in (0, far):
        got = launch(gpu, span(1, 3, n, fmt, 1, seed, draw0), plane, 3 + n * B + 20)
        check(got, [(3, expected(x, fmt, 1, seed, draw0))])
    # one file in three spans whose draws continue = the same file in one span
    a, b = 4097, 4097 + 1234
    whole = expected(x, fmt, 1, seed)
    three = np.concatenate([span(1, 7, a, fmt, 1, seed, 0), span(1 + b, 7 + b * B, n - b, fmt, 1, seed, 2 * b),
                            span(1 + a, 7 + a * B, b - a, fmt, 1, seed, 2 * a)])
    got3 = launch(gpu, three, plane, 7 + n * B + 9)
    got1 = launch(gpu, span(1, 7, n, fmt, 1, seed, 0), plane, 7 + n * B + 9)
    assert (got3 == got1).all()
    check(got3, [(7, whole)])


def special_values():
    k = np.arange(-40, 40, dtype=np.float64)
    half = ((k + 0.5) / 32767.0).astype(np.float32)                  # the half steps of s16 ...
    edge = ((np.array([-32767, -32766, 32766, 32767], np.float64) - 0.5) / 32767.0).astype(np.float32)
    steps = np.concatenate([half, edge])
    steps = np.concatenate([steps, np.nextafter(steps, np.float32(2)), np.nextafter(steps, np.float32(-2))])   # ... +- 1 ulp
    tiny = np.array([1, 0x7fffff, 0x80000001, 0x807fffff], np.uint32).view(np.float32)     # denormals
    other = np.array([1, -1, 1.0000001, -1.0000001, 3.5, -3.5, np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, 0.5, -0.5], np.float32)
    nan_payload = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32).view(np.float32)
    return np.concatenate([steps, tiny, other, nan_payload]).astype(np.float32)


@pytest.mark.parametrize("dither", [0, 1], ids=["off", "lcg31"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_input_values(gpu, fmt, dither):
    x = special_values()
    assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) > 1).any()
    plane = np.concatenate([np.zeros(2, np.float32), x])
    got = launch(gpu, span(2, 1, x.size, fmt, dither, 99), plane, 1 + x.size * BYTES[fmt] + 16)
    check(got, [(1, expected(x, fmt, dither, 99))])
    # and the same values through the vector path of a full tile
    big = np.resize(x, 4096 + 50)
    got = launch(gpu, span(0, 16, big.size, fmt, dither, 5), big, 16 + big.size * BYTES[fmt] + 16)
    check(got, [(16, expected(big, fmt, dither, 5))])


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_spans_that_leave_the_planes_are_not_touched(gpu, fmt):
    B = BYTES[fmt]
    n = 5000
    x = signal(3 * n, 41)
    # the middle span reaches one float past in_floats; its neighbours are written
    spans = np.concatenate([span(0, 5, n, fmt), span(2 * n + 1, 5 + n * B + 3, n, fmt), span(n, 5 + 2 * n * B + 9, n, fmt, 1, 8)])
    got = launch(gpu, spans, x, 5 + 3 * n * B + 40)
    check(got, [(5, expected(x[:n], fmt, 0)), (5 + 2 * n * B + 9, expected(x[n:2 * n], fmt, 1, 8))])
    # the last span reaches one byte past out_bytes (the buffer itself is longer: nothing behind the limit may change)
    limit = 5 + 3 * n * B + 12 - 1
    spans = np.concatenate([span(0, 5, n, fmt, 1, 3), span(n, 5 + n * B + 3, n, fmt), span(2 * n, 5 + 2 * n * B + 12, n, fmt)])
    got = launch(gpu, spans, x, limit + 64, out_limit=limit)
    check(got, [(5, expected(x[:n], fmt, 1, 3)), (5 + n * B + 3, expected(x[n:2 * n], fmt, 0))])
    # offsets and counts so large that their products wrap, and a format the kernel does not pack
    spans = np.concatenate([span(1 << 63, 0, n, fmt), span(0, 5, n, fmt), span(0, (1 << 64) - 8, n, fmt), span(n, 5 + n * B, 16, afgpu.WAV_FP32LE)])
    got = launch(gpu, spans, x, 5 + n * B + 100)
    check(got, [(5, expected(x[:n], fmt, 0))])


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_spans_without_tiles(gpu, case):
    """1, 2 and 5 spans, with spans of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    fmt, B = afgpu.WAV_S16LE, 2
    spans, pieces, plane, out_at = [], [], [], 16
    for k, count in enumerate(record_lengths(4096)[case]):
        x = signal(count, 900 + k)
        spans.append(span(sum(p.size for p in plane), out_at, count, fmt, 1, 77 + k))
        pieces.append((out_at, expected(x, fmt, 1, 77 + k)))
        plane.append(x)
        out_at += count * B + 16
    got = launch(gpu, np.concatenate(spans), np.concatenate(plane + [np.full(4, np.nan, np.float32)]), out_at + 16)
    check(got, pieces)
