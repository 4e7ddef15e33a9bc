"""afg_wav_pack_hip (csrc/wav_encode.hip): float32 to WAV sample bytes on the device, bit for bit against
  - the library's host writer (afg_wav_encode; afg_wav_encode_dithered with a callback of the same 31-bit generator), and
  - a numpy float64 restatement of TPDFDither.process (wav.d:679-700) and writeSamples (wav.d:482-527) for large inputs.
The integer formats are defined on [-1, 1] only (the reference asserts), so every input set stays inside."""
import numpy as np
import pytest

import afgpu
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

A, INC, M = 1103515245, 12345, 1 << 31
SCALE = {afgpu.WAV_S8: 127, afgpu.WAV_S16LE: 32767, afgpu.WAV_S24LE: 8388607}
BYTES = afgpu.WAV_FORMAT_BYTES
SEED = 0x1234ABC


def jump(n):
    """(a, c) of n generator steps: x -> (a x + c) mod 2^31."""
    an = pow(A, n, (A - 1) * M)
    return an % M, (INC * ((an - 1) // (A - 1))) % M


def draws(seed, first, n):
    """Draws first .. first + n - 1 (0-based) of the generator started at `seed`, as float64."""
    out = np.empty(n, np.uint64)
    if n == 0:
        return out.astype(np.float64)
    a, c = jump(first + 1)
    out[0] = (a * (seed % M) + c) % M
    filled = 1
    while filled < n:
        m = min(filled, n - filled)
        a, c = jump(filled)
        out[filled:filled + m] = (np.uint64(a) * out[:m] + np.uint64(c)) % np.uint64(M)
        filled += m
    return out.astype(np.float64)


def model(x, fmt, dither, seed=SEED, draw0=0):
    """The bytes the reference's arithmetic gives, in float64, one operation per numpy call (no fused operations)."""
    x = x.astype(np.float64)
    if fmt == afgpu.WAV_FP32LE:
        return x.astype(np.float32).view(np.uint8)
    if fmt == afgpu.WAV_FP64LE:
        return x.view(np.uint8)
    scale = float(SCALE[fmt])
    if dither:
        r = draws(seed, draw0, 2 * x.size)
        x = x * scale
        x = x + 0.3125
        x = x + 0.25 * (r[0::2] / 2147483647.0)
        x = x + 0.125 * (r[1::2] / 2147483647.0)
        x = np.floor(x)
        x = x / scale
        x = np.clip(x, -1.0, 1.0)
    off = float(SCALE[fmt] + 1)
    v = np.trunc((off + 0.5) + x * scale).astype(np.int64)
    if fmt == afgpu.WAV_S8:
        return (v & 0xff).astype(np.uint8)
    v = v - int(off)
    if fmt == afgpu.WAV_S16LE:
        return v.astype("<i2").view(np.uint8)
    w = (v & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(w[:, :3]).reshape(-1)


def host_writer(x, fmt, dither, seed=SEED):
    """The sample bytes of the library's own host writer."""
    if not dither:
        return np.frombuffer(afgpu.wav_encode(x[:, None], 44100, fmt), np.uint8)[44:]
    state = [seed % M]

    def rng():
        state[0] = (state[0] * A + INC) % M
        return state[0]
    return np.frombuffer(afgpu.wav_encode(x[:, None], 44100, fmt, dither=rng, rng_max=0x7fffffff), np.uint8)[44:]


def pack(gpu, pieces, in_floats=None, out_bytes=None, canary=None):
    """pieces: dicts(x=float32 array, fmt=, dither=, seed=, draw0=, [in_off=, out_off=, count=]); laid out back to back on the
    alignments the header asks for unless offsets are given.  Returns (whole output plane, spans)."""
    import torch
    spans = np.zeros(len(pieces), afgpu.WAV_PACK_SPAN_DTYPE)
    in_at = out_at = 0
    plane = []
    for k, p in enumerate(pieces):
        x = np.ascontiguousarray(p["x"], np.float32)
        spans[k]["in_off"] = p.get("in_off", in_at)
        spans[k]["out_off"] = p.get("out_off", out_at)
        spans[k]["count"] = p.get("count", x.size)
        spans[k]["draw0"] = p.get("draw0", 0)
        spans[k]["seed"] = p.get("seed", SEED)
        spans[k]["format"] = p["fmt"]
        spans[k]["dither"] = 1 if p.get("dither") else 0
        plane.append(x)
        pad = (-x.size) % 4
        if pad:
            plane.append(np.zeros(pad, np.float32))
        in_at += x.size + pad
        out_at += (x.size * BYTES[min(p["fmt"], 4)] + 15) & ~15
    flat = np.concatenate(plane) if plane else np.zeros(4, np.float32)
    in_floats = flat.size if in_floats is None else in_floats
    out_bytes = max(out_at, 16) if out_bytes is None else out_bytes
    tiles = afgpu.wav_pack_layout(spans)
    d_in = torch.from_numpy(flat).to(gpu)
    d_out = torch.full((max(out_at, out_bytes, 16),), 0xA5 if canary is None else canary, dtype=torch.uint8, device=gpu)
    d_spans = torch.from_numpy(spans.view(np.uint8).copy()).to(gpu)
    afgpu.wav_pack(len(spans), d_spans, tiles, d_in, in_floats, d_out, out_bytes)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), spans


def pack_one(gpu, x, fmt, dither, seed=SEED, draw0=0):
    out, _ = pack(gpu, [dict(x=x, fmt=fmt, dither=dither, seed=seed, draw0=draw0)])
    return out[:x.size * BYTES[fmt]]


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert got.size == want.size and bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:4]}"


def f32_neighbours(v64):
    """float32 values nearest to v64, one ulp below and one above, kept inside [-1, 1]."""
    c = v64.astype(np.float32)
    lo = np.nextafter(c, np.float32(-2))
    hi = np.nextafter(c, np.float32(2))
    return np.clip(np.concatenate([c, lo, hi]), np.float32(-1), np.float32(1))


def edge_values():
    tiny = np.array([1, 2, 0x007fffff, 0x00800000], np.uint32)
    d = np.concatenate([tiny, tiny | np.uint32(0x80000000)]).view(np.float32)
    return np.concatenate([np.array([1.0, -1.0, 0.0, -0.0], np.float32), d])


def grid_chunks(fmt, chunk=1 << 22):
    """The stated input set of an integer format, in chunks: every k / scale and every (k + 0.5) / scale with their float32
    neighbours, the edge values, and 2^24 seeded uniform values."""
    s = SCALE[fmt]
    for k0 in range(-s, s + 1, chunk):
        k = np.arange(k0, min(k0 + chunk, s + 1), dtype=np.float64)
        yield "steps", f32_neighbours(k / s)
    for k0 in range(-s, s, chunk):
        k = np.arange(k0, min(k0 + chunk, s), dtype=np.float64)
        yield "half steps", f32_neighbours((k + 0.5) / s)
    yield "edges", edge_values()
    rng = np.random.default_rng(2024 + fmt)
    for _ in range(4):
        yield "uniform", rng.uniform(-1.0, 1.0, 1 << 22).astype(np.float32)


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "lcg31"])
@pytest.mark.parametrize("fmt", [afgpu.WAV_S8, afgpu.WAV_S16LE, afgpu.WAV_S24LE], ids=["s8", "s16", "s24"])
def test_integer_formats_match_the_float64_model_on_the_whole_grid(gpu, fmt, dither):
    total = 0
    for what, x in grid_chunks(fmt):
        same(pack_one(gpu, x, fmt, dither), model(x, fmt, dither), f"{what} ({x.size} samples)")
        total += x.size
    assert total >= (1 << 24) + 6 * SCALE[fmt]


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "lcg31"])
@pytest.mark.parametrize("fmt", [afgpu.WAV_S8, afgpu.WAV_S16LE, afgpu.WAV_S24LE], ids=["s8", "s16", "s24"])
def test_integer_formats_match_the_host_writer(gpu, fmt, dither):
    """<= 2^17 samples: the dithered host writer draws through a Python callback."""
    rng = np.random.default_rng(7 + fmt)
    s = SCALE[fmt]
    k = rng.integers(-s, s + 1, 20000).astype(np.float64)
    x = np.concatenate([edge_values(), f32_neighbours(k / s), f32_neighbours((k[:10000] + 0.5) / s).clip(-1, 1),
                        rng.uniform(-1, 1, 30000).astype(np.float32)])[: (1 << 17) - 3]
    want = host_writer(x, fmt, dither)
    same(pack_one(gpu, x, fmt, dither), want, "device against host writer")
    same(model(x, fmt, dither), want, "float64 model against host writer")


def test_fp32_moves_every_bit_pattern_class(gpu):
    rng = np.random.default_rng(1)
    mant = np.concatenate([np.array([0, 1, 2, 0x200000, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff], np.uint32),
                           rng.integers(0, 1 << 23, 40).astype(np.uint32)])
    exp = np.arange(256, dtype=np.uint32)
    bits = (exp[:, None, None] << 23) | mant[None, :, None] | (np.array([0, 1], np.uint32) << 31)[None, None, :]
    x = bits.reshape(-1).view(np.float32)
    got = pack_one(gpu, x, afgpu.WAV_FP32LE, False)
    assert np.array_equal(got.view(np.uint32), bits.reshape(-1))                  # NaN payloads, signalling ones included
    got = pack_one(gpu, x, afgpu.WAV_FP32LE, True)                                # a dither request never touches floats
    assert np.array_equal(got.view(np.uint32), bits.reshape(-1))


def test_fp64_widens_like_numpy(gpu):
    rng = np.random.default_rng(2)
    fin = rng.integers(0, 0x7f800000, 50000).astype(np.uint32)                    # finite, denormals included
    den = rng.integers(1, 0x00800000, 5000).astype(np.uint32)
    qnan = (0x7fc00000 | rng.integers(0, 1 << 22, 500)).astype(np.uint32)         # quiet NaNs keep their payload
    special = np.array([0, 1, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0x3f800000], np.uint32)
    pos = np.concatenate([fin, den, qnan, special])
    bits = np.concatenate([pos, pos | np.uint32(0x80000000)])
    x = bits.view(np.float32)
    got = pack_one(gpu, x, afgpu.WAV_FP64LE, False)
    assert np.array_equal(got.view(np.uint64), x.astype(np.float64).view(np.uint64))
    want = np.frombuffer(afgpu.wav_encode(x[~np.isnan(x)][:, None], 8000, afgpu.WAV_FP64LE), np.uint8)[44:]
    same(pack_one(gpu, x[~np.isnan(x)], afgpu.WAV_FP64LE, False), want, "fp64 against host writer")


def test_span_shapes_and_a_mix_of_everything_in_one_launch(gpu):
    rng = np.random.default_rng(3)
    pieces = []
    for count in (0, 1, 3, 4, 4095, 4096, 4097, 4 * 4096 + 2):
        for fmt in range(5):
            for dither in (False, True):
                pieces.append(dict(x=rng.uniform(-1, 1, count).astype(np.float32), fmt=fmt, dither=dither,
                                   seed=int(rng.integers(0, 1 << 32)), draw0=2 * int(rng.integers(0, 1 << 40))))
    out, spans = pack(gpu, pieces)
    for p, sp in zip(pieces, spans):
        n = p["x"].size * BYTES[p["fmt"]]
        o = int(sp["out_off"])
        same(out[o:o + n], model(p["x"], p["fmt"], p["dither"], p["seed"], p["draw0"]), f"count {p['x'].size} fmt {p['fmt']} dither {p['dither']}")
        pad = out[o + n:o + ((n + 15) & ~15)]
        assert (pad == 0xA5).all(), "bytes behind a span were written"


def test_files_from_one_sample_to_2_24(gpu):
    rng = np.random.default_rng(4)
    sizes = [1, 2, 5, 100, 4097, 65537, (1 << 20) + 3, 1 << 24]
    pieces = [dict(x=rng.uniform(-1, 1, n).astype(np.float32), fmt=afgpu.WAV_S16LE if k % 2 else afgpu.WAV_S24LE, dither=True, seed=k + 1)
              for k, n in enumerate(sizes)]
    out, spans = pack(gpu, pieces)
    for p, sp in zip(pieces, spans):
        n = p["x"].size * BYTES[p["fmt"]]
        same(out[int(sp["out_off"]):int(sp["out_off"]) + n], model(p["x"], p["fmt"], True, p["seed"]), f"{p['x'].size} samples")


@pytest.mark.parametrize("fmt", [afgpu.WAV_S8, afgpu.WAV_S16LE, afgpu.WAV_S24LE], ids=["s8", "s16", "s24"])
def test_a_span_cut_at_a_tile_boundary_continues_the_draws(gpu, fmt):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, 3 * 4096 + 77).astype(np.float32)
    cut = 2 * 4096
    whole = pack_one(gpu, x, fmt, True)
    out, spans = pack(gpu, [dict(x=x[:cut], fmt=fmt, dither=True, draw0=0), dict(x=x[cut:], fmt=fmt, dither=True, draw0=2 * cut)])
    b = BYTES[fmt]
    two = np.concatenate([out[:cut * b], out[int(spans[1]["out_off"]):int(spans[1]["out_off"]) + (x.size - cut) * b]])
    same(two, whole, "two spans against one")
    same(whole, model(x, fmt, True), "one span against the model")
    wrong = pack_one(gpu, x[cut:], fmt, True, draw0=0)
    assert not np.array_equal(wrong, whole[cut * b:])                            # the position does matter


def test_spans_outside_the_planes_are_not_touched(gpu):
    x = np.linspace(-1, 1, 8192, dtype=np.float32)
    ok = dict(x=x, fmt=afgpu.WAV_S16LE, dither=False)
    cases = [
        (dict(ok, count=8192 + 4), {}),                                           # reads past in_floats
        (dict(ok, in_off=1 << 40), {}),
        (dict(ok, count=1 << 30), {}),
        (dict(ok), dict(out_bytes=8192 * 2 - 16)),                                # writes past out_bytes
        (dict(ok, out_off=16), dict(out_bytes=8192 * 2)),
        (dict(ok, out_off=(1 << 63)), {}),
        (dict(ok, in_off=2, count=4096), {}),                                     # not aligned as the header states
        (dict(ok, out_off=8, count=4096), {}),
        (dict(ok, fmt=5), {}),                                                    # no such format
    ]
    for piece, kw in cases:
        out, _ = pack(gpu, [piece], **kw)
        assert (out == 0xA5).all(), (piece.get("count"), piece.get("in_off"), piece.get("out_off"), kw)
    out, _ = pack(gpu, [ok])                                                      # and the same span inside the planes is packed
    same(out[:8192 * 2], model(x, afgpu.WAV_S16LE, False), "control")


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_spans_without_tiles(gpu, case):
    """1, 2 and 5 spans, with spans of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(11)
    pieces = [dict(x=rng.uniform(-1, 1, n).astype(np.float32), fmt=afgpu.WAV_S16LE, dither=True, seed=SEED + k)
              for k, n in enumerate(record_lengths(afgpu.WAV_TILE_SAMPLES)[case])]
    out, spans = pack(gpu, pieces)
    want = np.full(out.size, 0xA5, np.uint8)
    for p, sp in zip(pieces, spans):
        body = model(p["x"], p["fmt"], True, seed=p["seed"])
        want[int(sp["out_off"]):int(sp["out_off"]) + body.size] = body
    same(out, want, case)
