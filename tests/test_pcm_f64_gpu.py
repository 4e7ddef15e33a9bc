"""The conversion to float64 on the device (afg_pcm_to_f64_hip, csrc/pcm_f64.hip) against tests/f64_model.py, compared as
uint64: no tolerance, no excluded input.  The one clause that is not bit equality is the signalling float32 NaN, whose
result has to be a NaN with the input's sign (its quiet bit is not specified).

On the commit before float64 reads every test here fails: afgpu.pcm_to_f64 and the library's entry do not exist."""
import numpy as np
import pytest

import afgpu
import f64_model as fm
from record_cases import RECORD_CASES, record_lengths

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0x7FF8DEADBEEF0123)                             # what an output double nobody wrote holds


def launch(gpu, recs, plane, in_bytes, out_doubles):
    """One launch over a sentinel-filled output plane; returns the plane as uint64."""
    import torch
    tiles = afgpu.wav_layout(recs)
    assert tiles == sum(-(-int(r["count"]) // afgpu.WAV_TILE_SAMPLES) for r in recs)
    d_in = torch.from_numpy(plane).to(gpu)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).to(gpu)
    d_out = torch.from_numpy(np.full(out_doubles, SENTINEL, np.uint64).view(np.float64).copy()).to(gpu)
    afgpu.pcm_to_f64(len(recs), d_recs, tiles, d_in, in_bytes, d_out, out_doubles)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


def layout(spans):
    """spans: (kind, sample bytes, in_off modulo 16, out_off modulo 2).  Records, input plane, plane sizes."""
    recs = np.zeros(len(spans), afgpu.WAV_SPAN_DTYPE)
    in_at, out_at = 0, 0
    for k, (kind, raw, in_mis, out_mis) in enumerate(spans):
        assert len(raw) % fm.KIND_BYTES[kind] == 0
        in_at = (in_at + 15) // 16 * 16 + in_mis
        out_at = (out_at + 1) // 2 * 2 + out_mis
        recs[k] = (in_at, out_at, len(raw) // fm.KIND_BYTES[kind], 0, kind, 0)
        in_at += len(raw)
        out_at += int(recs[k]["count"])
    in_bytes, out_doubles = (in_at + 15) // 16 * 16 + 16, (out_at + 1) // 2 * 2 + 2
    plane = np.zeros(in_bytes, np.uint8)
    for r, (_, raw, _, _) in zip(recs, spans):
        plane[int(r["in_off"]):int(r["in_off"]) + len(raw)] = np.frombuffer(raw, np.uint8)
    return recs, plane, in_bytes, out_doubles


def convert(gpu, spans, check=None):
    """One launch; every span against the model (or `check(k, got_bits, raw)`), and no double outside the spans written."""
    recs, plane, in_bytes, out_doubles = layout(spans)
    got = launch(gpu, recs, plane, in_bytes, out_doubles)
    untouched = np.ones(out_doubles, bool)
    for k, (r, (kind, raw, _, _)) in enumerate(zip(recs, spans)):
        o, n = int(r["out_off"]), int(r["count"])
        if check is not None and check(k, got[o:o + n], raw):
            pass
        else:
            want = fm.convert(raw, kind).view(np.uint64)
            bad = np.flatnonzero(got[o:o + n] != want)
            if bad.size:
                print(f"span {k} {fm.KIND_NAMES[kind]}: {bad.size} of {n} differ, first at {bad[0]}: got {got[o + bad[0]]:#x} want {want[bad[0]]:#x}")
            assert bad.size == 0, (k, fm.KIND_NAMES[kind])
        untouched[o:o + n] = False
    assert (got[untouched] == SENTINEL).all(), "a double outside every span was written"
    return got


def test_u8_every_input(gpu):
    convert(gpu, [(fm.KIND_U8, np.arange(256, dtype=np.uint8).tobytes(), 0, 0)])


def test_s16_every_input(gpu):
    convert(gpu, [(fm.KIND_S16, np.arange(65536, dtype="<u2").tobytes(), 0, 0)])


def test_s24_every_input(gpu):
    v = np.arange(1 << 24, dtype=np.uint32)
    s24 = np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8).tobytes()
    convert(gpu, [(fm.KIND_S24, s24, 0, 0)])


def test_divided_kinds_through_the_per_sample_path(gpu):
    """the same arithmetic where a span's base is not aligned for the wide loads and stores"""
    v = np.arange(1 << 16, dtype=np.uint32) * 251 + 7
    s24 = np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], 1).astype(np.uint8).tobytes()
    convert(gpu, [(fm.KIND_U8, np.arange(256, dtype=np.uint8).tobytes(), 1, 1), (fm.KIND_S16, np.arange(65536, dtype="<u2").tobytes(), 2, 0),
                  (fm.KIND_S24, s24, 3, 1)])


@pytest.mark.parametrize("kind", [fm.KIND_S32, fm.KIND_FLAC_S32])
def test_int32_kinds(gpu, kind):
    rng = np.random.default_rng(41)
    edges = [0, 1, -1, -2**31, 2**31 - 1, 2**30, -2**30]
    edges += [s * (2**24 + d) for s in (1, -1) for d in (1, -1)]
    shifted = (np.arange(65536, dtype=np.int64) << 16).astype(np.uint32).view(np.int32)
    v = np.concatenate([np.array(edges, np.int64).astype("<i4"), shifted.astype("<i4"), rng.integers(-2**31, 2**31, 1 << 20, dtype=np.int64).astype("<i4")])
    convert(gpu, [(kind, v.tobytes(), 0, 0), (kind, v[:5001].tobytes(), 4, 1)])


def test_f32(gpu):
    rng = np.random.default_rng(42)
    n = 1 << 20
    sign = rng.integers(0, 2, 1 << 16, dtype=np.uint64).astype(np.uint32) << 31
    denormal = sign | rng.integers(1, 0x00800000, 1 << 16, dtype=np.uint64).astype(np.uint32)
    quiet = sign | np.uint32(0x7FC00000) | rng.integers(0, 0x00400000, 1 << 16, dtype=np.uint64).astype(np.uint32)
    signalling = sign | np.uint32(0x7F800000) | rng.integers(1, 0x00400000, 1 << 16, dtype=np.uint64).astype(np.uint32)
    assert fm.is_signalling_f32(signalling).all() and not fm.is_signalling_f32(quiet).any()
    edges = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                      0x7FFFFFFF, 0xFFFFFFFF, 0x3F800000, 0x7F7FFFFF], np.uint32)
    rand = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    rand = rand[~fm.is_signalling_f32(rand)]
    rand = rand[:rand.size & ~3]
    exact = np.concatenate([edges, denormal, quiet, rand])

    def nan_with_the_sign(k, got, raw):
        if k != 1 and k != 3:
            return False
        src = np.frombuffer(raw, "<u4")
        is_nan = ((got & np.uint64(0x7FF0000000000000)) == np.uint64(0x7FF0000000000000)) & ((got & np.uint64(0x000FFFFFFFFFFFFF)) != 0)
        assert is_nan.all(), "a signalling NaN did not come out a NaN"
        assert ((got >> np.uint64(63)).astype(np.uint32) == (src >> 31)).all(), "a signalling NaN lost its sign"
        return True

    convert(gpu, [(fm.KIND_F32, exact.astype("<u4").tobytes(), 0, 0), (fm.KIND_F32, signalling.astype("<u4").tobytes(), 0, 0),
                  (fm.KIND_F32, exact[:5003].astype("<u4").tobytes(), 4, 1), (fm.KIND_F32, signalling[:1001].astype("<u4").tobytes(), 1, 0)],
            check=nan_with_the_sign)


def test_f64_bits_survive(gpu):
    rng = np.random.default_rng(43)
    n = 1 << 20
    rand = rng.integers(0, 2**64, n, dtype=np.uint64)
    sign = rng.integers(0, 2, 4096, dtype=np.uint64) << np.uint64(63)
    payload = rng.integers(1, 2**51, 4096, dtype=np.uint64)
    classes = np.concatenate([sign | np.uint64(0x7FF8000000000000) | payload,          # quiet NaNs
                              sign | np.uint64(0x7FF0000000000000) | payload,          # signalling NaNs
                              sign | np.uint64(0x7FF0000000000000),                    # infinities
                              sign | payload,                                          # denormals
                              sign])                                                   # zeros
    v = np.concatenate([classes, rand])
    got = convert(gpu, [(fm.KIND_F64, v.astype("<u8").tobytes(), 0, 0), (fm.KIND_F64, v[:5001].astype("<u8").tobytes(), 8, 1)])
    assert (got[:v.size] == v).all()


def random_samples(rng, kind, n):
    raw = rng.integers(0, 256, n * fm.KIND_BYTES[kind], dtype=np.uint8)
    if kind == fm.KIND_F32:                                  # signalling NaNs have a clause of their own (test_f32)
        w = raw.view("<u4").copy()
        w[fm.is_signalling_f32(w)] |= np.uint32(0x00400000)
        raw = w.view(np.uint8)
    return raw.tobytes()


def test_shapes_with_all_kinds_in_one_launch(gpu):
    rng = np.random.default_rng(44)
    spans = []
    counts = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193]
    for i, n in enumerate(counts):
        for kind in range(7):
            for j, in_mis in enumerate((0, 1, 2, 3)):
                spans.append((kind, random_samples(rng, kind, n), in_mis, (i + kind + j) & 1))
    # every (count, kind) also with both parities of out_off at an aligned in_off
    for i, n in enumerate(counts):
        for kind in range(7):
            spans.append((kind, random_samples(rng, kind, n), 0, (i + kind + 1) & 1))
    order = rng.permutation(len(spans))
    convert(gpu, [spans[k] for k in order])


def test_adjacent_spans_and_spans_that_leave_the_planes(gpu):
    """Spans packed back to back keep off each other's doubles; a span whose end lies past in_bytes, and one past
    out_doubles, leave the plane untouched while their neighbours are converted."""
    rng = np.random.default_rng(45)
    kinds = [fm.KIND_S16, fm.KIND_F64, fm.KIND_U8, fm.KIND_S24, fm.KIND_FLAC_S32, fm.KIND_F32, fm.KIND_S32]
    counts = [4097, 5, 4096, 8193, 3, 4095, 1]
    raws = [random_samples(rng, k, n) for k, n in zip(kinds, counts)]
    recs = np.zeros(len(kinds) + 2, afgpu.WAV_SPAN_DTYPE)
    in_at, out_at = 0, 2
    for k, (kind, n, raw) in enumerate(zip(kinds, counts, raws)):
        recs[k] = (in_at, out_at, n, 0, kind, 0)              # output spans touch: out_off of one is the end of the one before
        in_at += (len(raw) + 15) // 16 * 16
        out_at += n
    gap = out_at                                              # 6000 doubles nobody may write: the two bad spans point here
    out_doubles = gap + 6000
    in_bytes = in_at + 16
    recs[-2] = (in_bytes - 4000 * 2 + 2, gap, 4000, 0, fm.KIND_S16, 0)              # ends 2 bytes past in_bytes
    recs[-1] = (0, out_doubles - 4999, 5000, 0, fm.KIND_U8, 0)                        # ends 1 double past out_doubles
    recs = recs[[0, 1, 7, 2, 3, 8, 4, 5, 6]]                  # the bad ones between good neighbours
    plane = rng.integers(0, 256, in_bytes, dtype=np.uint8)
    at = 0
    for raw in raws:
        plane[at:at + len(raw)] = np.frombuffer(raw, np.uint8)
        at += (len(raw) + 15) // 16 * 16
    got = launch(gpu, recs, plane, in_bytes, out_doubles)
    o = 2
    for kind, n, raw in zip(kinds, counts, raws):
        assert (got[o:o + n] == fm.convert(raw, kind).view(np.uint64)).all(), fm.KIND_NAMES[kind]
        o += n
    assert (got[:2] == SENTINEL).all() and (got[gap:] == SENTINEL).all()


@pytest.mark.parametrize("case", RECORD_CASES)
def test_record_counts_and_spans_without_tiles(gpu, case):
    """1, 2 and 5 spans, with spans of no samples first, in the middle and last (record_cases.py): the tile search's edges"""
    rng = np.random.default_rng(7)
    convert(gpu, [(fm.KIND_S16, rng.integers(0, 65536, n, dtype=np.uint64).astype("<u2").tobytes(), 2 * (k % 2), k % 2)
                  for k, n in enumerate(record_lengths(afgpu.WAV_TILE_SAMPLES)[case])])
