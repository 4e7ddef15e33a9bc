"""Hand-built QOA frame batches for the decoder tests: tests/test_qoa_model.py holds the integer model (qoa_model.py) and
the CPU oracle to each other on every case here, tests/test_qoa_decode_edges_gpu.py holds the kernel to both.

`build` lays out the byte plane and the output plane itself.  Every frame is a valid frame at a multiple of 8 bytes with
8 to 40 filler bytes before it, between frames and after the last one; every output row is followed by at least four
values no frame writes.  A frame may carry the slices a full 5120-sample frame has (`tails`): its size field covers
them, its sample count does not, and a decoder never looks at them.  A record with samples == 0 (include/afg.h) points
at a whole 20-sample stereo frame of its own and writes nothing.
"""
import functools
import zlib

import numpy as np

import afgpu
import oraclelib
import qoa_model

ODD_TAILS = (1, 2, 19, 20, 21, 39, 40, 41, 79, 80, 81, 99, 159, 160, 161, 5119, 5120)
# the largest scalefactor with one residual code repeated (test_qoa_gpu.py::test_qoa_weights_at_their_largest)
LARGEST_WORDS = (0xFFFFFFFFFFFFFFFF, 0xFDB6DB6DB6DB6DB6, 0xF000000000000000, 0xFB6DB6DB6DB6DB6D)
# one channel's history + weights, the three extreme states of the same test
EXTREME_LMS = ([32767] * 4 + [32767] * 4, [-32768] * 4 + [-32768] * 4,
               [-32768, 32767, -32768, 32767] + [32767, -32768, 32767, -32768])
I16_SENTINEL = -7
F32_SENTINEL_BITS = 0x7fc00000                       # a quiet NaN


def seed_of(name):
    return zlib.crc32(name.encode())


class Case:
    """frames (afgpu.QOA_FRAME_DTYPE), data (uint8 plane), out_total; `filler` marks the bytes outside every frame, `tail`
    the slices a frame carries past its last sample."""

    def __init__(self, name, frames, data, out_total, filler, tail):
        self.name, self.frames, self.data, self.out_total, self.filler, self.tail = name, frames, data, int(out_total), filler, tail
        self._model = self._oracle = None
        self._derived = {}

    def rows(self):
        """(first output value, number of values) per record"""
        return [(int(f["out_off"]), int(f["samples"]) * int(f["channels"])) for f in self.frames]

    def model(self):
        """qoa_model.decode of the case, computed once; self.peak: per record, the largest weight magnitude reached"""
        if self._model is None:
            stats = {}
            self._model = qoa_model.decode(self.frames, self.data, self.out_total, stats)
            self.peak = stats["max_abs_weight"]
            mask = np.zeros(self.out_total, bool)
            for off, cnt in self.rows():
                mask[off:off + cnt] = True
            assert (mask == self._model[0]).all(), "the model wrote something other than the rows"
            assert int(mask.sum()) == sum(cnt for _, cnt in self.rows())
        return self._model

    def oracle(self):
        if self._oracle is None:
            self._oracle = oraclelib.qoa_transform(self.frames, self.data, self.out_total)
        return self._oracle

    def shifted(self, row):
        """the same rows with row `row` moved by two values (still four untouched values on either side)"""
        if ("shift", row) not in self._derived:
            frames = self.frames.copy()
            frames["out_off"][row] += 2
            self._derived["shift", row] = Case(f"{self.name}/shift{row}", frames, self.data, self.out_total, self.filler, self.tail)
        return self._derived["shift", row]

    def redrawn(self, which, seed):
        """the same frames with every byte of `which` ("filler" or "tail") drawn again"""
        if (which, seed) not in self._derived:
            mask = getattr(self, which)
            data = self.data.copy()
            data[mask] = np.random.default_rng(seed).integers(0, 256, int(mask.sum()), dtype=np.uint8)
            assert (data[mask] != self.data[mask]).any()
            self._derived[which, seed] = Case(f"{self.name}/{which}{seed}", self.frames, data, self.out_total, self.filler, self.tail)
        return self._derived[which, seed]

    def only(self, keep):
        """a launch of the records `keep` alone, over the same planes"""
        keep = tuple(keep)
        if ("only", keep) not in self._derived:
            self._derived["only", keep] = Case(f"{self.name}/only", self.frames[np.asarray(keep)].copy(), self.data, self.out_total,
                                               self.filler, self.tail)
        return self._derived["only", keep]


def _pick(choice, f):
    return choice[f % len(choice)] if isinstance(choice, (list, tuple)) and not isinstance(choice[0], (int, np.integer)) else choice


def driven_words(lms, samples):
    """Slices that move the newest sample's weight by the largest step, 896, away from zero at every sample: scalefactor 15
    and the residual code (6: +14336, 7: -14336) whose sign suits the history value the weight meets.  After n samples the
    weight is 896 n beyond the int16 it started from, whatever the prediction does meanwhile."""
    h = np.array([lms[:4]], np.int64)
    w = np.array([lms[4:]], np.int64)
    away = 1 if lms[7] >= 0 else -1
    nsl = -(-samples // qoa_model.SLICE_LEN)
    codes = np.zeros(nsl * qoa_model.SLICE_LEN, np.uint64)
    for t in range(samples):
        codes[t] = 6 if (h[0, 3] >= 0) == (away > 0) else 7
        qoa_model.step(h, w, qoa_model.DEQUANT[15, codes[t:t + 1].astype(np.int64)])
    assert abs(int(w[0, 3])) == abs(int(lms[7])) + 896 * samples
    shifts = np.uint64(57) - np.uint64(3) * np.arange(qoa_model.SLICE_LEN, dtype=np.uint64)
    return np.uint64(15 << 60) | np.bitwise_or.reduce(codes.reshape(nsl, qoa_model.SLICE_LEN) << shifts, axis=1)


def _frame_bytes(rng, samples, channels, word, lms, tails):
    """One frame: header, LMS state, slices.  word: "random", "driven" (driven_words) or a 64-bit value repeated; lms: "random" or eight int16
    (history, weights) given to every channel.  Returns (bytes, number of bytes the decoder needs)."""
    nsl = -(-samples // qoa_model.SLICE_LEN)
    carried = 256 if tails and samples <= 5120 else nsl
    size = 8 + 16 * channels + 8 * channels * carried
    assert size <= 0xffff
    hdr = np.array([(channels << 56) | (44100 << 32) | (samples << 16) | size], ">u8").view(np.uint8)
    if isinstance(lms, str):
        state = rng.integers(0, 256, 16 * channels, dtype=np.uint8)
    else:
        state = np.tile(np.asarray(lms, ">i2").view(np.uint8), channels)
    if word == "driven":
        body = np.repeat(driven_words(lms, samples), channels)
    elif isinstance(word, str):
        body = rng.integers(0, 1 << 64, nsl * channels, dtype=np.uint64)
    else:
        body = np.full(nsl * channels, word, np.uint64)
    rest = rng.integers(0, 1 << 64, (carried - nsl) * channels, dtype=np.uint64)
    out = np.concatenate([hdr, state, body.astype(">u8").view(np.uint8), rest.astype(">u8").view(np.uint8)])
    return out, 8 + 16 * channels + 8 * channels * nsl


def build(name, shapes, words="random", lms="random", layout="aligned", tails=False):
    """shapes: (samples, channels) per record; samples 0 makes a skipped record.  words / lms: one choice for all frames
    or a list of choices taken in turn.  layout "aligned": every out_off a multiple of 4; "free": any."""
    rng = np.random.default_rng(seed_of(name))
    frames = np.zeros(len(shapes), afgpu.QOA_FRAME_DTYPE)
    planes, filler, tail, at, out = [], [], [], 0, 0

    def fill():
        nonlocal at
        n = 8 * int(rng.integers(1, 6))
        planes.append(rng.integers(0, 256, n, dtype=np.uint8))
        filler.append(np.ones(n, bool)); tail.append(np.zeros(n, bool))
        at += n

    for f, (samples, channels) in enumerate(shapes):
        fill()
        if samples == 0:
            body, used = _frame_bytes(rng, 20, 2, "random", "random", False)
        else:
            body, used = _frame_bytes(rng, samples, channels, _pick(words, f), _pick(lms, f), tails)
        assert at % 8 == 0
        out += int(rng.integers(6, 14))
        if layout == "aligned":
            out = (out + 3) & ~3
        frames[f] = (at, out, samples, channels, 0)
        planes.append(body)
        filler.append(np.zeros(body.size, bool))
        tail.append(np.arange(body.size) >= used)
        at += body.size
        out += samples * channels
    fill()
    out += int(rng.integers(6, 14))
    return Case(name, frames, np.concatenate(planes), out, np.concatenate(filler), np.concatenate(tail))


def ragged(rng, n, cap=161):
    """n sample counts of at most `cap` from ODD_TAILS, `cap` itself among them when it is one"""
    pool = [s for s in ODD_TAILS if s <= cap]
    counts = [int(x) for x in rng.choice(pool, n)]
    counts[int(rng.integers(0, n))] = pool[-1]
    return counts


# ------------------------------------------------------------------------------------------------------ the cases ---
@functools.lru_cache(maxsize=None)
def odd_tails():
    """32 stereo frames: every count of ODD_TAILS, then 15 of them again in shuffled order; random slices and state"""
    rng = np.random.default_rng(seed_of("odd_tails/order"))
    counts = list(ODD_TAILS) + [int(x) for x in rng.permutation(ODD_TAILS)[:15]]
    return build("odd_tails", [(s, 2) for s in counts], tails=True)


SMALL_CAPS = (20, 40, 99, 160, 161)                  # max_slices 1, 2, 5, 8, 9


@functools.lru_cache(maxsize=None)
def small_tails(cap):
    rng = np.random.default_rng(seed_of(f"small_tails{cap}/counts"))
    return build(f"small_tails{cap}", [(s, 2) for s in ragged(rng, 32, cap)], tails=True)


COMPOSITION_COUNTS = (1, 31, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def composition(n_frames):
    rng = np.random.default_rng(seed_of(f"composition{n_frames}/counts"))
    return build(f"composition{n_frames}", [(s, 2) for s in ragged(rng, n_frames)])


@functools.lru_cache(maxsize=None)
def one_mono():
    """65 frames, frame 40 mono: wavefront 1 takes the general path, wavefronts 0 and 2 the fast one"""
    rng = np.random.default_rng(seed_of("one_mono/counts"))
    shapes = [(s, 2) for s in ragged(rng, 65)]
    shapes[40] = (shapes[40][0], 1)
    return build("one_mono", shapes)


ZERO_RECORDS = (0, 13, *range(32, 64), 64, 80)


@functools.lru_cache(maxsize=None)
def zero_records():
    """96 stereo records; samples == 0 first in a wavefront and in its middle (wavefronts 0 and 2) and all through wavefront 1"""
    rng = np.random.default_rng(seed_of("zero_records/counts"))
    shapes = [(s, 2) for s in ragged(rng, 96)]
    for f in ZERO_RECORDS:
        shapes[f] = (0, 2)
    return build("zero_records", shapes)


GENERAL_TAILS = (1, 19, 21, 161, 5120)


@functools.lru_cache(maxsize=None)
def general():
    """channel counts 1 to 8, each with every count of GENERAL_TAILS, in shuffled order: 40 frames, two wavefronts"""
    rng = np.random.default_rng(seed_of("general/order"))
    shapes = [(s, c) for c in range(1, 9) for s in GENERAL_TAILS]
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    return build("general", shapes, layout="free", tails=True)


SWITCH_KINDS = ("9000", "9020", "9020+short", "9400")
SWITCH_WORDS = LARGEST_WORDS + ("driven",)
ODD_SHIFT, SMALL_SHIFT, MONO_SHIFT, ZERO_SHIFT = 16, 9, 3, 70        # the row the shifted layout of each case moves


def word_id(word):
    return word if isinstance(word, str) else f"{word:x}"


@functools.lru_cache(maxsize=None)
def switch(kind, word):
    """all-stereo wavefronts around the kernel's 24-bit limit: one largest-weight word, the extreme states in turn"""
    if kind == "9020+short":
        rng = np.random.default_rng(seed_of("switch/counts"))
        counts = [int(x) for x in rng.choice([s for s in ODD_TAILS if 19 <= s <= 161], 31)]
        shapes = [(s, 2) for s in counts[:7]] + [(9020, 2)] + [(s, 2) for s in counts[7:]]
    else:
        shapes = [(int(kind), 2)] * 3
    return build(f"switch{kind}/{word}", shapes, words=word, lms=list(EXTREME_LMS))


SWITCH_LONG_ROW = 7


@functools.lru_cache(maxsize=None)
def crafted(samples, word, lms, n_frames=3):
    """the stereo frames test_qoa_gpu.py crafts: word "random", "half" (all ones or random, evenly) or a value"""
    if word == "half":
        rng = np.random.default_rng(samples)
        case = build(f"crafted{samples}/half/{n_frames}", [(samples, 2)] * n_frames, lms="random" if lms is None else list(lms))
        data = case.data.copy()
        for f in case.frames:
            body = data[int(f["byte_off"]) + 40:int(f["byte_off"]) + 40 + 16 * -(-samples // 20)].view(">u8")
            body[rng.random(body.size) < 0.5] = 0xFFFFFFFFFFFFFFFF
        return Case(case.name, case.frames, data, case.out_total, case.filler, case.tail)
    return build(f"crafted{samples}/{word}/{lms}/{n_frames}", [(samples, 2)] * n_frames, words=word,
                 lms="random" if lms is None else list(lms))


def crafted_cases():
    """(name, maker) of what tests/test_qoa_gpu.py builds by hand: 5120 samples at the largest weights, 12000 and 20000
    random and extreme.  Makers, so that collecting the tests builds nothing."""
    far = tuple([-32768] * 4 + [32767] * 4)
    cases = [(f"crafted5120-{w:x}-{i}", functools.partial(crafted, 5120, w, tuple(s))) for w in LARGEST_WORDS for i, s in enumerate(EXTREME_LMS)]
    cases += [("crafted12000-random", functools.partial(crafted, 12000, "random", None)),
              ("crafted12000-ones", functools.partial(crafted, 12000, LARGEST_WORDS[0], far)),
              ("crafted20000-half", functools.partial(crafted, 20000, "half", None, 2)),
              ("crafted20000-ones", functools.partial(crafted, 20000, LARGEST_WORDS[0], far, 1))]
    return cases


def short_rows():
    return [f for f in range(32) if f != SWITCH_LONG_ROW]


def gpu_cases():
    """(name, maker) of every case tests/test_qoa_decode_edges_gpu.py launches, in both output layouts where it has two"""
    cases = [("odd_tails", odd_tails), ("odd_tails-shifted", lambda: odd_tails().shifted(ODD_SHIFT))]
    for cap in SMALL_CAPS:
        cases += [(f"small_tails{cap}", functools.partial(small_tails, cap)),
                  (f"small_tails{cap}-shifted", lambda cap=cap: small_tails(cap).shifted(SMALL_SHIFT))]
    for n in COMPOSITION_COUNTS:
        cases += [(f"composition{n}", functools.partial(composition, n)),
                  (f"composition{n}-shifted", lambda n=n: composition(n).shifted(n - 1))]
    cases += [("composition64-row5", lambda: composition(64).shifted(5)), ("one_mono", one_mono),
              ("one_mono-shifted", lambda: one_mono().shifted(MONO_SHIFT)), ("zero_records", zero_records),
              ("zero_records-shifted", lambda: zero_records().shifted(ZERO_SHIFT)), ("general", general)]
    for kind in SWITCH_KINDS:
        for word in SWITCH_WORDS:
            cases.append((f"switch{kind}-{word_id(word)}", functools.partial(switch, kind, word)))
    cases += [(f"switch-short-alone-{word_id(w)}", lambda w=w: switch("9020+short", w).only(short_rows())) for w in SWITCH_WORDS]
    cases += [("odd_tails-filler", lambda: odd_tails().redrawn("filler", 1)), ("odd_tails-tail", lambda: odd_tails().redrawn("tail", 2)),
              ("general-filler", lambda: general().redrawn("filler", 3)), ("general-tail", lambda: general().redrawn("tail", 4))]
    return cases
