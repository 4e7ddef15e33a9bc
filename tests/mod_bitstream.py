"""A generator of ProTracker MOD files for the MOD tests: 15- and 31-instrument files, the 4-channel tags and xCHN / xxCH for
1-32 channels, every effect pocketmod.d handles (0-F, E1-EE), one-shot, looped (down to 4 bytes) and zero-length samples, a
last sample cut by the end of the file, period-0 notes and songs that never end."""
import numpy as np

PERIODS = [856, 808, 762, 720, 678, 640, 604, 570, 538, 508, 480, 453, 428, 404, 381, 360, 339, 320,
           302, 285, 269, 254, 240, 226, 214, 202, 190, 180, 170, 160, 151, 143, 135, 127, 120, 113]


def tag_for(channels, style=None):
    if style is not None:
        return style
    if channels == 4:
        return b"M.K."
    return (b"%dCHN" % channels) if channels < 10 else (b"%dCH" % channels)


def cell(sample=0, period=0, effect=0, param=0):
    """4 bytes of a pattern cell; effect 0x0-0xF, or 0xE0-0xEF for the extended ones (param then 0-15)."""
    if effect >= 0xE0:
        eff = 0xE00 | ((effect & 0x0f) << 4) | (param & 0x0f)
    else:
        eff = (effect << 8) | (param & 0xff)
    return bytes([(sample & 0xf0) | ((period >> 8) & 0x0f), period & 0xff, ((sample & 0x0f) << 4) | ((eff >> 8) & 0x0f), eff & 0xff])


class Sample:
    def __init__(self, data=b"", finetune=0, volume=64, loop_start=0, loop_length=0, declared=None, name=b"smp"):
        self.data = bytes(data)
        self.finetune, self.volume = finetune, volume
        self.loop_start, self.loop_length = loop_start, loop_length       # bytes (even)
        self.declared = declared                                           # length in the header (bytes); default len(data)
        self.name = name


def build(patterns, order, samples, channels=4, instruments=31, tag=None, reset=0, title=b"generated", length=None, trailer=b""):
    """patterns: list of [64][channels] cells (bytes of 4); order: list of pattern indices; samples: list of Sample (at most
    instruments).  Sample data follow the patterns in order; `trailer` is appended after them."""
    out = bytearray(title[:20].ljust(20, b"\0"))
    for i in range(instruments):
        s = samples[i] if i < len(samples) else Sample(name=b"")
        dl = len(s.data) if s.declared is None else s.declared
        out += s.name[:22].ljust(22, b"\0")
        out += (dl // 2).to_bytes(2, "big") + bytes([s.finetune & 0x0f, s.volume & 0xff])
        out += (s.loop_start // 2).to_bytes(2, "big") + (s.loop_length // 2).to_bytes(2, "big")
    out += bytes([len(order) if length is None else length, reset])
    out += bytes(order).ljust(128, b"\0")
    if instruments == 31:
        out += tag_for(channels, tag)
    for p in patterns:
        for row in p:
            assert len(row) == channels
            for c in row:
                out += c
    for s in samples[:instruments]:
        out += s.data
    out += trailer
    return bytes(out)


def empty_pattern(channels):
    return [[cell() for _ in range(channels)] for _ in range(64)]


def random_sample(rng, n, loop=None, finetune=0, volume=64, **kw):
    data = rng.integers(-128, 128, n, dtype=np.int16).astype(np.int8).tobytes()
    if loop is None:
        return Sample(data, finetune, volume, **kw)
    return Sample(data, finetune, volume, loop[0], loop[1], **kw)


# every effect pocketmod.d:423-662 handles, with parameter ranges that exercise it
EFFECTS = [0x0, 0x1, 0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x8, 0x9, 0xA, 0xC, 0xE1, 0xE2, 0xE4, 0xE5, 0xE7, 0xE8, 0xE9, 0xEA, 0xEB,
           0xEC, 0xED, 0xEE, 0xF]


def random_song(rng, channels=4, n_patterns=2, instruments=31, tag=None, p_note=0.35, p_effect=0.5, jumps=True,
                n_samples=8, max_sample=3000, last_cut=False, zero_length=True, period0=True, order=None):
    """A song with random notes and effects.  Bxx / Dxx / E6x appear where `jumps`; the last pattern in the order ends
    the song (jumps go forward only, so the song returns to order 0 and ends)."""
    samples = []
    for i in range(min(n_samples, instruments)):
        n = int(rng.integers(8, max_sample)) & ~1
        kind = rng.integers(0, 4)
        ft = int(rng.integers(0, 16))
        vol = int(rng.integers(0, 70))
        if kind == 0:
            samples.append(random_sample(rng, n, None, ft, vol))
        elif kind == 1:                                        # short loop at the end
            ll = int(rng.choice([4, 6, 8, 32]))
            samples.append(random_sample(rng, n, (n - ll, ll), ft, vol))
        elif kind == 2:                                        # loop in the middle
            ls = int(rng.integers(0, n // 2)) & ~1
            ll = max(4, int(rng.integers(0, n - ls)) & ~1)
            samples.append(random_sample(rng, n, (ls, ll), ft, vol))
        else:                                                  # loop that runs past the sample's end
            ls = (n // 2) & ~1
            samples.append(random_sample(rng, n, (ls, n), ft, vol))
    if zero_length and samples:
        samples[int(rng.integers(0, len(samples)))] = Sample(b"", 0, 40, 0, 0)
    if last_cut and samples:
        samples[-1].declared = len(samples[-1].data) + 64      # the file ends 64 bytes early
    order = list(range(n_patterns)) if order is None else order
    pats = []
    for pi in range(n_patterns):
        p = empty_pattern(channels)
        for r in range(64):
            for c in range(channels):
                smp = per = eff = par = 0
                if rng.random() < p_note:
                    smp = int(rng.integers(1, len(samples) + 1)) if samples else 0
                    per = int(rng.choice(PERIODS))
                    if period0 and rng.random() < 0.03:
                        per = int(rng.integers(1, 60))                         # with finetune: period <= 0 or 0
                if rng.random() < p_effect:
                    eff = int(rng.choice(EFFECTS))
                    par = int(rng.integers(0, 256))
                    if eff == 0xF:
                        par = int(rng.choice([0, 1, 3, 6, 8, 0x1f, 0x20, 0x7d, 0x96, 0xff]))
                    if eff == 0xEE:
                        par = int(rng.integers(0, 3))
                    if eff == 0xE9:
                        par = int(rng.integers(0, 4))
                    if eff >= 0xE0:
                        par &= 0x0f
                p[r][c] = cell(smp, per, eff, par)
        if jumps:
            r = int(rng.integers(8, 40))
            p[r][0] = cell(0, 0, 0xE6, 0)                                    # loop start ...
            p[r + 4][0] = cell(0, 0, 0xE6, int(rng.integers(1, 3)))           # ... twice or so
            if pi + 1 < n_patterns and rng.random() < 0.5:
                p[60][channels - 1] = cell(0, 0, 0xD, int(rng.choice([0x00, 0x10, 0x32])))   # break into the next
            if pi == 0 and n_patterns > 2 and rng.random() < 0.5:
                p[50][0] = cell(0, 0, 0xB, 2)                                 # jump forward
        pats.append(p)
    data = build(pats, order, samples, channels, instruments, tag)
    return data[:-64] if last_cut else data                                  # the last sample runs past the end of the file


def endless_song(rng, channels=4):
    """One order whose last line breaks back to line 5 of the same pattern: the song never returns to line 0."""
    s = random_sample(rng, 2000, (1000, 996), 0, 50)
    p = empty_pattern(channels)
    p[0][0] = cell(1, 428)
    p[63][0] = cell(0, 0, 0xD, 0x05)
    p[10][1 % channels] = cell(1, 214, 0x4, 0x46)
    return build([p], [0], [s], channels, 31)


def single_note(period=428, finetune=0, volume=64, n=20000, loop=None, effect=0, param=0, speed=None, data=None):
    """One note on channel 0 of a 4-channel module, nothing else."""
    smp = Sample(data if data is not None else (np.arange(n) % 251 - 125).astype(np.int8).tobytes(), finetune, volume,
                 *(loop or (0, 0)))
    p = empty_pattern(4)
    p[0][0] = cell(1, period, effect, param)
    if speed is not None:
        p[0][1] = cell(0, 0, 0xF, speed)
    return build([p], [0], [smp], 4, 31)
