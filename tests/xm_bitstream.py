"""A generator of FastTracker II XM 1.04 files for the XM tests: 1-32 channels, packed and unpacked pattern cells, patterns
of 1-256 rows, instruments with 0-16 samples and a note map, 8- and 16-bit samples (one-shot, forward and ping-pong loops,
loops down to a few samples, zero-length samples), envelopes with sustain and loop, fadeout, autovibrato, both frequency
tables, every effect and volume-column command libxm.d handles, pattern loops, breaks and jumps, endless songs and cut files."""
import struct

import numpy as np

EFFECTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0xA, 0xC, 0xF, 16, 17, 20, 21, 25, 27, 29, 33]
E_SUB = [1, 2, 4, 5, 7, 9, 0xA, 0xB, 0xC, 0xD]


def delta(values, bits):
    v = np.asarray(values, np.int64)
    d = np.diff(np.concatenate([[0], v]))
    return (d.astype(np.int16).astype("<i2") if bits == 16 else d.astype(np.int8)).tobytes()


def sample(data, bits=8, loop=0, loop_start=0, loop_length=0, volume=64, finetune=0, panning=128, relative=0):
    """One sample: data in sample units (int), loop 0 none / 1 forward / 2 ping-pong, loop in sample units."""
    return dict(data=list(data), bits=bits, loop=loop, loop_start=loop_start, loop_length=loop_length, volume=volume,
                finetune=finetune, panning=panning, relative=relative)


def envelope(points=(), sustain=None, loop=None, on=True):
    return dict(points=list(points), sustain=sustain, loop=loop, on=on)


def instrument(samples, note_map=None, vol_env=None, pan_env=None, fadeout=0, vibrato=(0, 0, 0, 0)):
    return dict(samples=list(samples), note_map=note_map or [0] * 96, vol_env=vol_env or envelope(on=False),
                pan_env=pan_env or envelope(on=False), fadeout=fadeout, vibrato=vibrato)


def pack_pattern(rows, channels, packed=True):
    """rows: list (per row) of dicts channel -> (note, instrument, volume, effect, param)."""
    out = bytearray()
    for row in rows:
        for c in range(channels):
            cell = row.get(c, (0, 0, 0, 0, 0))
            if packed:
                mask = 0x80 | sum(1 << i for i in range(5) if cell[i])
                out.append(mask)
                out.extend(b for b in cell if b)
            else:
                if cell[0] & 0x80:
                    raise ValueError("an unpacked cell's note must be below 128")
                out.extend(cell)
    return bytes(out)


def build(channels, order, patterns, instruments, linear=True, tempo=3, bpm=200, restart=0, packed=True, empty_patterns=()):
    """patterns: list of row lists (see pack_pattern); empty_patterns: indexes stored with a packed size of 0."""
    head = b"Extended Module: " + b"generated".ljust(20) + b"\x1a" + b"afgpu tests".ljust(20) + struct.pack("<H", 0x0104)
    table = bytes(order) + bytes(256 - len(order))
    head += struct.pack("<IHHHHHHHH", 276, len(order), restart, channels, len(patterns), len(instruments), 1 if linear else 0, tempo, bpm) + table
    body = bytearray()
    for i, rows in enumerate(patterns):
        data = b"" if i in empty_patterns else pack_pattern(rows, channels, packed if isinstance(packed, bool) else packed[i])
        body += struct.pack("<IBHH", 9, 0, len(rows), len(data)) + data
    for ins in instruments:
        n = len(ins["samples"])
        if n == 0:
            body += struct.pack("<I", 29) + b"empty".ljust(22) + b"\x00" + struct.pack("<H", 0)
            continue
        h = bytearray(263)
        struct.pack_into("<I", h, 0, 263)
        h[4:26] = b"instrument".ljust(22)
        struct.pack_into("<H", h, 27, n)
        struct.pack_into("<I", h, 29, 40)
        h[33:129] = bytes(ins["note_map"])
        for env, at, cnt, sus, flag in ((ins["vol_env"], 129, 225, 227, 233), (ins["pan_env"], 177, 226, 230, 234)):
            for j, (f, v) in enumerate(env["points"]):
                struct.pack_into("<HH", h, at + 4 * j, f, v)
            h[cnt] = len(env["points"])
            f = 1 if env["on"] else 0
            if env["sustain"] is not None:
                h[sus] = env["sustain"]
                f |= 2
            if env["loop"] is not None:
                h[sus + 1], h[sus + 2] = env["loop"]
                f |= 4
            h[flag] = f
        h[235], h[236], h[237], h[238] = ins["vibrato"]
        struct.pack_into("<H", h, 239, ins["fadeout"])
        body += h
        for s in ins["samples"]:
            w = 2 if s["bits"] == 16 else 1
            body += struct.pack("<IIIBbBBb", len(s["data"]) * w, s["loop_start"] * w, s["loop_length"] * w, s["volume"], s["finetune"],
                                s["loop"] | (16 if w == 2 else 0), s["panning"], s["relative"]) + b"\x00" + b"sample".ljust(22)
        for s in ins["samples"]:
            body += delta(s["data"], s["bits"])
    return head + bytes(body)


def random_sample(rng, kind):
    bits = 16 if rng.random() < 0.5 else 8
    n = int(rng.integers(3, 40)) if rng.random() < 0.3 else int(rng.integers(200, 3000))
    amp = 30000 if bits == 16 else 120
    data = (np.sin(np.arange(n) * rng.uniform(0.05, 0.9)) * amp * rng.uniform(0.3, 1)).astype(np.int64)
    if kind == 0:
        return sample(data, bits, volume=int(rng.integers(20, 65)), panning=int(rng.integers(0, 256)), finetune=int(rng.integers(-128, 128)),
                      relative=int(rng.integers(-12, 13)))
    ls = int(rng.integers(0, n - 2))
    ll = int(rng.integers(2, n - ls + 1))
    return sample(data, bits, kind, ls, ll, int(rng.integers(20, 65)), int(rng.integers(-128, 128)), int(rng.integers(0, 256)),
                  int(rng.integers(-12, 13)))


def random_song(rng, channels=None, linear=None, rows=None, n_patterns=2):
    """A song that exercises the whole control layer; it ends when the order wraps to a played row."""
    channels = channels or int(rng.integers(1, 9))
    linear = bool(rng.integers(0, 2)) if linear is None else linear
    instruments = []
    for k in range(int(rng.integers(2, 5))):
        n = int(rng.integers(1, 4))
        smp = [random_sample(rng, int(rng.integers(0, 3))) for _ in range(n)]
        if rng.random() < 0.2:
            smp.append(sample([], 8))
        ve = envelope([(0, 64), (4, 40), (10, 20), (30, 0)], sustain=1 if rng.random() < 0.5 else None,
                      loop=(1, 2) if rng.random() < 0.4 else None) if rng.random() < 0.6 else None
        pe = envelope([(0, 32), (6, 60), (14, 10)], loop=(0, 2) if rng.random() < 0.5 else None) if rng.random() < 0.5 else None
        instruments.append(instrument(smp, [int(rng.integers(0, len(smp) + (1 if rng.random() < 0.1 else 0))) for _ in range(96)], ve, pe,
                                      int(rng.integers(0, 4000)), (int(rng.integers(0, 5)), int(rng.integers(0, 20)),
                                                                   int(rng.integers(0, 16)), int(rng.integers(0, 64)))))
    if rng.random() < 0.3:
        instruments.append(instrument([]))
    patterns = []
    for p in range(n_patterns):
        nr = rows or int(rng.choice([1, 5, 16, 24]))
        pat = []
        for r in range(nr):
            row = {}
            for c in range(channels):
                if rng.random() < 0.55:
                    continue
                note = int(rng.integers(30, 70)) if rng.random() < 0.6 else (97 if rng.random() < 0.15 else 0)
                ins = int(rng.integers(1, len(instruments) + 2)) if rng.random() < 0.7 else 0
                vol = int(rng.integers(0x10, 0x100)) if rng.random() < 0.4 else 0
                fx = int(rng.choice(EFFECTS)) if rng.random() < 0.6 else 0
                par = int(rng.integers(0, 256)) if fx or rng.random() < 0.2 else 0
                if fx == 0xF:
                    par = int(rng.choice([2, 3, 4, 180, 220, 255]))
                if fx == 9:
                    par = int(rng.integers(0, 6))
                if rng.random() < 0.12:
                    fx, par = 0xE, (int(rng.choice(E_SUB)) << 4) | int(rng.integers(0, 16))
                row[c] = (note, ins, vol, fx, par)
            pat.append(row)
        patterns.append(pat)
    # one pattern loop, one break and one jump forward, placed where they cannot keep the song from ending
    if len(patterns[0]) >= 5:
        patterns[0][1][0] = (0, 0, 0, 0xE, 0x60)
        patterns[0][3][0] = (0, 0, 0, 0xE, 0x62)
    order = list(range(n_patterns)) + ([0] if n_patterns > 1 else [])
    if len(patterns[-1]) >= 5:
        patterns[-1][2][channels - 1] = (0, 0, 0, 0xD, 0x00)
    return build(channels, order, patterns, instruments, linear=linear, tempo=int(rng.integers(2, 5)), bpm=int(rng.integers(180, 256)),
                 packed=bool(rng.integers(0, 2)))


def endless_song():
    """One channel, one looped note and a header BPM of 0: the first tick's length is rate / (0 * 0.4) = infinity, so the
    tick never ends, no further row is read and the loop count stays 0."""
    smp = sample((np.sin(np.arange(64) * 0.3) * 100).astype(np.int64), 8, 2, 3, 50)
    rows = [{0: (49, 1, 0, 0, 0)}, {}]
    return build(1, [0], [rows], [instrument([smp])], tempo=6, bpm=0)


def single_note(volume=64, panning=128, bits=8):
    """One channel, one note whose real note number gives period 4608 (note 48: cell value 49, relative 0, finetune 0)."""
    n = 4000
    amp = 100 if bits == 8 else 20000
    data = (np.sin(np.arange(n) * 0.11) * amp).astype(np.int64)
    data[0] = amp // 2
    ins = instrument([sample(data, bits, 0, volume=volume, panning=panning)])
    rows = [{0: (49, 1, 0, 0, 0)}] + [{} for _ in range(3)]
    return build(1, [0], [rows], [ins], linear=True, tempo=6, bpm=125), data
