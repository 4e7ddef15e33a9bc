"""A literal float32 restatement of pocketmod.d (the reference's MOD player) in numpy: the independent model the MOD tests
compare the product with.  Each function cites the lines it restates.  The position chain is stepped sequentially
(np.add.accumulate over float32, one segment at a time): no closed form, so that the product's jump (csrc/mod_chain.h) is
checked against plain float adds.

render(frames) returns the mixed frames of one pocketmod_render call and records what it mixed (ticks, segments) in the
same shape as afg_mod_parse.  Bytes past the end of the file read 0 (the product's documented divergence)."""
import numpy as np

F = np.float32
RATE = 44100
MAX_FRAMES = 30 * 60 * 44100

# pocketmod.d:136-153
FINETUNE = [
    [0] * 36,
    [-6, -6, -5, -5, -4, -3, -3, -3, -3, -3, -3, -3, -3, -3, -2, -3, -2, -2, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0],
    [-12, -12, -10, -11, -8, -8, -7, -7, -6, -6, -6, -6, -6, -6, -5, -5, -4, -4, -4, -3, -3, -3, -3, -2, -3, -3, -2, -3, -3, -2, -2, -2, -2, -2, -2, -1],
    [-18, -17, -16, -16, -13, -12, -12, -11, -10, -10, -10, -9, -9, -9, -8, -8, -7, -6, -6, -5, -5, -5, -5, -4, -5, -4, -3, -4, -4, -3, -3, -3, -3, -2, -2, -2],
    [-24, -23, -21, -21, -18, -17, -16, -15, -14, -13, -13, -12, -12, -12, -11, -10, -9, -8, -8, -7, -7, -7, -7, -6, -6, -6, -5, -5, -5, -4, -4, -4, -4, -3, -3, -3],
    [-30, -29, -26, -26, -23, -21, -20, -19, -18, -17, -17, -16, -15, -14, -13, -13, -11, -11, -10, -9, -9, -9, -8, -7, -8, -7, -6, -6, -6, -5, -5, -5, -5, -4, -4, -4],
    [-36, -34, -32, -31, -27, -26, -24, -23, -22, -21, -20, -19, -18, -17, -16, -15, -14, -13, -12, -11, -11, -10, -10, -9, -9, -9, -7, -8, -7, -6, -6, -6, -6, -5, -5, -4],
    [-42, -40, -37, -36, -32, -30, -29, -27, -25, -24, -23, -22, -21, -20, -18, -18, -16, -15, -14, -13, -13, -12, -12, -10, -10, -10, -9, -9, -9, -8, -7, -7, -7, -6, -6, -5],
    [51, 48, 46, 42, 42, 38, 36, 34, 32, 30, 24, 27, 25, 24, 23, 21, 21, 19, 18, 17, 16, 15, 14, 14, 12, 12, 12, 10, 10, 10, 9, 8, 8, 8, 7, 7],
    [44, 42, 40, 37, 37, 35, 32, 31, 29, 27, 25, 24, 22, 21, 20, 19, 18, 17, 16, 15, 15, 14, 13, 12, 11, 10, 10, 9, 9, 9, 8, 7, 7, 7, 6, 6],
    [38, 36, 34, 32, 31, 30, 28, 27, 25, 24, 22, 21, 19, 18, 17, 16, 16, 15, 14, 13, 13, 12, 11, 11, 9, 9, 9, 8, 7, 7, 7, 6, 6, 6, 5, 5],
    [31, 30, 29, 26, 26, 25, 24, 22, 21, 20, 18, 17, 16, 15, 14, 13, 13, 12, 12, 11, 11, 10, 9, 9, 8, 7, 8, 7, 6, 6, 6, 5, 5, 5, 5, 5],
    [25, 24, 23, 21, 21, 20, 19, 18, 17, 16, 14, 14, 13, 12, 11, 10, 11, 10, 10, 9, 9, 8, 7, 7, 6, 6, 6, 5, 5, 5, 5, 4, 4, 4, 3, 4],
    [19, 18, 17, 16, 16, 15, 15, 14, 13, 12, 11, 10, 9, 9, 9, 8, 8, 18, 7, 7, 7, 6, 5, 6, 5, 4, 5, 4, 4, 4, 4, 3, 3, 3, 3, 3],
    [12, 12, 12, 10, 11, 11, 10, 10, 9, 8, 7, 7, 6, 6, 6, 5, 6, 5, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 2, 3, 3, 2, 2, 2, 2, 2],
    [6, 6, 6, 5, 6, 6, 6, 5, 5, 5, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1],
]
# pocketmod.d:185-199
PERIOD_NOTE = {p: i for i, p in enumerate([856, 808, 762, 720, 678, 640, 604, 570, 538, 508, 480, 453, 428, 404, 381, 360, 339, 320,
                                           302, 285, 269, 254, 240, 226, 214, 202, 190, 180, 170, 160, 151, 143, 135, 127, 120, 113])}
SIN = [0x00, 0x19, 0x32, 0x4a, 0x62, 0x78, 0x8e, 0xa2, 0xb4, 0xc5, 0xd4, 0xe0, 0xec, 0xf4, 0xfa, 0xfe]     # pocketmod.d:206-209
ARPEGGIO = [F(x) for x in (1.000000, 1.059463, 1.122462, 1.189207, 1.259921, 1.334840, 1.414214, 1.498307,
                           1.587401, 1.681793, 1.781797, 1.887749, 2.000000, 2.118926, 2.244924, 2.378414)]   # pocketmod.d:242-247
TAGS = {b"M.K.": 4, b"M!K!": 4, b"FLT4": 4, b"4CHN": 4, b"OKTA": 8, b"OCTA": 8, b"CD81": 8, b"FA08": 8}     # pocketmod.d:746-755
TAGS.update({b"%dCHN" % n: n for n in range(1, 10)})
TAGS.update({b"%dCH" % n: n for n in range(10, 33)})


def cvt_i32(x):
    """cast(int) of a float on x86-64 (cvttss2si): INT_MIN for NaN and out of range."""
    x = float(x)
    if not (-2147483904.0 < x < 2147483648.0):
        return -2147483648
    return int(x)


def s8(v):
    return ((int(v) + 128) & 0xff) - 128


def s16(v):
    return ((int(v) + 0x8000) & 0xffff) - 0x8000


def ident(data, size):
    """_pocketmod_ident (pocketmod.d:724-811): (channels, samples, length at, order at, patterns at) or None."""
    if size >= 1084:
        tag = bytes(data[1080:1084])
        if tag in TAGS:
            return TAGS[tag], 31, 950, 952, 1084
    if size < 600:
        return None
    ok = lambda c: c == 0 or 32 <= c <= 126
    if not all(ok(data[i]) for i in range(20)):
        return None
    if not all(ok(data[20 + i * 30 + j]) for i in range(15) for j in range(22)):
        return None
    return 4, 15, 470, 472, 600


def probe(data):
    """stream.d:1796-1830 behind the earlier probes: the product leaves RIFF/WAVE files and XM headers to those formats."""
    data = bytes(data)
    if len(data) < 600:
        return False
    if len(data) >= 12 and data[:4] == b"RIFF" and data[8:12] == b"WAVE":
        return False
    if len(data) >= 60 and data[:17] == b"Extended Module: " and data[37] == 0x1A and data[58] == 4 and data[59] == 1:
        return False
    if ident(data, min(len(data), 1084)) is None:
        return False
    return Mod.init(data) is not None


class Chan:
    def __init__(self):
        self.dirty = self.sample = self.volume = self.balance = 0
        self.period = self.delayed = self.target = 0
        self.finetune = self.loop_count = self.loop_line = self.lfo_step = 0
        self.lfo_type = [0, 0]
        self.effect = self.param = self.param3 = self.param4 = self.param7 = self.param9 = 0
        self.paramE1 = self.paramE2 = self.paramEA = self.paramEB = self.real_volume = 0
        self.position = F(0)
        self.increment = F(0)


class Mod:
    PITCH, VOLUME = 1, 2

    @classmethod
    def init(cls, data):
        """pocketmod_init (pocketmod.d:813-906), rate 44100; None when refused."""
        data = bytes(data)
        size = len(data)
        if size <= 0:
            return None
        idn = ident(data, size)
        if idn is None:
            return None
        m = cls()
        m.data = data
        m.size = size
        m.num_channels, m.num_samples, la, m.order_at, m.patterns_at = idn
        m.length, m.reset = data[la], data[la + 1]
        if m.length == 0 or m.length > 128:
            return None
        if m.reset >= m.length:
            m.reset = 0
        npat = 0
        i = 0
        while i < 128 and data[m.order_at + i] < 128:
            npat = max(npat, data[m.order_at + i])
            i += 1
        m.num_patterns = npat + 1
        pattern_bytes = 256 * m.num_channels * m.num_patterns
        header = m.patterns_at
        for i in range(m.length):
            if header + 256 * m.num_channels * data[m.order_at + i] > size:
                return None
        if header + pattern_bytes > size:
            return None
        remaining = size - header - pattern_bytes
        area = header + pattern_bytes
        m.plane = np.frombuffer(data[area:] + bytes(16), np.uint8).view(np.int8)
        m.sample_off, m.sample_len = [], []
        off = 0
        for i in range(m.num_samples):
            h = 12 + 30 * (i + 1)
            length = ((data[h] << 8) | data[h + 1]) << 1
            ln = min(length if length > 2 else 0, remaining)
            m.sample_off.append(off)
            m.sample_len.append(ln)
            off += ln
            remaining -= ln
        while len(m.sample_off) < 31:
            m.sample_off.append(off)
            m.sample_len.append(0)
        m.ch = [Chan() for _ in range(32)]
        for i in range(m.num_channels):
            m.ch[i].balance = 0x80 + (0x20 if (((i + 1) >> 1) & 1) else -0x20)
        m.ticks_per_line = 6
        m.samples_per_tick = F(RATE) / F(50.0)
        m.lfo_rng = 0xbadc0de
        m.visited = [0] * 32
        m.loop_count = 0
        m.pattern_delay = 0
        m.pattern = 0
        m.line = -1
        m.tick = m.ticks_per_line - 1
        m.sample = F(0)
        m.next_tick()
        return m

    def byte(self, off):
        return self.data[off] if 0 <= off < self.size else 0

    # ---- control layer ----
    def lfo(self, ch, step):                                        # pocketmod.d:216-225
        t = ch.lfo_type[1 if ch.effect == 7 else 0] & 3
        if t == 0:
            step &= 0x3f
            x = SIN[step & 0x0f]
            x = x if (step & 0x1f) < 0x10 else 0xff - x
            return x if step < 0x20 else -x
        if t == 1:
            return 0xff - ((step & 0x3f) << 3)
        if t == 2:
            return 0xff if (step & 0x3f) < 0x20 else -0xff
        return (self.lfo_rng & 0x1ff) - 0xff

    def update_pitch(self, ch):                                     # pocketmod.d:227-258
        ch.increment = F(0)
        if ch.period:
            period = F(ch.period)
            if ch.effect in (4, 6):
                step = (ch.param4 >> 4) * ch.lfo_step
                rate = ch.param4 & 0x0f
                period = F(period + F(F(self.lfo(ch, step) * rate) / F(128.0)))
            elif ch.effect == 0 and ch.param:
                tick_mod = int(np.fmod(self.tick, 3))               # D's % truncates
                step = (ch.param >> ((2 - tick_mod) << 2)) & 0x0f
                period = F(period / ARPEGGIO[step])
            ch.increment = F(F(3546894.6) / F(period * F(RATE)))
        ch.dirty &= ~self.PITCH

    def update_volume(self, ch):                                    # pocketmod.d:260-269
        volume = ch.volume
        if ch.effect == 7:
            step = ch.lfo_step * (ch.param7 >> 4)
            volume += (self.lfo(ch, step) * (ch.param7 & 0x0f)) >> 6
        ch.real_volume = min(max(volume, 0), 0x40)
        ch.dirty &= ~self.VOLUME

    def pitch_slide(self, ch, amount):                              # pocketmod.d:271-279
        hi = 856 + FINETUNE[ch.finetune][0]
        lo = 113 + FINETUNE[ch.finetune][35]
        ch.period = (ch.period + amount) & 0xffff
        ch.period = max(ch.period, lo) & 0xffff
        ch.period = min(ch.period, hi) & 0xffff
        ch.dirty |= self.PITCH

    def volume_slide(self, ch, param):                              # pocketmod.d:281-288
        change = (param >> 4) if (param & 0xf0) else -(param & 0x0f)
        ch.volume = min(max(ch.volume + change, 0), 0x40)
        ch.dirty |= self.VOLUME

    def order(self, p):
        return self.byte(self.order_at + p)

    def next_line(self):                                            # pocketmod.d:354-530
        pattern_break = -1
        if self.line == 0:
            self.visited[(self.pattern & 0xff) >> 3] |= 1 << (self.pattern & 7)
        self.line = s8(self.line + 1)
        if self.line == 64:
            self.pattern = s8(self.pattern + 1)
            if self.pattern == self.length:
                self.pattern = self.reset
            self.line = 0
        pos = self.patterns_at + (self.order(self.pattern) * 64 + self.line) * self.num_channels * 4
        for i in range(self.num_channels):
            b0, b1, b2, b3 = (self.byte(pos + 4 * i + k) for k in range(4))
            sample = (b0 & 0xf0) | (b2 >> 4)
            period = ((b0 & 0x0f) << 8) | b1
            effect = ((b2 & 0x0f) << 8) | b3
            ch = self.ch[i]
            ch.effect = (effect >> 8) if (effect >> 8) != 0xe else (effect >> 4)
            ch.param = (effect & 0xff) if (effect >> 8) != 0xe else (effect & 0x0f)
            if sample:
                if sample <= 31:
                    h = 12 + 30 * sample
                    ch.sample = sample
                    ch.finetune = self.byte(h + 2) & 0x0f
                    ch.volume = min(self.byte(h + 3), 0x40)
                    if ch.effect != 0xED:
                        ch.dirty |= self.VOLUME
                else:
                    ch.sample = 0
            if period:
                note = PERIOD_NOTE.get(period, 0)
                period += FINETUNE[ch.finetune][note]
                if ch.effect != 0x3:
                    if ch.effect != 0xED:
                        ch.period = period & 0xffff
                        ch.dirty |= self.PITCH
                        ch.position = F(0)
                        ch.lfo_step = 0
                    else:
                        ch.delayed = period & 0xffff
            e, p = ch.effect, ch.param
            mem = lambda dst, src: src if src else dst
            if e == 0x3:
                ch.param3 = mem(ch.param3, p)
            if e in (0x3, 0x5):
                ch.target = mem(ch.target, period & 0xffff)
            elif e in (0x4, 0x7):
                old = ch.param4 if e == 4 else ch.param7
                new = ((p & 0x0f) or (old & 0x0f)) | ((p & 0xf0) or (old & 0xf0))
                if e == 4:
                    ch.param4 = new
                else:
                    ch.param7 = new
            elif e == 0xE1:
                ch.paramE1 = mem(ch.paramE1, p)
            elif e == 0xE2:
                ch.paramE2 = mem(ch.paramE2, p)
            elif e == 0xEA:
                ch.paramEA = mem(ch.paramEA, p)
            elif e == 0xEB:
                ch.paramEB = mem(ch.paramEB, p)
            elif e == 0x8:
                ch.balance = p
            elif e == 0x9:
                if period != 0 or sample != 0:
                    ch.param9 = p if p else ch.param9
                    ch.position = F(ch.param9 << 8)
            elif e == 0xB:
                self.pattern = p if p < self.length else 0
                self.line = -1
            elif e == 0xC:
                ch.volume = min(max(p, 0), 0x40)
                ch.dirty |= self.VOLUME
            elif e == 0xD:
                pattern_break = (p >> 4) * 10 + (p & 15)
            elif e == 0xE4:
                ch.lfo_type[0] = p
            elif e == 0xE5:
                ch.finetune = p
                ch.dirty |= self.PITCH
            elif e == 0xE6:
                if p:
                    if not ch.loop_count:
                        ch.loop_count = p
                        self.line = s8(ch.loop_line)
                    else:
                        ch.loop_count = (ch.loop_count - 1) & 0xff
                        if ch.loop_count:
                            self.line = s8(ch.loop_line)
                else:
                    ch.loop_line = (self.line - 1) & 0xff
            elif e == 0xE7:
                ch.lfo_type[1] = p
            elif e == 0xE8:
                ch.balance = (p << 4) & 0xff
            elif e == 0xEE:
                self.pattern_delay = p
            elif e == 0xF:
                if p:
                    if p < 0x20:
                        self.ticks_per_line = p
                    else:
                        self.samples_per_tick = F(F(RATE) / F(F(0.4) * F(p)))
        if pattern_break != -1:
            self.line = s8((pattern_break if pattern_break < 64 else 0) - 1)
            self.pattern = s8(self.pattern + 1)
            if self.pattern == self.length:
                self.pattern = self.reset

    def next_tick(self):                                            # pocketmod.d:532-662
        self.tick = s16(self.tick + 1)
        if self.tick == self.ticks_per_line:
            if self.pattern_delay > 0:
                self.pattern_delay -= 1
            else:
                self.next_line()
            self.tick = 0
        for i in range(self.num_channels):
            ch = self.ch[i]
            param = ch.param
            self.lfo_rng = (0x0019660d * self.lfo_rng + 0x3c6ef35f) & 0xffffffff
            e = ch.effect
            if e == 0x0:
                ch.dirty |= self.PITCH
            elif e == 0xE9:
                if not (param and int(np.fmod(self.tick, param))):
                    ch.position = F(0)
                    ch.lfo_step = 0
            elif e == 0xEC:
                if self.tick == param:
                    ch.volume = 0
                    ch.dirty |= self.VOLUME
            elif e == 0xED:
                if self.tick == param and ch.sample:
                    ch.dirty |= self.VOLUME | self.PITCH
                    ch.period = ch.delayed
                    ch.position = F(0)
                    ch.lfo_step = 0
            if self.tick == 0:
                if e == 0xE1:
                    self.pitch_slide(ch, -ch.paramE1)
                elif e == 0xE2:
                    self.pitch_slide(ch, ch.paramE2)
                elif e == 0xEA:
                    self.volume_slide(ch, ch.paramEA << 4)
                elif e == 0xEB:
                    self.volume_slide(ch, ch.paramEB & 15)
            else:
                if e == 0x1:
                    self.pitch_slide(ch, -param)
                elif e == 0x2:
                    self.pitch_slide(ch, param)
                elif e in (0x3, 0x5):
                    if e == 0x5:
                        self.volume_slide(ch, param)
                    rate = ch.param3
                    order = int(ch.period < ch.target)
                    closer = ch.period + (rate if order else -rate)
                    new_order = int(closer < ch.target)
                    ch.period = (closer if new_order == order else ch.target) & 0xffff
                    ch.dirty |= self.PITCH
                elif e in (0x4, 0x6):
                    if e == 0x6:
                        self.volume_slide(ch, param)
                    ch.lfo_step = (ch.lfo_step + 1) & 0xff
                    ch.dirty |= self.PITCH
                elif e == 0x7:
                    ch.lfo_step = (ch.lfo_step + 1) & 0xff
                    ch.dirty |= self.VOLUME
                elif e == 0xA:
                    self.volume_slide(ch, param)
            if ch.dirty & self.VOLUME:
                self.update_volume(ch)
            if ch.dirty & self.PITCH:
                self.update_pitch(ch)

    # ---- mixer ----
    def render_channel(self, index, ch, out, at, frames):           # pocketmod.d:664-721
        s = ch.sample - 1
        h = 12 + 30 * ch.sample
        loop_start = ((self.byte(h + 4) << 8) | self.byte(h + 5)) << 1
        loop_length = ((self.byte(h + 6) << 8) | self.byte(h + 7)) << 1
        loop_end = loop_start + loop_length if loop_length > 2 else 0xffffff
        length = self.sample_len[s]
        sample_end = F(1 + min(loop_end, length))
        volume = F(F(ch.real_volume) / F(128 * 64 * 4))
        level_l = F(volume * F(F(1.0) - F(F(ch.balance) / F(255.0))))
        level_r = F(volume * F(F(0.0) + F(F(ch.balance) / F(255.0))))
        left = frames
        while True:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                num = cvt_i32(F(F(sample_end - ch.position) / ch.increment))
            num = min(num, left)
            if num > 0:
                self.segments.append((at, num, ch.position, ch.increment, level_l, level_r, self.sample_off[s], loop_start,
                                      loop_length, loop_end, length, index))
                steps = np.full(num + 1, ch.increment, np.float32)
                steps[0] = ch.position
                pos = np.add.accumulate(steps, dtype=np.float32)            # sequential float32 adds
                x0 = pos[:num].astype(np.int64)                             # positions are >= 0: truncation
                idx = self.sample_off[s] + x0
                ok = (x0 >= 0) & (idx < len(self.plane))
                smp = np.where(ok, self.plane[np.minimum(idx, len(self.plane) - 1)], 0).astype(np.float32)
                out[at:at + num, 0] = out[at:at + num, 0] + level_l * smp
                out[at:at + num, 1] = out[at:at + num, 1] + level_r * smp
                ch.position = pos[num]
                at += num
            if ch.position >= F(loop_end):
                ch.position = F(ch.position - F(loop_length))
            elif ch.position >= F(length):
                ch.position = F(-1.0)
                break
            left -= num
            if not num > 0:
                break

    def render(self, frames):
        """pocketmod_render(c, buffer, frames * 8) (pocketmod.d:908-952): (float32 [n, 2]); ticks and segments of the call
        in self.ticks / self.segments (frames relative to the call)."""
        out = np.zeros((frames, 2), np.float32)
        self.ticks, self.segments = [], []
        rendered, remaining = 0, frames
        while remaining > 0:
            num = cvt_i32(F(self.samples_per_tick - self.sample))
            num = min(num + (1 if num == 0 else 0), remaining)
            seg0 = len(self.segments)
            tick_rec = [rendered, num, seg0, 0, self.pattern, self.line]
            for i in range(self.num_channels):
                ch = self.ch[i]
                if ch.sample != 0 and ch.position >= F(0):
                    self.render_channel(i, ch, out, rendered, num)
            tick_rec[3] = len(self.segments) - seg0
            self.ticks.append(tuple(tick_rec))
            remaining -= num
            rendered += num
            self.sample = F(self.sample + F(num))
            if self.sample >= self.samples_per_tick:
                self.sample = F(self.sample - self.samples_per_tick)
                self.next_tick()
                if self.line == 0 and self.tick == 0:
                    if self.visited[(self.pattern & 0xff) >> 3] & (1 << (self.pattern & 7)):
                        self.visited = [0] * 32
                        self.loop_count += 1
                    break
        return out[:rendered]

    def seek(self, pattern, row, tick=0):                           # pocketmod.d:954-962
        self.line = s8(row)
        self.pattern = s8(pattern)
        self.tick = s16(tick)
        self.sample = F(0)


def read(mod, frames):
    """AudioStream.readSamplesFloat for a MOD (stream.d:611-620)."""
    if mod.loop_count >= 1:
        return np.zeros((0, 2), np.float32)
    return mod.render(frames)


def decode_stream(data, read_sizes, max_frames=None):
    """The stream read by read: read_sizes cycles; returns the concatenated frames."""
    m = Mod.init(data)
    assert m is not None
    parts, total, k = [], 0, 0
    while True:
        want = read_sizes[k % len(read_sizes)]
        if max_frames is not None:
            want = min(want, max_frames - total)
            if want <= 0:
                break
        got = read(m, want)
        k += 1
        if len(got) == 0:
            break
        parts.append(got)
        total += len(got)
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)


def decode_batch(data, cap=MAX_FRAMES, keep_records=False):
    """The batch path's definition (afg.h): reads of cap minus the frames so far until the song loops or the cap is
    reached.  Returns (frames [n, 2], capped, ticks, segments) with song-relative frames."""
    m = Mod.init(data)
    parts, ticks, segs, total, capped = [], [], [], 0, False
    while True:
        if m.loop_count >= 1:
            break
        if total >= cap:
            capped = True
            break
        got = m.render(cap - total)
        if len(got) == 0:
            break
        if keep_records:
            base = len(segs)
            ticks += [(t[0] + total, t[1], t[2] + base, t[3], t[4], t[5]) for t in m.ticks]
            segs += [(s[0] + total,) + s[1:] for s in m.segments]
        parts.append(got)
        total += len(got)
    out = np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)
    return out, capped, ticks, segs
