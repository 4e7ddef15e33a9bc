"""A sequential restatement of libxm.d as stream.d drives it (44100 Hz, stereo, max loop count 1), in numpy float32 scalars:
every position, volume ramp and frame_count is stepped one frame at a time, with no closed form and no segments, so that the
product's records and jumps are tested against plain stepping.  pow, sin and sqrt go through the C library (ctypes), the same
functions the product calls: exp2 and sin in double rounded once, sqrtf.

decode_stream(data, reads) -> (list of float32 [n, 2] arrays, one per read; Player); decode_batch(data) -> float32 [n, 2].
Where libxm.d reads outside its arrays the model follows the product's documented choices."""
import ctypes
import ctypes.util
import math

import numpy as np

_m = ctypes.CDLL(ctypes.util.find_library("m"))
_m.exp2.restype = _m.sin.restype = ctypes.c_double
_m.exp2.argtypes = _m.sin.argtypes = [ctypes.c_double]
_m.sqrtf.restype = ctypes.c_float
_m.sqrtf.argtypes = [ctypes.c_float]

F = np.float32
RATE = 44100
MAX_FRAMES = 30 * 60 * 44100
AMIGA = [1712 * 1024, 1616 * 1024, 1525 * 1024, 1440 * 1024, 1357 * 1024, 1281 * 1024, 1209 * 1024, 1141 * 1024, 1077 * 1024,
         1017 * 1024, 961 * 1024, 907 * 1024, 856 * 1024]
RETRIG_ADD = [0, -1, -2, -4, -8, -16, 0, 0, 0, 1, 2, 4, 8, 16, 0, 0]
RETRIG_MUL = [F(1)] * 6 + [F(.6666667), F(.5)] + [F(1)] * 6 + [F(1.5), F(2)]
np.seterr(all="ignore")


def sqrtf(x):
    return F(_m.sqrtf(float(x)))


def i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def shl(v, n):
    return i32(v << (n & 31))


def shr(v, n):
    return v >> (n & 31)


def slide(val, goal, incr):
    if val > goal:
        val = F(val - incr)
        if val < goal:
            val = goal
    elif val < goal:
        val = F(val + incr)
        if val > goal:
            val = goal
    return val


def lerp(u, v, t):
    return F(u + F(t * F(v - u)))


class Obj:
    pass


def load(data):
    """xm_create_context_safe: the module, or None when refused."""
    n = len(data)
    if n < 60 or data[:17] != b"Extended Module: " or data[37] != 0x1A or data[59] != 1 or data[58] != 4:
        return None
    u8 = lambda o: data[o] if o < n else 0
    u16 = lambda o: u8(o) | (u8(o + 1) << 8)
    u32 = lambda o: u16(o) | (u16(o + 2) << 16)
    m = Obj()
    off = 60
    m.length, m.restart, m.channels, npat, nins = u16(off + 4), u16(off + 6), u16(off + 8), u16(off + 10), u16(off + 12)
    if m.length == 0 or m.length >= 256 or m.restart >= m.length or m.channels == 0 or m.channels > 32:
        return None
    # the product's budget on what a file may declare
    budget = (16 << 20) + 16 * n
    need = npat * 16 + nins * 512 + 256 * m.length
    o = off + u32(off)
    for _ in range(npat):
        if need > budget:
            break
        rows = u16(o + 5)
        if rows > 256:
            return None
        need += rows * m.channels * 5
        o += u32(o) + u16(o + 7)
    for _ in range(nins):
        if need > budget:
            break
        ns = u16(o + 27)
        hs = u32(o)
        if hs == 0 or hs > 263:
            hs = 263
        o += hs
        agg = 0
        for _ in range(ns):
            if need > budget:
                break
            agg = (agg + u32(o)) & 0xFFFFFFFF
            need += u32(o) + 64
            o += 40
        o += agg
    if need > budget:
        return None
    hsize = u32(off)
    m.linear = bool(u32(off + 14) & 1)
    m.tempo, m.bpm = u16(off + 16), u16(off + 18)
    m.table = [u8(off + 20 + i) for i in range(256)]
    off += hsize
    m.patterns = []
    for _ in range(npat):
        packed = u16(off + 7)
        rows = u16(off + 5)
        slots = [[0, 0, 0, 0, 0] for _ in range(rows * m.channels)]
        off += u32(off)
        j = k = 0
        while j < packed:
            note = u8(off + j)
            cell = [0, 0, 0, 0, 0]
            if note & 0x80:
                j += 1
                for b in range(5):
                    if note & (1 << b):
                        cell[b] = u8(off + j)
                        j += 1
            else:
                cell = [note, u8(off + j + 1), u8(off + j + 2), u8(off + j + 3), u8(off + j + 4)]
                j += 5
            if k < len(slots):
                slots[k] = cell
            k += 1
        off += packed
        m.patterns.append((rows, slots))
    m.instruments = []
    for _ in range(nins):
        ins = Obj()
        hs = u32(off)
        if hs == 0 or hs > 263:
            hs = 263
        bound = off + hs
        u8b = lambda o: data[o] if (o < bound and o < n) else 0
        ins.num_samples = u16(off + 27)
        ins.samples = []
        if ins.num_samples:
            ins.map = [u8b(off + 33 + j) for j in range(96)]
            envs = []
            for at, cnt, sus, flag in ((129, 225, 227, 233), (177, 226, 230, 234)):
                e = Obj()
                e.n = min(u8b(off + cnt), 12)
                e.frame = [u16(off + at + 4 * j) for j in range(e.n)] + [0] * (12 - e.n)
                e.value = [u16(off + at + 4 * j + 2) for j in range(e.n)] + [0] * (12 - e.n)
                e.sustain, e.ls, e.le = u8b(off + sus), u8b(off + sus + 1), u8b(off + sus + 2)
                f = u8b(off + flag)
                e.on, e.sustain_on, e.loop_on = bool(f & 1), bool(f & 2), bool(f & 4)
                envs.append(e)
            ins.venv, ins.penv = envs
            ins.vib_type = {1: 2, 2: 1}.get(u8b(off + 235), u8b(off + 235))
            ins.vib_sweep, ins.vib_depth, ins.vib_rate = u8b(off + 236), u8b(off + 237), u8b(off + 238)
            ins.fadeout = u16(off + 239)
        off += hs
        for _ in range(ins.num_samples):
            s = Obj()
            s.length, s.loop_start, ll = u32(off), u32(off + 4), u32(off + 8)
            s.loop_end = (s.loop_start + ll) & 0xFFFFFFFF
            s.volume = F(F(u8(off + 12)) / F(0x40))
            s.finetune = u8(off + 13) - 256 if u8(off + 13) > 127 else u8(off + 13)
            s.loop_start = min(s.loop_start, s.length)
            s.loop_end = min(s.loop_end, s.length)
            s.loop_length = (s.loop_end - s.loop_start) & 0xFFFFFFFF
            f2 = u8(off + 14)
            s.loop = 0 if ((f2 & 3) == 0 or s.loop_length == 0) else (1 if (f2 & 3) == 1 else 2)
            s.bits = 16 if f2 & 16 else 8
            s.panning = F(F(u8(off + 15)) / F(0xFF))
            s.relative = u8(off + 16) - 256 if u8(off + 16) > 127 else u8(off + 16)
            if s.bits == 16:
                s.loop_start >>= 1; s.loop_length >>= 1; s.loop_end >>= 1; s.length >>= 1
            ins.samples.append(s)
            off += 40
        for s in ins.samples:
            w = 2 if s.bits == 16 else 1
            raw = np.zeros(s.length * w, np.uint8)
            have = data[off:off + s.length * w] if off < n else b""
            raw[:len(have)] = np.frombuffer(have, np.uint8)
            if w == 2:
                s.data = np.cumsum(raw.view("<u2").astype(np.uint16), dtype=np.uint16).view(np.int16)
                s.scale = F(32768)
            else:
                s.data = np.cumsum(raw, dtype=np.uint8).view(np.int8)
                s.scale = F(128)
            off += s.length * w
        m.instruments.append(ins)
    for i in range(m.length):
        if m.table[i] >= npat:
            if i + 1 == m.length and m.length > 1:
                m.length -= 1
            else:
                return None
    if m.restart >= m.length:
        return None
    m.num_patterns = npat
    return m


class Chan:
    def __init__(self):
        self.note = self.orig_note = F(0)
        self.instrument = self.sample = None
        self.cur = [0, 0, 0, 0, 0]
        self.pos = self.period = self.freq = self.step = F(0)
        self.ping = True
        self.volume, self.panning = F(1), F(.5)
        self.av_ticks = 0
        self.sustained = False
        self.fadeout, self.venv_v, self.penv_p = F(1), F(1), F(.5)
        self.venv_c = self.penv_c = 0
        self.av_off = F(0)
        self.arp, self.arp_off = False, 0
        self.vs = self.fvs = self.gvs = self.ps = self.pu = self.pd = self.fpu = self.fpd = self.xpu = self.xpd = self.tp = 0
        self.tp_target = F(0)
        self.retrig = self.delay = self.loop_origin = self.loop_n = 0
        self.vib, self.vib_wave, self.vib_retrig, self.vib_param, self.vib_ticks, self.vib_off = False, 0, True, 0, 0, F(0)
        self.trem_wave, self.trem_retrig, self.trem_param, self.trem_ticks, self.trem_vol = 0, True, 0, 0, F(0)
        self.tremor, self.tremor_on = 0, False
        self.target = [F(0), F(0)]
        self.fc = 0
        self.prev = [F(0)] * 32
        self.actual = [F(0), F(0)]


def tone_porta(c):
    return c[3] == 3 or c[3] == 5 or (c[2] >> 4) == 0xF


def has_vib(c):
    return c[3] == 4 or c[3] == 6 or (c[2] >> 4) == 0xB


def cvt_i32(x):
    if not (x > -2147483904.0 and x < 2147483648.0):
        return -(1 << 31)
    return int(x)


class Player:
    def __init__(self, m):
        self.m = m
        self.tempo, self.bpm = m.tempo, m.bpm
        self.gvol = F(1)
        self.rand = 24492
        self.index = self.row = self.tick_n = 0
        self.remaining = F(0)
        self.pjump = self.pbreak = False
        self.jdest = self.jrow = self.extra = 0
        self.visits = [0] * (256 * m.length)
        self.loop_count = 0
        self.ch = [Chan() for _ in range(m.channels)]
        self.ticks = []                                     # (frames, scale, index, row, loop_count) per tick piece

    # ---- frequencies ----
    def amiga_period(self, note):
        intnote = int(note) & 0xFFFFFFFF
        a = intnote % 12
        octave = ((cvt_i32(F(F(note / F(12)) - F(2))) + 128) & 255) - 128
        p1, p2 = AMIGA[a], AMIGA[a + 1]
        if octave > 0:
            p1, p2 = shr(p1, octave), shr(p2, octave)
        elif octave < 0:
            p1, p2 = shl(p1, -octave), shl(p2, -octave)
        return F(lerp(F(p1), F(p2), F(note - F(intnote))) / F(1024))

    def period_of(self, note):
        return F(F(7680) - F(note * F(64))) if self.m.linear else self.amiga_period(note)

    @staticmethod
    def amiga_freq(period):
        return F(0) if period == 0 else F(F(7093789.2) / F(period * F(2)))

    def frequency(self, period, note_off, period_off):
        if self.m.linear:
            p = F(F(period - F(F(64) * note_off)) - F(F(16) * period_off))
            return F(F(8363) * F(_m.exp2(float(F(F(F(4608) - p) / F(768))))))
        if note_off == 0:
            return self.amiga_freq(F(period + F(F(16) * period_off)))
        a = octave = 0
        period = F(period * F(1024))
        if period > F(AMIGA[0]):
            octave -= 1
            while octave > -31 and period > F((AMIGA[0] << ((-octave) & 31)) & 0xFFFFFFFF):
                octave -= 1
        elif period < F(AMIGA[12]):
            octave += 1
            while octave < 31 and period < F(AMIGA[12] >> (octave & 31)):
                octave += 1
        p1 = p2 = 0
        for i in range(12):
            p1, p2 = AMIGA[i], AMIGA[i + 1]
            if octave > 0:
                p1, p2 = shr(p1, octave), shr(p2, octave)
            elif octave < 0:
                p1, p2 = shl(p1, -octave), shl(p2, -octave)
            if F(p2) <= period <= F(p1):
                a = i
                break
        note = F(F(F(12) * F(octave + 2)) + F(a)) + F(F(period - F(p1)) / F(F(p2) - F(p1)))
        return self.amiga_freq(F(self.amiga_period(F(F(note) + note_off)) + F(F(16) * period_off)))

    def update_freq(self, ch):
        ch.freq = self.frequency(ch.period, F(ch.arp_off), F(ch.vib_off + ch.av_off))
        ch.step = F(ch.freq / F(RATE))

    def waveform(self, kind, step):
        step %= 0x40
        if kind == 0:
            return F(-F(_m.sin(float(F(F(F(F(2) * F(3.141592)) * F(step)) / F(0x40))))))
        if kind == 1:
            return F(F(0x20 - step) / F(0x20))
        if kind == 2:
            return F(1) if step >= 0x20 else F(-1)
        if kind == 3:
            self.rand = (self.rand * 1103515245 + 12345) & 0xFFFFFFFF
            return F(F(F((self.rand >> 16) & 0x7FFF) / F(0x4000)) - F(1))
        if kind == 4:
            return F(F(step - 0x20) / F(0x20))
        return F(0)

    def autovibrato(self, ch):
        ins = ch.instrument
        if ins is None or ins.num_samples == 0 or ins.vib_depth == 0:
            if ch.av_off != 0:
                ch.av_off = F(0)
                self.update_freq(ch)
            return
        sweep = F(1)
        if ch.av_ticks < ins.vib_sweep:
            sweep = lerp(F(0), F(1), F(F(ch.av_ticks) / F(ins.vib_sweep)))
        step = (ch.av_ticks * ins.vib_rate) >> 2
        ch.av_ticks = (ch.av_ticks + 1) & 0xFFFF
        ch.av_off = F(F(F(F(.25) * self.waveform(ins.vib_type, step & 255)) * F(ins.vib_depth)) / F(0xF)) * sweep
        ch.av_off = F(ch.av_off)
        self.update_freq(ch)

    def vibrato(self, ch, param):
        ch.vib_ticks = (ch.vib_ticks + (param >> 4)) & 0xFFFF
        ch.vib_off = F(F(F(F(-2) * self.waveform(ch.vib_wave, ch.vib_ticks & 255)) * F(param & 15)) / F(0xF))
        self.update_freq(ch)

    def pitch_slide(self, ch, off):
        off = F(off)
        if self.m.linear:
            off = F(off * F(4))
        ch.period = F(ch.period + off)
        if ch.period < 0:
            ch.period = F(0)
        self.update_freq(ch)

    def tone_portamento(self, ch):
        if ch.tp_target == 0:
            return
        if ch.period != ch.tp_target:
            ch.period = slide(ch.period, ch.tp_target, F(F(4 if self.m.linear else 1) * F(ch.tp)))
            self.update_freq(ch)

    @staticmethod
    def vslide(v, raw, unit=0x40):
        raw &= 255
        if (raw & 0xF0) and (raw & 0x0F):
            return v
        if raw & 0xF0:
            v = F(v + F(F(raw >> 4) / F(unit)))
            return F(1) if v > 1 else v
        v = F(v - F(F(raw & 15) / F(unit)))
        return F(0) if v < 0 else v

    # ---- notes ----
    def trigger(self, ch, keep_vol=False, keep_period=False, keep_pos=False, keep_env=False):
        if not keep_pos:
            ch.pos, ch.ping = F(0), True
        if ch.sample is not None:
            if not keep_vol:
                ch.volume = ch.sample.volume
            ch.panning = ch.sample.panning
        if not keep_env:
            ch.sustained = True
            ch.fadeout = ch.venv_v = F(1)
            ch.penv_p = F(.5)
            ch.venv_c = ch.penv_c = 0
        ch.vib_off = ch.trem_vol = F(0)
        ch.tremor_on = False
        ch.av_ticks = 0
        if ch.vib_retrig:
            ch.vib_ticks = 0
        if ch.trem_retrig:
            ch.trem_ticks = 0
        if not keep_period:
            ch.period = self.period_of(ch.note)
            self.update_freq(ch)

    @staticmethod
    def key_off(ch):
        ch.sustained = False
        if ch.instrument is None or ch.instrument.num_samples == 0 or not ch.instrument.venv.on:
            ch.volume = F(0)

    def note_value(self, note, smp, finetune=None):
        ft = smp.finetune if finetune is None else finetune
        return F(F(F(note + smp.relative) + F(F(ft) / F(128))) - F(1))

    def handle(self, ch, s):
        m = self.m
        note, insn, vc, fx, p = s
        if insn > 0:
            if tone_porta(ch.cur) and ch.instrument is not None and ch.sample is not None:
                self.trigger(ch, keep_period=True, keep_pos=True)
            elif note == 0 and ch.sample is not None:
                self.trigger(ch, keep_pos=True)
            elif insn > len(m.instruments):
                ch.volume = F(0)
                ch.instrument = ch.sample = None
            else:
                ch.instrument = m.instruments[insn - 1]
        if 0 < note < 97:
            ins = ch.instrument
            if tone_porta(ch.cur) and ins is not None and ch.sample is not None:
                ch.note = self.note_value(note, ch.sample)
                ch.tp_target = self.period_of(ch.note)
            elif ins is None or ins.num_samples == 0:
                ch.volume = F(0)
            elif ins.map[note - 1] < ins.num_samples:
                for z in range(32):
                    ch.prev[z] = self.next_of_sample(ch)
                ch.fc = 0
                ch.sample = ins.samples[ins.map[note - 1]]
                ch.orig_note = ch.note = self.note_value(note, ch.sample)
                self.trigger(ch, keep_vol=not insn > 0)
            else:
                ch.volume = F(0)
        elif note == 97:
            self.key_off(ch)
        hi = vc >> 4
        if 1 <= hi <= 4 or (hi == 5 and vc <= 0x50):
            ch.volume = F(F(vc - 0x10) / F(0x40))
        elif hi == 8:
            ch.volume = self.vslide(ch.volume, vc & 15)
        elif hi == 9:
            ch.volume = self.vslide(ch.volume, vc << 4)
        elif hi == 0xA:
            ch.vib_param = (ch.vib_param & 15) | ((vc & 15) << 4)
        elif hi == 0xC:
            ch.panning = F(F(((vc & 15) << 4) | (vc & 15)) / F(0xFF))
        elif hi == 0xF and vc & 15:
            ch.tp = ((vc & 15) << 4) | (vc & 15)
        if fx == 1 and p:
            ch.pu = p
        elif fx == 2 and p:
            ch.pd = p
        elif fx == 3 and p:
            ch.tp = p
        elif fx == 4:
            if p & 15:
                ch.vib_param = (ch.vib_param & 0xF0) | (p & 15)
            if p >> 4:
                ch.vib_param = (p & 0xF0) | (ch.vib_param & 15)
        elif fx in (5, 6, 0xA) and p:
            ch.vs = p
        elif fx == 7:
            if p & 15:
                ch.trem_param = (ch.trem_param & 0xF0) | (p & 15)
            if p >> 4:
                ch.trem_param = (p & 0xF0) | (ch.trem_param & 15)
        elif fx == 8:
            ch.panning = F(F(p) / F(0xFF))
        elif fx == 9:
            if ch.sample is not None and 0 < note < 97:
                final = p << (7 if ch.sample.bits == 16 else 8)
                ch.pos = F(-1) if final >= ch.sample.length else F(final)
        elif fx == 0xB:
            if p < m.length:
                self.pjump, self.jdest, self.jrow = True, p, 0
        elif fx == 0xC:
            ch.volume = F(F(min(p, 0x40)) / F(0x40))
        elif fx == 0xD:
            self.pbreak = True
            self.jrow = ((p >> 4) * 10 + (p & 15)) & 255
        elif fx == 0xE:
            sub, y = p >> 4, p & 15
            if sub == 1:
                if y:
                    ch.fpu = y
                self.pitch_slide(ch, -ch.fpu)
            elif sub == 2:
                if y:
                    ch.fpd = y
                self.pitch_slide(ch, ch.fpd)
            elif sub == 4:
                ch.vib_wave, ch.vib_retrig = p & 3, not ((p >> 2) & 1)
            elif sub == 5:
                if 0 < ch.cur[0] < 97 and ch.sample is not None:
                    ch.note = self.note_value(ch.cur[0], ch.sample, (y - 8) * 16)
                    ch.period = self.period_of(ch.note)
                    self.update_freq(ch)
            elif sub == 6:
                if y:
                    if y == ch.loop_n:
                        ch.loop_n = 0
                    else:
                        ch.loop_n = (ch.loop_n + 1) & 255
                        self.pjump, self.jrow, self.jdest = True, ch.loop_origin, self.index
                else:
                    ch.loop_origin = self.row
                    self.jrow = ch.loop_origin
            elif sub == 7:
                ch.trem_wave, ch.trem_retrig = p & 3, not ((p >> 2) & 1)
            elif sub == 0xA:
                if y:
                    ch.fvs = y
                ch.volume = self.vslide(ch.volume, ch.fvs << 4)
            elif sub == 0xB:
                if y:
                    ch.fvs = y
                ch.volume = self.vslide(ch.volume, ch.fvs)
            elif sub == 0xD:
                if note == 0 and insn == 0:
                    if ch.cur[4] & 15:
                        ch.note = ch.orig_note
                        self.trigger(ch, keep_vol=True)
                    else:
                        self.trigger(ch, keep_vol=True, keep_period=True, keep_pos=True)
            elif sub == 0xE:
                self.extra = ((ch.cur[4] & 15) * self.tempo) & 0xFFFF
        elif fx == 0xF and p:
            if p <= 0x1F:
                self.tempo = p
            else:
                self.bpm = p
        elif fx == 16:
            self.gvol = F(F(min(p, 0x40)) / F(0x40))
        elif fx == 17 and p:
            ch.gvs = p
        elif fx == 21:
            ch.venv_c = ch.penv_c = p
        elif fx == 25 and p:
            ch.ps = p
        elif fx == 27 and p:
            ch.retrig = ((ch.retrig & 0xF0) | (p & 15)) if (p >> 4) == 0 else p
        elif fx == 29 and p:
            ch.tremor = p
        elif fx == 33:
            if (p >> 4) == 1:
                if p & 15:
                    ch.xpu = p & 15
                self.pitch_slide(ch, F(F(-1) * F(ch.xpu)))
            elif (p >> 4) == 2:
                if p & 15:
                    ch.xpd = p & 15
                self.pitch_slide(ch, ch.xpd)

    def post_change(self):
        if self.index >= self.m.length:
            self.index = self.m.restart & 255

    def do_row(self):
        m = self.m
        if self.pjump:
            self.index, self.row = self.jdest, self.jrow
            self.pjump = self.pbreak = False
            self.jrow = 0
            self.post_change()
        elif self.pbreak:
            self.index = (self.index + 1) & 255
            self.row = self.jrow
            self.pbreak = False
            self.jrow = 0
            self.post_change()
        rows, slots = m.patterns[m.table[self.index]]
        in_loop = False
        for i, ch in enumerate(self.ch):
            s = slots[self.row * m.channels + i] if self.row < rows else [0, 0, 0, 0, 0]
            ch.cur = s
            if s[3] != 0xE or (s[4] >> 4) != 0xD:
                self.handle(ch, s)
            else:
                ch.delay = s[4] & 15
            if ch.loop_n > 0:
                in_loop = True
        if not in_loop:
            k = 256 * self.index + self.row
            self.loop_count = self.visits[k]
            self.visits[k] = (self.visits[k] + 1) & 255
        self.row = (self.row + 1) & 255
        if not self.pjump and not self.pbreak and (self.row >= rows or self.row == 0):
            self.index = (self.index + 1) & 255
            self.row = self.jrow
            self.jrow = 0
            self.post_change()

    @staticmethod
    def env_tick(ch, e, counter, out):
        fr = lambda i: e.frame[i] if i < 12 else 0
        if e.n < 2:
            if e.n == 1:
                out = F(F(e.value[0]) / F(0x40))
                if out > 1:
                    out = F(1)
            return counter, out
        if e.loop_on:
            ls, le = fr(e.ls), fr(e.le)
            if counter >= le:
                counter = (counter - ((le - ls) & 0xFFFF)) & 0xFFFF
        j = 0
        while j < e.n - 2:
            if e.frame[j] <= counter <= e.frame[j + 1]:
                break
            j += 1
        if counter <= e.frame[j]:
            v = F(e.value[j])
        elif counter >= e.frame[j + 1]:
            v = F(e.value[j + 1])
        else:
            p = F(F(counter - e.frame[j]) / F(e.frame[j + 1] - e.frame[j]))
            v = F(F(F(e.value[j]) * F(F(1) - p)) + F(F(e.value[j + 1]) * p))
        out = F(v / F(0x40))
        if not ch.sustained or not e.sustain_on or counter != fr(e.sustain):
            counter = (counter + 1) & 0xFFFF
        return counter, out

    def envelopes(self, ch):
        ins = ch.instrument
        if ins is None or ins.num_samples == 0:
            return
        if ins.venv.on:
            if not ch.sustained:
                ch.fadeout = F(ch.fadeout - F(F(ins.fadeout) / F(32768)))
                if ch.fadeout < 0:
                    ch.fadeout = F(0)
            ch.venv_c, ch.venv_v = self.env_tick(ch, ins.venv, ch.venv_c, ch.venv_v)
        if ins.penv.on:
            ch.penv_c, ch.penv_p = self.env_tick(ch, ins.penv, ch.penv_c, ch.penv_p)

    def do_tick(self):
        if self.tick_n == 0:
            self.do_row()
        t = self.tick_n
        for ch in self.ch:
            self.envelopes(ch)
            self.autovibrato(ch)
            c = ch.cur
            if ch.arp and not c[4]:
                ch.arp, ch.arp_off = False, 0
                self.update_freq(ch)
            if ch.vib and not has_vib(c):
                ch.vib, ch.vib_off = False, F(0)
                self.update_freq(ch)
            vc, fx, p = c[2], c[3], c[4]
            if t != 0:
                hi = vc >> 4
                if hi == 6:
                    ch.volume = self.vslide(ch.volume, vc & 15)
                elif hi == 7:
                    ch.volume = self.vslide(ch.volume, vc << 4)
                elif hi == 0xB:
                    ch.vib = False
                    self.vibrato(ch, ch.vib_param)
                elif hi == 0xD:
                    ch.panning = self.vslide(ch.panning, vc & 15, 0xFF)
                elif hi == 0xE:
                    ch.panning = self.vslide(ch.panning, vc << 4, 0xFF)
                elif hi == 0xF:
                    self.tone_portamento(ch)
            if fx == 0:
                if p > 0:
                    ao = self.tempo % 3
                    if ao == 2 and t == 1:
                        ch.arp, ch.arp_off = True, p >> 4
                        self.update_freq(ch)
                    elif ao >= 1 and t == 0:
                        ch.arp, ch.arp_off = False, 0
                        self.update_freq(ch)
                    else:
                        k = ((t - ao) & 0xFFFF) % 3
                        ch.arp, ch.arp_off = (False, 0) if k == 0 else ((True, p >> 4) if k == 2 else (True, p & 15))
                        self.update_freq(ch)
            elif t != 0 and fx == 1:
                self.pitch_slide(ch, -ch.pu)
            elif t != 0 and fx == 2:
                self.pitch_slide(ch, ch.pd)
            elif t != 0 and fx == 3:
                self.tone_portamento(ch)
            elif t != 0 and fx == 4:
                ch.vib = True
                self.vibrato(ch, ch.vib_param)
            elif t != 0 and fx == 5:
                self.tone_portamento(ch)
                ch.volume = self.vslide(ch.volume, ch.vs)
            elif t != 0 and fx == 6:
                ch.vib = True
                self.vibrato(ch, ch.vib_param)
                ch.volume = self.vslide(ch.volume, ch.vs)
            elif t != 0 and fx == 7:
                step = ch.trem_ticks * (ch.trem_param >> 4)
                ch.trem_ticks = (ch.trem_ticks + 1) & 255
                ch.trem_vol = F(F(F(F(-1) * self.waveform(ch.trem_wave, step & 255)) * F(ch.trem_param & 15)) / F(0xF))
            elif t != 0 and fx == 0xA:
                ch.volume = self.vslide(ch.volume, ch.vs)
            elif fx == 0xE:
                sub = p >> 4
                if sub == 9:
                    if t != 0 and p & 15 and t % (p & 15) == 0:
                        self.trigger(ch, keep_vol=True)
                        self.envelopes(ch)
                elif sub == 0xC:
                    if (p & 15) == t:
                        ch.volume = F(0)
                elif sub == 0xD:
                    if ch.delay == t:
                        self.handle(ch, c)
                        self.envelopes(ch)
            elif fx == 17 and t != 0:
                g = ch.gvs
                if not ((g & 0xF0) and (g & 15)):
                    self.gvol = self.vslide(self.gvol, g)
            elif fx == 20:
                if t == p:
                    self.key_off(ch)
            elif fx == 25 and t != 0:
                ch.panning = self.vslide(ch.panning, ch.ps, 0xFF)
            elif fx == 27 and t != 0:
                if ch.retrig & 15 and t % (ch.retrig & 15) == 0:
                    self.trigger(ch, keep_vol=True, keep_env=True)
                    ins = ch.instrument
                    if not vc and not (ins is not None and ins.num_samples and ins.venv.on):
                        v = F(F(ch.volume * RETRIG_MUL[ch.retrig >> 4]) + F(F(RETRIG_ADD[ch.retrig >> 4]) / F(0x40)))
                        ch.volume = F(0) if v < 0 else (F(1) if v > 1 else v)
            elif fx == 29 and t != 0:
                ch.tremor_on = ((t - 1) % ((ch.tremor >> 4) + (ch.tremor & 15) + 2)) > (ch.tremor >> 4)
            pan = F(ch.panning + F(F(F(ch.penv_p - F(.5)) * F(F(.5) - F(abs(F(ch.panning - F(.5)))))) * F(2)))
            if ch.tremor_on:
                vol = F(0)
            else:
                vol = F(ch.volume + ch.trem_vol)
                vol = F(0) if vol < 0 else (F(1) if vol > 1 else vol)
                vol = F(vol * F(ch.fadeout * ch.venv_v))
            ch.target = [F(vol * sqrtf(F(F(1) - pan))), F(vol * sqrtf(pan))]
        self.tick_n = (self.tick_n + 1) & 0xFFFF
        if self.tick_n >= self.tempo + self.extra:
            self.tick_n = 0
            self.extra = 0
        self.remaining = F(self.remaining + F(F(RATE) / F(F(self.bpm) * F(0.4))))

    # ---- the per-frame layer ----
    @staticmethod
    def advance(ch):
        s = ch.sample
        if s.loop == 0:
            ch.pos = F(ch.pos + ch.step)
            if ch.pos >= F(s.length):
                ch.pos = F(-1)
        elif s.loop == 1:
            ch.pos = F(ch.pos + ch.step)
            while ch.pos >= F(s.loop_end) and ch.pos != np.inf:
                ch.pos = F(ch.pos - F(s.loop_length))
        elif ch.ping:
            ch.pos = F(ch.pos + ch.step)
            if ch.pos >= F(s.loop_end):
                ch.ping = False
                ch.pos = F(F((s.loop_end << 1) & 0xFFFFFFFF) - ch.pos)
            if ch.pos >= F(s.length):
                ch.ping = False
                ch.pos = F(ch.pos - F(s.length - 1))
        else:
            ch.pos = F(ch.pos - ch.step)
            if ch.pos <= F(s.loop_start):
                ch.ping = True
                ch.pos = F(F((s.loop_start << 1) & 0xFFFFFFFF) - ch.pos)
            if ch.pos <= 0:
                ch.ping = True
                ch.pos = F(0)

    def next_of_sample(self, ch):
        if ch.instrument is None or ch.sample is None or ch.pos < 0:
            if ch.fc < 32:
                return lerp(ch.prev[ch.fc], F(0), F(F(ch.fc) / F(32)))
            return F(0)
        s = ch.sample
        if s.length == 0:
            return F(0)
        if not ch.pos >= 0:
            a = 0
        elif ch.pos >= F(s.length):
            a = s.length - 1
        else:
            a = min(int(ch.pos), s.length - 1)
        u = F(F(s.data[a]) / s.scale)
        self.advance(ch)
        if ch.fc < 32:
            return lerp(ch.prev[ch.fc], u, F(F(ch.fc) / F(32)))
        return u

    def generate(self, frames, stop_at_loop=False):
        """xm_generate_samples: float32 [frames, 2] (fewer with stop_at_loop: the frames before the loop count is raised)."""
        out = np.zeros((min(frames, 1 << 16), 2), np.float32)
        ramp = F(1.0 / 128.0)
        piece = None
        for i in range(frames):
            if i == len(out):
                out = np.concatenate([out, np.zeros((min(len(out), frames - len(out)), 2), np.float32)])
            if self.remaining <= 0:
                self.do_tick()
                piece = None
                if stop_at_loop and self.loop_count >= 1:
                    return out[:i]
            self.remaining = F(self.remaining - F(1))
            scale = F(self.gvol * F(0.25))
            if piece is None:
                piece = [0, scale, self.index, self.row, self.loop_count]
                self.ticks.append(piece)
            piece[0] += 1
            if self.loop_count >= 1:
                continue
            left = right = F(0)
            for ch in self.ch:
                if ch.instrument is None or ch.sample is None or ch.pos < 0:
                    continue
                v = self.next_of_sample(ch)
                left = F(left + F(v * ch.actual[0]))
                right = F(right + F(v * ch.actual[1]))
                ch.fc += 1
                ch.actual[0] = slide(ch.actual[0], ch.target[0], ramp)
                ch.actual[1] = slide(ch.actual[1], ch.target[1], ramp)
            out[i, 0] = F(left * scale)
            out[i, 1] = F(right * scale)
        return out[:frames]

    def seek(self, pot, row):
        if pot < 0 or pot >= self.m.length or row < 0 or row > 255:
            return False
        self.index, self.row, self.tick_n, self.remaining = pot, row, 0, F(0)
        return True


def decode_stream(data, reads):
    """The stream's reads (stream.d:595-605): a read returns nothing once the loop count is >= 1, else all its frames."""
    m = load(data)
    if m is None:
        return None, None
    p = Player(m)
    outs = []
    for n in reads:
        if p.loop_count >= 1:
            outs.append(np.zeros((0, 2), np.float32))
        else:
            p.ticks = []
            outs.append(p.generate(n))
    return outs, p


def decode_batch(data, limit=MAX_FRAMES):
    m = load(data)
    if m is None:
        return None
    return Player(m).generate(limit, stop_at_loop=True)
