// afg_mod_front.cpp -- ProTracker MOD: probe, init and the control layer (pocketmod.d:354-662, :724-952) on the host.
//
// The reference mixes as it goes: each tick it changes the channels' pitch, volume and position, then adds every channel
// into the output frame by frame.  Here the control layer runs alone and writes down what the mixer would do: per tick (or
// per piece of a tick, where a read ends inside one) an afg_mod_tick, and per pass of the mixer's segment loop
// (pocketmod.d:684-720) an afg_mod_segment.  The only mixer state the control layer needs back is each channel's position
// at the end of a segment; mod_chain.h computes it without stepping through the frames.
#include "afg_mod_front.h"
#include "../csrc/afg_common.h"
#include "../csrc/mod_chain.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <new>

namespace afg_mod {

namespace {

enum : uint8_t { kPitch = 0x01, kVolume = 0x02 };     // POCKETMOD_PITCH / POCKETMOD_VOLUME

// pocketmod.d:136-153: finetune adjustment per finetune setting and note index
const int8_t kFinetune[16][36] = {
    {   0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0 },
    {  -6, -6, -5, -5, -4, -3, -3, -3, -3, -3, -3, -3, -3, -3, -2, -3, -2, -2, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,  0 },
    { -12,-12,-10,-11, -8, -8, -7, -7, -6, -6, -6, -6, -6, -6, -5, -5, -4, -4, -4, -3, -3, -3, -3, -2, -3, -3, -2, -3, -3, -2, -2, -2, -2, -2, -2, -1 },
    { -18,-17,-16,-16,-13,-12,-12,-11,-10,-10,-10, -9, -9, -9, -8, -8, -7, -6, -6, -5, -5, -5, -5, -4, -5, -4, -3, -4, -4, -3, -3, -3, -3, -2, -2, -2 },
    { -24,-23,-21,-21,-18,-17,-16,-15,-14,-13,-13,-12,-12,-12,-11,-10, -9, -8, -8, -7, -7, -7, -7, -6, -6, -6, -5, -5, -5, -4, -4, -4, -4, -3, -3, -3 },
    { -30,-29,-26,-26,-23,-21,-20,-19,-18,-17,-17,-16,-15,-14,-13,-13,-11,-11,-10, -9, -9, -9, -8, -7, -8, -7, -6, -6, -6, -5, -5, -5, -5, -4, -4, -4 },
    { -36,-34,-32,-31,-27,-26,-24,-23,-22,-21,-20,-19,-18,-17,-16,-15,-14,-13,-12,-11,-11,-10,-10, -9, -9, -9, -7, -8, -7, -6, -6, -6, -6, -5, -5, -4 },
    { -42,-40,-37,-36,-32,-30,-29,-27,-25,-24,-23,-22,-21,-20,-18,-18,-16,-15,-14,-13,-13,-12,-12,-10,-10,-10, -9, -9, -9, -8, -7, -7, -7, -6, -6, -5 },
    {  51, 48, 46, 42, 42, 38, 36, 34, 32, 30, 24, 27, 25, 24, 23, 21, 21, 19, 18, 17, 16, 15, 14, 14, 12, 12, 12, 10, 10, 10,  9,  8,  8,  8,  7,  7 },
    {  44, 42, 40, 37, 37, 35, 32, 31, 29, 27, 25, 24, 22, 21, 20, 19, 18, 17, 16, 15, 15, 14, 13, 12, 11, 10, 10,  9,  9,  9,  8,  7,  7,  7,  6,  6 },
    {  38, 36, 34, 32, 31, 30, 28, 27, 25, 24, 22, 21, 19, 18, 17, 16, 16, 15, 14, 13, 13, 12, 11, 11,  9,  9,  9,  8,  7,  7,  7,  6,  6,  6,  5,  5 },
    {  31, 30, 29, 26, 26, 25, 24, 22, 21, 20, 18, 17, 16, 15, 14, 13, 13, 12, 12, 11, 11, 10,  9,  9,  8,  7,  8,  7,  6,  6,  6,  5,  5,  5,  5,  5 },
    {  25, 24, 23, 21, 21, 20, 19, 18, 17, 16, 14, 14, 13, 12, 11, 10, 11, 10, 10,  9,  9,  8,  7,  7,  6,  6,  6,  5,  5,  5,  5,  4,  4,  4,  3,  4 },
    {  19, 18, 17, 16, 16, 15, 15, 14, 13, 12, 11, 10,  9,  9,  9,  8,  8, 18,  7,  7,  7,  6,  5,  6,  5,  4,  5,  4,  4,  4,  4,  3,  3,  3,  3,  3 },
    {  12, 12, 12, 10, 11, 11, 10, 10,  9,  8,  7,  7,  6,  6,  6,  5,  6,  5,  5,  5,  5,  4,  4,  4,  3,  3,  3,  3,  2,  3,  3,  2,  2,  2,  2,  2 },
    {   6,  6,  6,  5,  6,  6,  6,  5,  5,  5,  4,  4,  3,  3,  3,  3,  3,  3,  3,  3,  3,  2,  2,  2,  2,  1,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1 },
};

// pocketmod.d:183-200: the 36 ProTracker periods at finetune 0, highest first; any other period is note 0
const uint16_t kPeriods[36] = { 856, 808, 762, 720, 678, 640, 604, 570, 538, 508, 480, 453, 428, 404, 381, 360, 339, 320,
                                302, 285, 269, 254, 240, 226, 214, 202, 190, 180, 170, 160, 151, 143, 135, 127, 120, 113 };

int period_to_note(int period)
{
    for (int i = 0; i < 36; i++) if (kPeriods[i] == period) return i;
    return 0;
}

// pocketmod.d:203-213: table sine with 64 steps per period, amplitude 255
int lfo_sine(int step)
{
    static const uint8_t sin16[16] = { 0x00, 0x19, 0x32, 0x4a, 0x62, 0x78, 0x8e, 0xa2, 0xb4, 0xc5, 0xd4, 0xe0, 0xec, 0xf4, 0xfa, 0xfe };
    int x = sin16[step & 0x0f];
    x = (step & 0x1f) < 0x10 ? x : 0xff - x;
    return step < 0x20 ? x : -x;
}

int clamp_volume(int x) { return std::min(std::max(x, 0), 0x40); }

// pocketmod.d:106-120: parameter memory (a zero parameter, or nibble, keeps the old value)
void mem(uint8_t &dst, uint8_t src) { dst = src ? src : dst; }
void mem2(uint8_t &dst, uint8_t src) { dst = (uint8_t)(((src & 0x0f) ? (src & 0x0f) : (dst & 0x0f)) | ((src & 0xf0) ? (src & 0xf0) : (dst & 0xf0))); }

void pitch_slide(uint8_t finetune, uint16_t &period, uint8_t &dirty, int amount)      // pocketmod.d:271-279
{
    const int hi = 856 + kFinetune[finetune][0], lo = 113 + kFinetune[finetune][35];
    period = (uint16_t)(period + amount);
    period = (uint16_t)std::max((int)period, lo);
    period = (uint16_t)std::min((int)period, hi);
    dirty |= kPitch;
}

void volume_slide(uint8_t &volume, uint8_t &dirty, int param)                          // pocketmod.d:281-288
{
    // if both nibbles are set the high one wins (songs rely on it)
    const int change = (param & 0xf0) ? (param >> 4) : -(param & 0x0f);
    volume = (uint8_t)clamp_volume(volume + change);
    dirty |= kVolume;
}

// Where _pocketmod_ident finds the song (pocketmod.d:724-811); channels 0: not a MOD.
struct Layout { int channels = 0, samples = 0; size_t length_at = 0, order_at = 0, patterns_at = 0; };

Layout ident(const uint8_t *d, size_t size)
{
    Layout l;
    if (size >= 1084) {
        // the 40 tags of pocketmod.d:746-755 (FLT8 left out there too); "4CHN" is listed twice in the reference
        static const char *const four[8] = { "M.K.", "M!K!", "FLT4", "4CHN", "OKTA", "OCTA", "CD81", "FA08" };
        static const int four_ch[8] = { 4, 4, 4, 4, 8, 8, 8, 8 };
        const uint8_t *tag = d + 1080;
        int ch = 0;
        for (int i = 0; i < 8 && !ch; i++) if (!std::memcmp(tag, four[i], 4)) ch = four_ch[i];
        if (!ch && tag[0] >= '1' && tag[0] <= '9' && !std::memcmp(tag + 1, "CHN", 3)) ch = tag[0] - '0';
        if (!ch && tag[0] >= '1' && tag[0] <= '3' && tag[1] >= '0' && tag[1] <= '9' && tag[2] == 'C' && tag[3] == 'H') {
            const int n = (tag[0] - '0') * 10 + (tag[1] - '0');
            if (n >= 10 && n <= 32) ch = n;
        }
        if (ch) {
            l.channels = ch; l.samples = 31; l.length_at = 950; l.order_at = 952; l.patterns_at = 1084;
            return l;
        }
    }
    if (size < 600) return l;
    // a 15-instrument module: the title and the 15 sample names are printable ASCII or NUL
    auto printable = [](uint8_t c) { return c == 0 || (c >= ' ' && c <= '~'); };
    for (int i = 0; i < 20; i++) if (!printable(d[i])) return l;
    for (int i = 0; i < 15; i++)
        for (int j = 0; j < 22; j++) if (!printable(d[20 + i * 30 + j])) return l;
    l.channels = 4; l.samples = 15; l.length_at = 470; l.order_at = 472; l.patterns_at = 600;
    return l;
}

// The probes that run before MOD's in the reference and claim files of their own (stream.d:1638-1655 WAV, :1750-1793 XM):
// those files stay refused (WAV and XM are not decoded here).  A RIFF/WAVE file is treated as claimed by the WAV probe,
// a file that passes xm_check_sanity_preload (libxm.d:360-380) by the XM probe.
bool claimed_by_earlier_probe(const uint8_t *d, size_t size)
{
    if (size >= 12 && !std::memcmp(d, "RIFF", 4) && !std::memcmp(d + 8, "WAVE", 4)) return true;
    if (size >= 60 && !std::memcmp(d, "Extended Module: ", 17) && d[37] == 0x1A && d[58] == 0x04 && d[59] == 0x01) return true;
    return false;
}

}  // namespace

bool probe(const uint8_t *data, size_t size, Song *song)
{
    if (!data || size < 600 || size > (size_t)INT_MAX || claimed_by_earlier_probe(data, size)) return false;
    if (!ident(data, std::min<size_t>(size, 1084)).channels) return false;        // stream.d:1803-1809
    Song local;
    return (song ? song : &local)->init(data, size);
}

bool Song::init(const uint8_t *data, size_t size)
{
    // pocketmod_init (pocketmod.d:813-906) with rate 44100
    *this = Song();
    if (!data || size == 0 || size > (size_t)INT_MAX) return false;
    const Layout l = ident(data, size);
    if (!l.channels || l.channels > kMaxChannels) return false;
    data_ = data;
    size_ = size;
    num_channels_ = l.channels;
    num_samples_ = l.samples;
    length_ = data[l.length_at];
    reset_ = data[l.length_at + 1];
    order_at_ = l.order_at;
    patterns_at_ = l.patterns_at;
    if (length_ == 0 || length_ > 128) return false;
    if (reset_ >= length_) reset_ = 0;
    // patterns in the file: the highest order entry below the first one of 128 or more, plus one
    int np = 0;
    for (int i = 0; i < 128 && data[order_at_ + i] < 128; i++) np = std::max(np, (int)data[order_at_ + i]);
    num_patterns_ = np + 1;
    const int64_t pattern_bytes = 256 * (int64_t)num_channels_ * num_patterns_, header_bytes = (int64_t)patterns_at_;
    for (int i = 0; i < length_; i++)
        if (header_bytes + 256 * (int64_t)num_channels_ * data[order_at_ + i] > (int64_t)size) return false;   // over-read
    if (header_bytes + pattern_bytes > (int64_t)size) return false;
    // samples follow the patterns back to back; one that runs past the end of the file is cut (pocketmod.d:878-890)
    const size_t area = (size_t)(header_bytes + pattern_bytes);
    int64_t remaining = (int64_t)size - (int64_t)area;
    uint32_t off = 0;
    for (int i = 0; i < num_samples_; i++) {
        const uint8_t *h = header(i + 1);
        const uint32_t len = (uint32_t)(((h[0] << 8) | h[1]) << 1);
        samples_[i].off = off;
        samples_[i].length = (uint32_t)std::min<int64_t>(len > 2 ? len : 0, remaining);
        off += samples_[i].length;
        remaining -= samples_[i].length;
    }
    // sample numbers above a 15-instrument module's 15 have no data in the reference (a null pointer): here they point at
    // the zero padding
    for (int i = num_samples_; i < 31; i++) samples_[i].off = off;
    plane_.assign(data + area, data + size);
    plane_.resize(plane_.size() + kPlanePad, 0);
    for (int i = 0; i < num_channels_; i++) ch_[i].balance = (uint8_t)(0x80 + ((((i + 1) >> 1) & 1) ? 0x20 : -0x20));   // LRRL
    ticks_per_line_ = 6;
    samples_per_tick_ = kRate / 50.0f;
    lfo_rng_ = 0xbadc0de;
    line_ = -1;
    tick_ = (int16_t)(ticks_per_line_ - 1);
    next_tick();
    return true;
}

uint8_t Song::order(int pattern) const
{
    const int64_t at = (int64_t)order_at_ + pattern;     // pattern_ is an int8 as in the reference: it can go negative
    return at < 0 ? 0 : byte((size_t)at);
}

int Song::lfo(const Chan &ch, int step) const
{
    switch (ch.lfo_type[ch.effect == 7] & 3) {           // the vibrato or the tremolo waveform (E4x / E7x)
    case 0: return lfo_sine(step & 0x3f);
    case 1: return 0xff - ((step & 0x3f) << 3);          // saw
    case 2: return (step & 0x3f) < 0x20 ? 0xff : -0xff;  // square
    default: return (int)(lfo_rng_ & 0x1ff) - 0xff;      // random
    }
}

void Song::update_pitch(Chan &ch)
{
    ch.increment = 0.0f;                                 // period 0: the channel does not advance (and mixes nothing)
    if (ch.period) {
        float period = ch.period;
        if (ch.effect == 0x4 || ch.effect == 0x6) {      // vibrato
            const int step = (ch.param4 >> 4) * ch.lfo_step, rate = ch.param4 & 0x0f;
            period += lfo(ch, step) * rate / 128.0f;
        } else if (ch.effect == 0x0 && ch.param) {       // arpeggio: 2^(X/12) as the reference rounds it
            static const float arpeggio[16] = { 1.000000f, 1.059463f, 1.122462f, 1.189207f, 1.259921f, 1.334840f, 1.414214f, 1.498307f,
                                                1.587401f, 1.681793f, 1.781797f, 1.887749f, 2.000000f, 2.118926f, 2.244924f, 2.378414f };
            const int step = (ch.param >> ((2 - tick_ % 3) << 2)) & 0x0f;
            period /= arpeggio[step];
        }
        ch.increment = 3546894.6f / (period * (float)kRate);
    }
    ch.dirty &= (uint8_t)~kPitch;
}

void Song::update_volume(Chan &ch)
{
    int volume = ch.volume;
    if (ch.effect == 0x7) {                              // tremolo
        const int step = ch.lfo_step * (ch.param7 >> 4);
        volume += lfo(ch, step) * (ch.param7 & 0x0f) >> 6;
    }
    ch.real_volume = (uint8_t)clamp_volume(volume);
    ch.dirty &= (uint8_t)~kVolume;
}

void Song::next_line()
{
    int pattern_break = -1;
    if (line_ == 0) visited_[(uint8_t)pattern_ >> 3] |= (uint8_t)(1 << (pattern_ & 7));    // entering an order index
    if (++line_ == 64) {
        if (++pattern_ == length_) pattern_ = (int8_t)reset_;
        line_ = 0;
    }
    const size_t row = patterns_at_ + (size_t)((order(pattern_) * 64 + line_) * num_channels_ * 4);
    for (int i = 0; i < num_channels_; i++) {
        Chan &ch = ch_[i];
        const uint8_t b0 = byte(row + 4 * i), b1 = byte(row + 4 * i + 1), b2 = byte(row + 4 * i + 2), b3 = byte(row + 4 * i + 3);
        const int sample = (b0 & 0xf0) | (b2 >> 4);
        int period = ((b0 & 0x0f) << 8) | b1;
        const int effect = ((b2 & 0x0f) << 8) | b3;
        const bool extended = (effect >> 8) == 0xe;      // Exy: the effect is 0xE0 + x, the parameter y
        ch.effect = (uint8_t)(extended ? effect >> 4 : effect >> 8);
        ch.param = (uint8_t)(extended ? effect & 0x0f : effect & 0xff);

        if (sample) {                                    // new instrument: finetune and default volume
            if (sample <= 31) {
                const size_t h = 12 + 30 * (size_t)sample;
                ch.sample = (uint8_t)sample;
                ch.finetune = byte(h + 2) & 0x0f;
                ch.volume = (uint8_t)std::min<int>(byte(h + 3), 0x40);
                if (ch.effect != 0xED) ch.dirty |= kVolume;
            } else {
                ch.sample = 0;
            }
        }
        if (period) {                                    // new note: restart the sample (unless 3xx or EDx hold it)
            period += kFinetune[ch.finetune][period_to_note(period)];
            if (ch.effect != 0x3) {
                if (ch.effect != 0xED) {
                    ch.period = (uint16_t)period;
                    ch.dirty |= kPitch;
                    ch.position = 0.0f;
                    ch.lfo_step = 0;
                } else {
                    ch.delayed = (uint16_t)period;
                }
            }
        }
        switch (ch.effect) {                             // effects read once per line (pocketmod.d:423-518)
        case 0x3: mem(ch.param3, ch.param); ch.target = (uint16_t)period ? (uint16_t)period : ch.target; break;
        case 0x5: ch.target = (uint16_t)period ? (uint16_t)period : ch.target; break;
        case 0x4: mem2(ch.param4, ch.param); break;
        case 0x7: mem2(ch.param7, ch.param); break;
        case 0xE1: mem(ch.paramE1, ch.param); break;
        case 0xE2: mem(ch.paramE2, ch.param); break;
        case 0xEA: mem(ch.paramEA, ch.param); break;
        case 0xEB: mem(ch.paramEB, ch.param); break;
        case 0x8: ch.balance = ch.param; break;
        case 0x9:                                        // sample offset
            if (period != 0 || sample != 0) {
                ch.param9 = ch.param ? ch.param : ch.param9;
                ch.position = (float)(ch.param9 << 8);
            }
            break;
        case 0xB: pattern_ = (int8_t)(ch.param < length_ ? ch.param : 0); line_ = -1; break;
        case 0xC: ch.volume = (uint8_t)clamp_volume(ch.param); ch.dirty |= kVolume; break;
        case 0xD: pattern_break = (ch.param >> 4) * 10 + (ch.param & 15); break;
        case 0xE4: ch.lfo_type[0] = ch.param; break;
        case 0xE5: ch.finetune = ch.param; ch.dirty |= kPitch; break;
        case 0xE6:                                       // pattern loop: E60 marks the line, E6x jumps back x times
            if (ch.param) {
                if (!ch.loop_count) { ch.loop_count = ch.param; line_ = (int8_t)ch.loop_line; }
                else if (--ch.loop_count) line_ = (int8_t)ch.loop_line;
            } else {
                ch.loop_line = (uint8_t)(line_ - 1);
            }
            break;
        case 0xE7: ch.lfo_type[1] = ch.param; break;
        case 0xE8: ch.balance = (uint8_t)(ch.param << 4); break;
        case 0xEE: pattern_delay_ = ch.param; break;
        case 0xF:                                        // speed (ticks per line) below 0x20, tempo from there
            if (ch.param) {
                if (ch.param < 0x20) ticks_per_line_ = ch.param;
                else samples_per_tick_ = (float)kRate / (0.4f * ch.param);
            }
            break;
        default: break;
        }
    }
    // one jump per line however many Dxy it holds
    if (pattern_break != -1) {
        line_ = (int8_t)((pattern_break < 64 ? pattern_break : 0) - 1);
        if (++pattern_ == length_) pattern_ = (int8_t)reset_;
    }
}

void Song::next_tick()
{
    tick_ = (int16_t)(tick_ + 1);
    if (tick_ == ticks_per_line_) {
        if (pattern_delay_ > 0) pattern_delay_--;
        else next_line();
        tick_ = 0;
    }
    for (int i = 0; i < num_channels_; i++) {
        Chan &ch = ch_[i];
        const int param = ch.param;
        lfo_rng_ = 0x0019660du * lfo_rng_ + 0x3c6ef35fu;
        switch (ch.effect) {                             // effects of every tick (pocketmod.d:555-589)
        case 0x0: ch.dirty |= kPitch; break;             // arpeggio
        case 0xE9:                                       // retrigger every x ticks
            if (!(param && tick_ % param)) { ch.position = 0.0f; ch.lfo_step = 0; }
            break;
        case 0xEC:                                       // note cut at tick x
            if (tick_ == param) { ch.volume = 0; ch.dirty |= kVolume; }
            break;
        case 0xED:                                       // note delay to tick x
            if (tick_ == param && ch.sample) {
                ch.dirty |= kVolume | kPitch;
                ch.period = ch.delayed;
                ch.position = 0.0f;
                ch.lfo_step = 0;
            }
            break;
        default: break;
        }
        if (tick_ == 0) {                                // fine slides: first tick only
            switch (ch.effect) {
            case 0xE1: pitch_slide(ch.finetune, ch.period, ch.dirty, -(int)ch.paramE1); break;
            case 0xE2: pitch_slide(ch.finetune, ch.period, ch.dirty, (int)ch.paramE2); break;
            case 0xEA: volume_slide(ch.volume, ch.dirty, ch.paramEA << 4); break;
            case 0xEB: volume_slide(ch.volume, ch.dirty, ch.paramEB & 15); break;
            default: break;
            }
        } else {                                         // slides and LFOs: every tick but the first
            switch (ch.effect) {
            case 0x1: pitch_slide(ch.finetune, ch.period, ch.dirty, -param); break;
            case 0x2: pitch_slide(ch.finetune, ch.period, ch.dirty, +param); break;
            case 0x5: volume_slide(ch.volume, ch.dirty, param); /* fall through */
            case 0x3: {                                  // tone portamento towards the target, never past it
                const int rate = ch.param3;
                const int below = ch.period < ch.target;
                const int closer = ch.period + (below ? rate : -rate);
                const int still_below = closer < ch.target;
                ch.period = (uint16_t)(still_below == below ? closer : ch.target);
                ch.dirty |= kPitch;
                break;
            }
            case 0x6: volume_slide(ch.volume, ch.dirty, param); /* fall through */
            case 0x4: ch.lfo_step++; ch.dirty |= kPitch; break;
            case 0x7: ch.lfo_step++; ch.dirty |= kVolume; break;
            case 0xA: volume_slide(ch.volume, ch.dirty, param); break;
            default: break;
            }
        }
        if (ch.dirty & kVolume) update_volume(ch);
        if (ch.dirty & kPitch) update_pitch(ch);
    }
}

void Song::mix_channel(int index, Chan &ch, int frames, uint32_t frame, std::vector<afg_mod_segment> &segs)
{
    // _pocketmod_render_channel (pocketmod.d:664-721): one segment per pass of its loop that writes frames
    const SampleSlot &smp = samples_[ch.sample - 1];
    const size_t h = 12 + 30 * (size_t)ch.sample;
    const int loop_start = ((byte(h + 4) << 8) | byte(h + 5)) << 1;
    const int loop_length = ((byte(h + 6) << 8) | byte(h + 7)) << 1;
    const int loop_end = loop_length > 2 ? loop_start + loop_length : 0xffffff;
    const float sample_end = (float)(1 + std::min(loop_end, (int)smp.length));
    const float volume = ch.real_volume / (float)(128 * 64 * 4);
    const float level_l = volume * (1.0f - ch.balance / 255.0f);
    const float level_r = volume * (0.0f + ch.balance / 255.0f);
    uint32_t left = (uint32_t)frames;                    // samples_to_write (int arithmetic that may wrap in the reference)
    int num;
    do {
        num = cvt_i32((sample_end - ch.position) / ch.increment);
        num = std::min(num, (int)left);
        if (num > 0) {
            afg_mod_segment s;
            s.frame = frame;
            s.frames = (uint32_t)num;
            s.position = ch.position;
            s.increment = ch.increment;
            s.level_l = level_l;
            s.level_r = level_r;
            s.sample_off = smp.off;
            s.loop_start = loop_start;
            s.loop_length = loop_length;
            s.loop_end = loop_end;
            s.length = (int32_t)smp.length;
            s.channel = (uint32_t)index;
            segs.push_back(s);
            ch.position = chain_jump(ch.position, ch.increment, (uint32_t)num);
            frame += (uint32_t)num;
        }
        if (ch.position >= (float)loop_end) {            // wrap at the loop end ...
            ch.position -= (float)loop_length;
        } else if (ch.position >= (float)smp.length) {   // ... or stop at the end of the sample
            ch.position = -1.0f;
            break;
        }
        left -= (uint32_t)num;
    } while (num > 0);
}

int Song::render(int frames, uint32_t frame0, uint32_t seg0, std::vector<afg_mod_tick> &ticks, std::vector<afg_mod_segment> &segs)
{
    // pocketmod_render (pocketmod.d:908-952), frames = buffer_size / 8
    int rendered = 0, remaining = frames;
    while (remaining > 0) {
        int num = cvt_i32(samples_per_tick_ - sample_);  // frames left in this tick
        num = std::min(num + !num, remaining);
        afg_mod_tick t;
        std::memset(&t, 0, sizeof(t));
        t.frame = frame0 + (uint32_t)rendered;
        t.frames = (uint32_t)num;
        t.seg = (uint32_t)(segs.size() - seg0);
        t.pattern = pattern_;
        t.line = line_;
        for (int i = 0; i < num_channels_; i++) {
            Chan &ch = ch_[i];
            if (ch.sample != 0 && ch.position >= 0.0f) mix_channel(i, ch, num, t.frame, segs);
        }
        t.n_seg = (uint32_t)(segs.size() - seg0) - t.seg;
        ticks.push_back(t);
        remaining -= num;
        rendered += num;
        if ((sample_ += (float)num) >= samples_per_tick_) {
            sample_ -= samples_per_tick_;
            next_tick();
            if (line_ == 0 && tick_ == 0) {              // a read stops at every new pattern
                const uint8_t bit = (uint8_t)(1 << (pattern_ & 7));
                uint8_t &v = visited_[(uint8_t)pattern_ >> 3];
                if (v & bit) {                           // an order index played before: the song has looped
                    std::memset(visited_, 0, sizeof(visited_));
                    loop_count_++;
                }
                break;
            }
        }
    }
    return rendered;
}

void Song::seek(int pattern, int row, int tick)
{
    line_ = (int8_t)row;
    pattern_ = (int8_t)pattern;
    tick_ = (int16_t)tick;
    sample_ = 0.0f;
}

uint64_t render_song(Song &song, std::vector<afg_mod_tick> &ticks, std::vector<afg_mod_segment> &segs, bool *capped)
{
    const uint32_t seg0 = (uint32_t)segs.size();
    uint64_t total = 0;
    *capped = false;
    for (;;) {
        if (song.loop_count() >= 1) break;               // stream.d:614
        if (total >= (uint64_t)AFG_MOD_MAX_FRAMES) { *capped = true; break; }
        const int n = song.render((int)((uint64_t)AFG_MOD_MAX_FRAMES - total), (uint32_t)total, seg0, ticks, segs);
        if (n <= 0) break;
        total += (uint64_t)n;
    }
    return total;
}

}  // namespace afg_mod

// ---------------------------------------------------------------------------------------------
// afg_mod_parse: the batch path's control layer for one file, host only
// ---------------------------------------------------------------------------------------------
namespace {
struct ModParsedOwner {
    std::vector<afg_mod_tick> ticks;
    std::vector<afg_mod_segment> segs;
    std::vector<uint8_t> plane;
};
}  // namespace

extern "C" {

int afg_mod_parse(const uint8_t *data, size_t length, afg_mod_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        afg_mod::Song song;
        if (!afg_mod::probe(data, length, &song)) {
            afg::set_error("afg_mod_parse: not a ProTracker MOD");
            return AFG_ERR_UNSUPPORTED;
        }
        std::unique_ptr<ModParsedOwner> own(new (std::nothrow) ModParsedOwner);
        if (!own) return AFG_ERR_OOM;
        bool capped = false;
        out->n_frames = afg_mod::render_song(song, own->ticks, own->segs, &capped);
        own->plane = song.plane();
        out->channels = (uint32_t)song.num_channels();
        out->capped = capped ? 1u : 0u;
        out->n_ticks = own->ticks.size();
        out->n_segments = own->segs.size();
        out->n_sample_bytes = own->plane.size();
        out->ticks = own->ticks.data();
        out->segments = own->segs.data();
        out->sample_bytes = own->plane.data();
        out->owner = own.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("afg_mod_parse: out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_mod_parsed_free(afg_mod_parsed *p)
{
    if (!p) return;
    delete (ModParsedOwner *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

}  // extern "C"
