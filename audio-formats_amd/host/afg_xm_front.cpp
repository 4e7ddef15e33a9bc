// afg_xm_front.cpp -- FastTracker II XM: the loader and the control layer of libxm.d on the host.
//
// The reference mixes as it goes: xm_sample runs xm_tick when a tick's frames are used up, then steps and adds every
// channel frame by frame.  Here the control layer runs alone and writes down what the mixer would do.  The per-frame state
// it needs back -- each channel's position, its two ramping volumes, frame_count -- it advances itself: positions by the
// closed form of mod_chain.h where the chain runs forward, frame by frame where it runs backwards; the volume ramp frame by
// frame for the at most 128 frames it takes (the values go to the side table, so the device's steady segments pay nothing
// and the ramp's roundings are the reference's own adds); the 32 stored cross-fade values by running xm_next_of_sample.
// Every float expression is written in the reference's order and compiled without contraction.
#include "afg_xm_front.h"
#include "../csrc/afg_common.h"
#include "../csrc/mod_chain.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace afg_xm {

namespace {

enum { kNoLoop = 0, kForwardLoop = 1, kPingPongLoop = 2 };
enum : unsigned { kKeepVolume = 1, kKeepPeriod = 2, kKeepSamplePosition = 4, kKeepEnvelope = 8 };
enum { kSine = 0, kRampDown = 1, kSquare = 2, kRandom = 3, kRampUp = 4 };
constexpr uint32_t kInstrumentHeaderLength = 263;
constexpr uint32_t kMaxTickFrames = 4096;
constexpr float kAmplification = 0.25f, kVolumeRamp = 1.0f / 128.0f;

const uint32_t kAmigaFrequencies[13] = { 1712 * 1024, 1616 * 1024, 1525 * 1024, 1440 * 1024, 1357 * 1024, 1281 * 1024, 1209 * 1024,
                                         1141 * 1024, 1077 * 1024, 1017 * 1024, 961 * 1024, 907 * 1024, 856 * 1024 };
const float kMultiRetrigAdd[16] = { 0.0f, -1.0f, -2.0f, -4.0f, -8.0f, -16.0f, 0.0f, 0.0f, 0.0f, 1.0f, 2.0f, 4.0f, 8.0f, 16.0f, 0.0f, 0.0f };
const float kMultiRetrigMultiply[16] = { 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, .6666667f, .5f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.5f, 2.0f };

void slide_towards(float &val, float goal, float incr)      // XM_SLIDE_TOWARDS
{
    if (val > goal) {
        val -= incr;
        if (val < goal) val = goal;
    } else if (val < goal) {
        val += incr;
        if (val > goal) val = goal;
    }
}
float lerp(float u, float v, float t) { return u + t * (v - u); }
float inverse_lerp(float u, float v, float l) { return (l - u) / (v - u); }
bool note_is_valid(int n) { return n > 0 && n < 97; }
// shifts as x86 executes them (the count taken modulo 32): C++ leaves larger counts undefined
int32_t shl(int32_t v, int n) { return (int32_t)((uint32_t)v << (n & 31)); }
int32_t shr(int32_t v, int n) { return v >> (n & 31); }

// Bounded little-endian reads: bytes past the end of the file read 0 (libxm.d:327-354)
struct Reader {
    const uint8_t *d;
    size_t n;
    uint8_t u8b(size_t off, size_t bound) const { return (off < bound && off < n) ? d[off] : 0; }
    uint8_t u8(size_t off) const { return off < n ? d[off] : 0; }
    uint16_t u16(size_t off) const { return (uint16_t)(u8(off) | (u8(off + 1) << 8)); }
    uint32_t u32(size_t off) const { return (uint32_t)u16(off) | ((uint32_t)u16(off + 2) << 16); }
};

}  // namespace

bool probe(const uint8_t *data, size_t size, Song *song)
{
    if (!data || size > (size_t)INT_MAX) return false;
    Song local;
    return (song ? song : &local)->load(data, size);
}

bool Song::load(const uint8_t *data, size_t size)
{
    // xm_check_sanity_preload
    if (size < 60 || std::memcmp(data, "Extended Module: ", 17) != 0 || data[37] != 0x1A || data[59] != 0x01 || data[58] != 0x04)
        return false;
    const Reader r{ data, size };
    // xm_get_memory_needed_for_context, as a budget: what the file declares must stay within 16 MiB + 16 x its length
    // before anything is allocated (a pattern header of 9 bytes may declare 256 x 32 empty cells; a sample's data may be cut)
    const uint64_t budget = ((uint64_t)16 << 20) + 16 * (uint64_t)size;
    size_t offset = 60;
    const uint32_t length = r.u16(offset + 4), restart = r.u16(offset + 6), channels = r.u16(offset + 8);
    const uint32_t n_patterns = r.u16(offset + 10), n_instruments = r.u16(offset + 12);
    // length >= 256 never passes the reference's POT check (its uint8 index cannot reach it); a restart position outside the
    // order and more than 32 channels are this library's bounds
    if (length == 0 || length >= 256 || restart >= length || channels == 0 || channels > (uint32_t)kMaxChannels) return false;
    {
        uint64_t need = (uint64_t)n_patterns * 16 + (uint64_t)n_instruments * 512 + 256 * (uint64_t)length;
        size_t off = offset + r.u32(offset);
        for (uint32_t i = 0; i < n_patterns && need <= budget; i++) {
            const uint32_t rows = r.u16(off + 5);
            if (rows > 256) return false;                    // current_row is a uint8: this library's bound
            need += (uint64_t)rows * channels * 5;
            off += (size_t)r.u32(off) + r.u16(off + 7);
        }
        for (uint32_t i = 0; i < n_instruments && need <= budget; i++) {
            const uint32_t n_samples = r.u16(off + 27);
            uint32_t hs = r.u32(off);
            if (hs == 0 || hs > kInstrumentHeaderLength) hs = kInstrumentHeaderLength;
            off += hs;
            uint32_t aggregate = 0;
            for (uint32_t j = 0; j < n_samples && need <= budget; j++) {
                const uint32_t sz = r.u32(off);
                aggregate += sz;
                need += (uint64_t)sz + 64;
                off += 40;
            }
            off += aggregate;
        }
        if (need > budget) return false;
    }

    // xm_load_module
    length_ = (int)length; restart_ = (int)restart; num_channels_ = (int)channels; num_patterns_ = (int)n_patterns;
    const uint32_t header_size = r.u32(offset);
    const uint16_t flags = (uint16_t)r.u32(offset + 14);
    linear_ = (flags & 1) != 0;
    tempo_ = r.u16(offset + 16);
    bpm_ = r.u16(offset + 18);
    for (int i = 0; i < 256; i++) pattern_table_[i] = r.u8(offset + 20 + (size_t)i);
    offset += header_size;

    patterns_.assign(n_patterns, Pattern());
    for (uint32_t i = 0; i < n_patterns; i++) {
        const uint16_t packed = r.u16(offset + 7);
        Pattern &pat = patterns_[i];
        pat.num_rows = r.u16(offset + 5);
        pat.slots.assign((size_t)pat.num_rows * channels, Slot());
        offset += r.u32(offset);
        Slot spare;
        for (uint32_t j = 0, k = 0; j < packed; ++k) {
            const uint8_t note = r.u8(offset + j);
            Slot &slot = k < pat.slots.size() ? pat.slots[k] : spare;   // cells past the pattern are dropped
            if (note & 0x80) {
                ++j;
                slot.note = (note & 1) ? r.u8(offset + j++) : 0;
                slot.instrument = (note & 2) ? r.u8(offset + j++) : 0;
                slot.volume_column = (note & 4) ? r.u8(offset + j++) : 0;
                slot.effect_type = (note & 8) ? r.u8(offset + j++) : 0;
                slot.effect_param = (note & 16) ? r.u8(offset + j++) : 0;
            } else {
                slot.note = note;
                slot.instrument = r.u8(offset + j + 1);
                slot.volume_column = r.u8(offset + j + 2);
                slot.effect_type = r.u8(offset + j + 3);
                slot.effect_param = r.u8(offset + j + 4);
                j += 5;
            }
        }
        offset += packed;
    }

    instruments_.assign(n_instruments, Instrument());
    data_.clear();
    for (uint32_t i = 0; i < n_instruments; i++) {
        Instrument &in = instruments_[i];
        uint32_t hs = r.u32(offset);
        if (hs == 0 || hs > kInstrumentHeaderLength) hs = kInstrumentHeaderLength;
        const size_t bound = offset + hs;
        // (the reference's 16-bit bounded read checks the file's end only, not the header's: libxm.d:553-556)
        in.num_samples = r.u16(offset + 27);
        if (in.num_samples > 0) {
            for (int j = 0; j < 96; j++) in.sample_of_notes[j] = r.u8b(offset + 33 + (size_t)j, bound);
            Envelope &ve = in.volume_envelope, &pe = in.panning_envelope;
            ve.num_points = std::min<uint8_t>(r.u8b(offset + 225, bound), 12);
            pe.num_points = std::min<uint8_t>(r.u8b(offset + 226, bound), 12);
            for (int j = 0; j < ve.num_points; j++) {
                ve.frame[j] = r.u16(offset + 129 + 4 * (size_t)j);
                ve.value[j] = r.u16(offset + 129 + 4 * (size_t)j + 2);
            }
            for (int j = 0; j < pe.num_points; j++) {
                pe.frame[j] = r.u16(offset + 177 + 4 * (size_t)j);
                pe.value[j] = r.u16(offset + 177 + 4 * (size_t)j + 2);
            }
            ve.sustain_point = r.u8b(offset + 227, bound);
            ve.loop_start_point = r.u8b(offset + 228, bound);
            ve.loop_end_point = r.u8b(offset + 229, bound);
            pe.sustain_point = r.u8b(offset + 230, bound);
            pe.loop_start_point = r.u8b(offset + 231, bound);
            pe.loop_end_point = r.u8b(offset + 232, bound);
            uint8_t f = r.u8b(offset + 233, bound);
            ve.enabled = f & 1; ve.sustain_enabled = f & 2; ve.loop_enabled = f & 4;
            f = r.u8b(offset + 234, bound);
            pe.enabled = f & 1; pe.sustain_enabled = f & 2; pe.loop_enabled = f & 4;
            in.vibrato_type = r.u8b(offset + 235, bound);
            if (in.vibrato_type == 2) in.vibrato_type = 1;
            else if (in.vibrato_type == 1) in.vibrato_type = 2;
            in.vibrato_sweep = r.u8b(offset + 236, bound);
            in.vibrato_depth = r.u8b(offset + 237, bound);
            in.vibrato_rate = r.u8b(offset + 238, bound);
            in.volume_fadeout = r.u16(offset + 239);
            in.samples.assign(in.num_samples, Sample());
        }
        offset += hs;
        for (uint32_t j = 0; j < in.num_samples; j++) {
            Sample &s = in.samples[j];
            s.length = r.u32(offset);
            s.loop_start = r.u32(offset + 4);
            s.loop_length = r.u32(offset + 8);
            s.loop_end = s.loop_start + s.loop_length;
            s.volume = (float)r.u8(offset + 12) / (float)0x40;
            s.finetune = (int8_t)r.u8(offset + 13);
            if (s.loop_start > s.length) s.loop_start = s.length;
            if (s.loop_end > s.length) s.loop_end = s.length;
            s.loop_length = s.loop_end - s.loop_start;
            const uint8_t f2 = r.u8(offset + 14);
            if ((f2 & 3) == 0 || s.loop_length == 0) s.loop_type = kNoLoop;
            else if ((f2 & 3) == 1) s.loop_type = kForwardLoop;
            else s.loop_type = kPingPongLoop;
            s.bits = (f2 & 16) ? 16 : 8;
            s.panning = (float)r.u8(offset + 15) / (float)0xFF;
            s.relative_note = (int8_t)r.u8(offset + 16);
            if (s.bits == 16) { s.loop_start >>= 1; s.loop_length >>= 1; s.loop_end >>= 1; s.length >>= 1; }
            offset += 40;
        }
        for (uint32_t j = 0; j < in.num_samples; j++) {
            Sample &s = in.samples[j];
            data_.resize((data_.size() + 1) & ~(size_t)1);
            s.off = (uint32_t)data_.size();
            if (s.bits == 16) {
                data_.resize(data_.size() + 2 * (size_t)s.length);
                int16_t *dst = (int16_t *)(data_.data() + s.off);
                int16_t v = 0;
                for (uint32_t k = 0; k < s.length; k++) {
                    v = (int16_t)(v + (int16_t)r.u16(offset + ((size_t)k << 1)));
                    dst[k] = v;
                }
                offset += (size_t)s.length << 1;
            } else {
                data_.resize(data_.size() + s.length);
                int8_t *dst = (int8_t *)(data_.data() + s.off);
                int8_t v = 0;
                for (uint32_t k = 0; k < s.length; k++) {
                    v = (int8_t)(v + (int8_t)r.u8(offset + k));
                    dst[k] = v;
                }
                offset += s.length;
            }
        }
    }
    data_.resize(((data_.size() + 15) & ~(size_t)15) + 16);

    // xm_create_context_safe: the playing state
    global_volume_ = 1.0f;
    next_rand_ = 24492;
    table_index_ = 0; row_ = 0; current_tick_ = 0; remaining_ = 0.0f;
    position_jump_ = pattern_break_ = false; jump_dest_ = jump_row_ = 0; extra_ticks_ = 0; loop_count_ = 0;
    ch_.assign((size_t)channels, Chan());
    row_loop_count_.assign((size_t)length * 256, 0);

    // xm_check_sanity_postload
    for (int i = 0; i < length_; ++i) {
        if (pattern_table_[i] >= num_patterns_) {
            if (i + 1 == length_ && length_ > 1) --length_;
            else return false;
        }
    }
    if (restart_ >= length_) return false;
    return true;
}

bool Song::seek(int pot, int row)
{
    if (pot < 0 || pot >= length_ || row < 0 || row > 255) return false;   // the reference checks nothing
    table_index_ = (uint8_t)pot;
    row_ = (uint8_t)row;
    current_tick_ = 0;
    remaining_ = 0;
    return true;
}

float Song::waveform(int type, uint8_t step)
{
    step %= 0x40;
    switch (type) {
    case kSine:
        // D evaluates sin in `real`; here in double, rounded once
        return -(float)std::sin((double)(2.0f * 3.141592f * (float)step / (float)0x40));
    case kRampDown: return (float)(0x20 - step) / 0x20;
    case kSquare: return (step >= 0x20) ? 1.0f : -1.0f;
    case kRandom:
        next_rand_ = next_rand_ * 1103515245u + 12345u;
        return (float)((next_rand_ >> 16) & 0x7FFF) / (float)0x4000 - 1.0f;
    case kRampUp: return (float)(step - 0x20) / 0x20;
    default: break;
    }
    return .0f;
}

void Song::autovibrato(Chan &ch)
{
    if (ch.instrument == nullptr || ch.instrument->vibrato_depth == 0) {
        if (ch.autovibrato_note_offset != 0.0f) {
            ch.autovibrato_note_offset = 0.0f;
            update_frequency(ch);
        }
        return;
    }
    const Instrument &in = *ch.instrument;
    float sweep = 1.0f;
    if (ch.autovibrato_ticks < in.vibrato_sweep)
        sweep = lerp(0.0f, 1.0f, (float)ch.autovibrato_ticks / (float)in.vibrato_sweep);
    const unsigned step = (unsigned)((int)(ch.autovibrato_ticks++) * (int)in.vibrato_rate) >> 2;
    ch.autovibrato_note_offset = .25f * waveform(in.vibrato_type, (uint8_t)step) * (float)in.vibrato_depth / (float)0xF * sweep;
    update_frequency(ch);
}

void Song::vibrato(Chan &ch, uint8_t param)
{
    ch.vibrato_ticks = (uint16_t)(ch.vibrato_ticks + (param >> 4));
    ch.vibrato_note_offset = -2.0f * waveform(ch.vibrato_waveform, (uint8_t)ch.vibrato_ticks) * (float)(param & 0x0F) / (float)0xF;
    update_frequency(ch);
}

void Song::tremolo(Chan &ch, uint8_t param, uint16_t pos)
{
    const unsigned step = (unsigned)pos * (unsigned)(param >> 4);
    ch.tremolo_volume = -1.0f * waveform(ch.tremolo_waveform, (uint8_t)step) * (float)(param & 0x0F) / (float)0xF;
}

void Song::arpeggio(Chan &ch, uint8_t param, uint16_t tick)
{
    switch (tick % 3) {
    case 0: ch.arp_in_progress = false; ch.arp_note_offset = 0; break;
    case 2: ch.arp_in_progress = true; ch.arp_note_offset = param >> 4; break;
    case 1: ch.arp_in_progress = true; ch.arp_note_offset = param & 0x0F; break;
    }
    update_frequency(ch);
}

void Song::tone_portamento(Chan &ch)
{
    if (ch.tone_portamento_target_period == 0.0f) return;
    if (ch.period != ch.tone_portamento_target_period) {
        slide_towards(ch.period, ch.tone_portamento_target_period, (linear_ ? 4.0f : 1.0f) * ch.tone_portamento_param);
        update_frequency(ch);
    }
}

void Song::pitch_slide(Chan &ch, float period_offset)
{
    if (linear_) period_offset *= 4.0f;
    ch.period += period_offset;
    if (ch.period < 0) ch.period = 0;
    update_frequency(ch);
}

static void panning_slide(float &panning, uint8_t rawval)
{
    if ((rawval & 0xF0) && (rawval & 0x0F)) return;
    if (rawval & 0xF0) {
        const float f = (float)(rawval >> 4) / (float)0xFF;
        panning += f;
        if (panning > 1) panning = 1;
    } else {
        const float f = (float)(rawval & 0x0F) / (float)0xFF;
        panning -= f;
        if (panning < 0) panning = 0;
    }
}

static void volume_slide(float &volume, uint8_t rawval)
{
    if ((rawval & 0xF0) && (rawval & 0x0F)) return;
    if (rawval & 0xF0) {
        const float f = (float)(rawval >> 4) / (float)0x40;
        volume += f;
        if (volume > 1) volume = 1;
    } else {
        const float f = (float)(rawval & 0x0F) / (float)0x40;
        volume -= f;
        if (volume < 0) volume = 0;
    }
}

static float amiga_period(float note)
{
    // cast(uint) of a float as x86-64 does it: through a 64-bit truncation
    const uint32_t intnote = (note > -9.0e18f && note < 9.0e18f) ? (uint32_t)(int64_t)note : 0u;
    const uint8_t a = (uint8_t)(intnote % 12);
    const int8_t octave = (int8_t)afg_mod::cvt_i32(note / 12.0f - 2);
    int32_t p1 = (int32_t)kAmigaFrequencies[a], p2 = (int32_t)kAmigaFrequencies[a + 1];
    if (octave > 0) { p1 = shr(p1, octave); p2 = shr(p2, octave); }
    else if (octave < 0) { p1 = shl(p1, -(int)octave); p2 = shl(p2, -(int)octave); }
    return lerp((float)p1, (float)p2, note - (float)intnote) / 1024;
}

static float amiga_frequency(float period)
{
    if (period == .0f) return .0f;
    return 7093789.2f / (period * 2.0f);
}

float Song::period_of(float note) const
{
    return linear_ ? 7680.0f - note * 64.0f : amiga_period(note);
}

float Song::frequency_of(float period, float note_offset, float period_offset) const
{
    if (linear_) {
        // D evaluates pow in `real`; here exp2 in double, rounded once
        const float x = (4608.0f - (period - 64.0f * note_offset - 16.0f * period_offset)) / 768.0f;
        return 8363.0f * (float)std::exp2((double)x);
    }
    if (note_offset == 0) return amiga_frequency(period + 16.0f * period_offset);
    uint8_t a = 0;
    int8_t octave = 0;
    int32_t p1 = 0, p2 = 0;
    period *= 1024;
    // (both searches end within 31 steps here; the reference's do not end for a period the shifted table never reaches)
    if (period > (float)kAmigaFrequencies[0]) {
        --octave;
        while (octave > -31 && period > (float)(kAmigaFrequencies[0] << ((-(int)octave) & 31))) --octave;
    } else if (period < (float)kAmigaFrequencies[12]) {
        ++octave;
        while (octave < 31 && period < (float)(kAmigaFrequencies[12] >> (octave & 31))) ++octave;
    }
    for (uint8_t i = 0; i < 12; ++i) {
        p1 = (int32_t)kAmigaFrequencies[i]; p2 = (int32_t)kAmigaFrequencies[i + 1];
        if (octave > 0) { p1 = shr(p1, octave); p2 = shr(p2, octave); }
        else if (octave < 0) { p1 = shl(p1, -(int)octave); p2 = shl(p2, -(int)octave); }
        if ((float)p2 <= period && period <= (float)p1) { a = i; break; }
    }
    const float note = 12.0f * (float)(octave + 2) + (float)a + inverse_lerp((float)p1, (float)p2, period);
    return amiga_frequency(amiga_period(note + note_offset) + 16.0f * period_offset);
}

void Song::update_frequency(Chan &ch)
{
    ch.frequency = frequency_of(ch.period, (float)ch.arp_note_offset, ch.vibrato_note_offset + ch.autovibrato_note_offset);
    ch.step = ch.frequency / (float)kRate;
}

void Song::trigger_note(Chan &ch, unsigned flags)
{
    if (!(flags & kKeepSamplePosition)) {
        ch.sample_position = 0.0f;
        ch.ping = true;
    }
    if (ch.sample != nullptr) {
        if (!(flags & kKeepVolume)) ch.volume = ch.sample->volume;
        ch.panning = ch.sample->panning;
    }
    if (!(flags & kKeepEnvelope)) {
        ch.sustained = true;
        ch.fadeout_volume = ch.volume_envelope_volume = 1.0f;
        ch.panning_envelope_panning = .5f;
        ch.volume_envelope_frame_count = ch.panning_envelope_frame_count = 0;
    }
    ch.vibrato_note_offset = 0.0f;
    ch.tremolo_volume = 0.0f;
    ch.tremor_on = false;
    ch.autovibrato_ticks = 0;
    if (ch.vibrato_waveform_retrigger) ch.vibrato_ticks = 0;
    if (ch.tremolo_waveform_retrigger) ch.tremolo_ticks = 0;
    if (!(flags & kKeepPeriod)) {
        ch.period = period_of(ch.note);
        update_frequency(ch);
    }
}

static void key_off(bool &sustained, float &volume, bool envelope_enabled)
{
    sustained = false;
    if (!envelope_enabled) volume = .0f;
}

void Song::handle_note_and_instrument(Chan &ch, const Slot &s)
{
    if (s.instrument > 0) {
        if (ch.current.has_tone_portamento() && ch.instrument != nullptr && ch.sample != nullptr) {
            trigger_note(ch, kKeepPeriod | kKeepSamplePosition);
        } else if (s.note == 0 && ch.sample != nullptr) {
            trigger_note(ch, kKeepSamplePosition);
        } else if (s.instrument > instruments_.size()) {
            ch.volume = .0f;
            ch.instrument = nullptr;
            ch.sample = nullptr;
        } else {
            ch.instrument = &instruments_[(size_t)s.instrument - 1];
        }
    }

    if (note_is_valid(s.note)) {
        const Instrument *in = ch.instrument;
        if (ch.current.has_tone_portamento() && in != nullptr && ch.sample != nullptr) {
            ch.note = (float)(s.note + ch.sample->relative_note) + ch.sample->finetune / 128.0f - 1.0f;
            ch.tone_portamento_target_period = period_of(ch.note);
        } else if (in == nullptr || in->num_samples == 0) {
            ch.volume = .0f;
        } else if (in->sample_of_notes[s.note - 1] < in->num_samples) {
            for (int z = 0; z < kRampPoints; ++z) ch.end_of_previous_sample[z] = next_of_sample(ch);
            ch.frame_count = 0;
            ch.sample = &in->samples[in->sample_of_notes[s.note - 1]];
            ch.orig_note = ch.note = (float)(s.note + ch.sample->relative_note) + ch.sample->finetune / 128.0f - 1.0f;
            trigger_note(ch, s.instrument > 0 ? 0 : kKeepVolume);
        } else {
            ch.volume = .0f;
        }
    } else if (s.note == 97) {
        key_off(ch.sustained, ch.volume, ch.instrument != nullptr && ch.instrument->volume_envelope.enabled);
    }

    switch (s.volume_column >> 4) {
    case 0x5:
        if (s.volume_column > 0x50) break;
        /* fall through */
    case 0x1: case 0x2: case 0x3: case 0x4:
        ch.volume = (float)(s.volume_column - 0x10) / (float)0x40;
        break;
    case 0x8: volume_slide(ch.volume, s.volume_column & 0x0F); break;
    case 0x9: volume_slide(ch.volume, (uint8_t)(s.volume_column << 4)); break;
    case 0xA: ch.vibrato_param = (uint8_t)((ch.vibrato_param & 0x0F) | ((s.volume_column & 0x0F) << 4)); break;
    case 0xC: ch.panning = (float)(((s.volume_column & 0x0F) << 4) | (s.volume_column & 0x0F)) / (float)0xFF; break;
    case 0xF:
        if (s.volume_column & 0x0F) ch.tone_portamento_param = (uint8_t)(((s.volume_column & 0x0F) << 4) | (s.volume_column & 0x0F));
        break;
    default: break;
    }

    const uint8_t p = s.effect_param;
    switch (s.effect_type) {
    case 1: if (p > 0) ch.portamento_up_param = p; break;
    case 2: if (p > 0) ch.portamento_down_param = p; break;
    case 3: if (p > 0) ch.tone_portamento_param = p; break;
    case 4:
        if (p & 0x0F) ch.vibrato_param = (ch.vibrato_param & 0xF0) | (p & 0x0F);
        if (p >> 4) ch.vibrato_param = (p & 0xF0) | (ch.vibrato_param & 0x0F);
        break;
    case 5: case 6: case 0xA: if (p > 0) ch.volume_slide_param = p; break;
    case 7:
        if (p & 0x0F) ch.tremolo_param = (ch.tremolo_param & 0xF0) | (p & 0x0F);
        if (p >> 4) ch.tremolo_param = (p & 0xF0) | (ch.tremolo_param & 0x0F);
        break;
    case 8: ch.panning = (float)p / (float)0xFF; break;
    case 9:
        if (ch.sample != nullptr && note_is_valid(s.note)) {
            const uint32_t final_offset = (uint32_t)p << (ch.sample->bits == 16 ? 7 : 8);
            if (final_offset >= ch.sample->length) { ch.sample_position = -1; break; }
            ch.sample_position = (float)final_offset;
        }
        break;
    case 0xB:
        if (p < length_) { position_jump_ = true; jump_dest_ = p; jump_row_ = 0; }
        break;
    case 0xC: ch.volume = (float)((p > 0x40) ? 0x40 : p) / (float)0x40; break;
    case 0xD:
        pattern_break_ = true;
        jump_row_ = (uint8_t)((p >> 4) * 10 + (p & 0x0F));
        break;
    case 0xE:
        switch (p >> 4) {
        case 1:
            if (p & 0x0F) ch.fine_portamento_up_param = p & 0x0F;
            pitch_slide(ch, (float)-(int)ch.fine_portamento_up_param);
            break;
        case 2:
            if (p & 0x0F) ch.fine_portamento_down_param = p & 0x0F;
            pitch_slide(ch, ch.fine_portamento_down_param);
            break;
        case 4: ch.vibrato_waveform = p & 3; ch.vibrato_waveform_retrigger = !((p >> 2) & 1); break;
        case 5:
            if (note_is_valid(ch.current.note) && ch.sample != nullptr) {
                ch.note = (float)(ch.current.note + ch.sample->relative_note) + (float)(((p & 0x0F) - 8) * 16) / 128.0f - 1.0f;
                ch.period = period_of(ch.note);
                update_frequency(ch);
            }
            break;
        case 6:
            if (p & 0x0F) {
                if ((p & 0x0F) == ch.pattern_loop_count) { ch.pattern_loop_count = 0; break; }
                ch.pattern_loop_count++;
                position_jump_ = true;
                jump_row_ = ch.pattern_loop_origin;
                jump_dest_ = table_index_;
            } else {
                ch.pattern_loop_origin = row_;
                jump_row_ = ch.pattern_loop_origin;
            }
            break;
        case 7: ch.tremolo_waveform = p & 3; ch.tremolo_waveform_retrigger = !((p >> 2) & 1); break;
        case 0xA:
            if (p & 0x0F) ch.fine_volume_slide_param = p & 0x0F;
            volume_slide(ch.volume, (uint8_t)(ch.fine_volume_slide_param << 4));
            break;
        case 0xB:
            if (p & 0x0F) ch.fine_volume_slide_param = p & 0x0F;
            volume_slide(ch.volume, ch.fine_volume_slide_param);
            break;
        case 0xD:
            if (s.note == 0 && s.instrument == 0) {
                if (ch.current.effect_param & 0x0F) {
                    ch.note = ch.orig_note;
                    trigger_note(ch, kKeepVolume);
                } else {
                    trigger_note(ch, kKeepVolume | kKeepPeriod | kKeepSamplePosition);
                }
            }
            break;
        case 0xE: extra_ticks_ = (uint16_t)((ch.current.effect_param & 0x0F) * tempo_); break;
        default: break;
        }
        break;
    case 0xF:
        if (p > 0) {
            if (p <= 0x1F) tempo_ = p;
            else bpm_ = p;
        }
        break;
    case 16: global_volume_ = (float)((p > 0x40) ? 0x40 : p) / (float)0x40; break;
    case 17: if (p > 0) ch.global_volume_slide_param = p; break;
    case 21: ch.volume_envelope_frame_count = p; ch.panning_envelope_frame_count = p; break;
    case 25: if (p > 0) ch.panning_slide_param = p; break;
    case 27:
        if (p > 0) {
            if ((p >> 4) == 0) ch.multi_retrig_param = (ch.multi_retrig_param & 0xF0) | (p & 0x0F);
            else ch.multi_retrig_param = p;
        }
        break;
    case 29: if (p > 0) ch.tremor_param = p; break;
    case 33:
        switch (p >> 4) {
        case 1:
            if (p & 0x0F) ch.extra_fine_portamento_up_param = p & 0x0F;
            pitch_slide(ch, -1.0f * ch.extra_fine_portamento_up_param);
            break;
        case 2:
            if (p & 0x0F) ch.extra_fine_portamento_down_param = p & 0x0F;
            pitch_slide(ch, ch.extra_fine_portamento_down_param);
            break;
        default: break;
        }
        break;
    default: break;
    }
}

void Song::post_pattern_change()
{
    if (table_index_ >= length_) table_index_ = (uint8_t)restart_;
}

void Song::row_step()
{
    if (position_jump_) {
        table_index_ = jump_dest_;
        row_ = jump_row_;
        position_jump_ = false;
        pattern_break_ = false;
        jump_row_ = 0;
        post_pattern_change();
    } else if (pattern_break_) {
        table_index_++;
        row_ = jump_row_;
        pattern_break_ = false;
        jump_row_ = 0;
        post_pattern_change();
    }
    // (an order index set by a seek stays inside the order: Song::seek)
    const Pattern &cur = patterns_[pattern_table_[table_index_]];
    bool in_a_loop = false;
    for (int i = 0; i < num_channels_; ++i) {
        // a row past the pattern's end (a break or a seek into a shorter pattern) reads empty cells
        const Slot s = row_ < cur.num_rows ? cur.slots[(size_t)row_ * (size_t)num_channels_ + (size_t)i] : Slot();
        Chan &ch = ch_[(size_t)i];
        ch.current = s;
        if (s.effect_type != 0xE || (s.effect_param >> 4) != 0xD) handle_note_and_instrument(ch, s);
        else ch.note_delay_param = s.effect_param & 0x0F;
        if (!in_a_loop && ch.pattern_loop_count > 0) in_a_loop = true;
    }
    if (!in_a_loop) loop_count_ = row_loop_count_[256 * (size_t)table_index_ + row_]++;
    row_++;
    if (!position_jump_ && !pattern_break_ && (row_ >= cur.num_rows || row_ == 0)) {
        table_index_++;
        row_ = jump_row_;
        jump_row_ = 0;
        post_pattern_change();
    }
}

static void envelope_tick(bool sustained, const uint16_t *frame, const uint16_t *value, uint8_t num_points, uint8_t sustain_point,
                          uint8_t loop_start_point, uint8_t loop_end_point, bool sustain_enabled, bool loop_enabled,
                          uint16_t &counter, float &outval)
{
    // a point index of 12 or more (the file's byte is not checked) reads frame 0
    auto frame_at = [&](uint8_t i) -> uint16_t { return i < 12 ? frame[i] : (uint16_t)0; };
    if (num_points < 2) {
        if (num_points == 1) {
            outval = (float)value[0] / (float)0x40;
            if (outval > 1) outval = 1;
        }
        return;
    }
    if (loop_enabled) {
        const uint16_t loop_start = frame_at(loop_start_point), loop_end = frame_at(loop_end_point);
        const uint16_t loop_length = (uint16_t)(loop_end - loop_start);
        if (counter >= loop_end) counter = (uint16_t)(counter - loop_length);
    }
    uint8_t j;
    for (j = 0; j < (num_points - 2); ++j)
        if (frame[j] <= counter && frame[j + 1] >= counter) break;
    float v;
    if (counter <= frame[j]) v = value[j];
    else if (counter >= frame[j + 1]) v = value[j + 1];
    else {
        const float p = (float)(counter - frame[j]) / (float)(frame[j + 1] - frame[j]);
        v = value[j] * (1 - p) + value[j + 1] * p;
    }
    outval = v / (float)0x40;
    if (!sustained || !sustain_enabled || counter != frame_at(sustain_point)) counter++;
}

void Song::envelopes(Chan &ch)
{
    if (ch.instrument == nullptr) return;
    const Envelope &ve = ch.instrument->volume_envelope, &pe = ch.instrument->panning_envelope;
    if (ve.enabled) {
        if (!ch.sustained) {
            ch.fadeout_volume -= ch.instrument->volume_fadeout / 32768.0f;
            if (ch.fadeout_volume < 0) ch.fadeout_volume = 0;
        }
        envelope_tick(ch.sustained, ve.frame, ve.value, ve.num_points, ve.sustain_point, ve.loop_start_point, ve.loop_end_point,
                      ve.sustain_enabled, ve.loop_enabled, ch.volume_envelope_frame_count, ch.volume_envelope_volume);
    }
    if (pe.enabled)
        envelope_tick(ch.sustained, pe.frame, pe.value, pe.num_points, pe.sustain_point, pe.loop_start_point, pe.loop_end_point,
                      pe.sustain_enabled, pe.loop_enabled, ch.panning_envelope_frame_count, ch.panning_envelope_panning);
}

void Song::tick()
{
    if (current_tick_ == 0) row_step();

    for (int i = 0; i < num_channels_; ++i) {
        Chan &ch = ch_[(size_t)i];
        envelopes(ch);
        autovibrato(ch);
        if (ch.arp_in_progress && !ch.current.has_arpeggio()) {
            ch.arp_in_progress = false;
            ch.arp_note_offset = 0;
            update_frequency(ch);
        }
        if (ch.vibrato_in_progress && !ch.current.has_vibrato()) {
            ch.vibrato_in_progress = false;
            ch.vibrato_note_offset = 0.0f;
            update_frequency(ch);
        }
        const uint8_t vc = ch.current.volume_column;
        if (current_tick_ != 0) {
            switch (vc >> 4) {
            case 0x6: volume_slide(ch.volume, vc & 0x0F); break;
            case 0x7: volume_slide(ch.volume, (uint8_t)(vc << 4)); break;
            case 0xB: ch.vibrato_in_progress = false; vibrato(ch, ch.vibrato_param); break;
            case 0xD: panning_slide(ch.panning, vc & 0x0F); break;
            case 0xE: panning_slide(ch.panning, (uint8_t)(vc << 4)); break;
            case 0xF: tone_portamento(ch); break;
            default: break;
            }
        }
        const uint8_t p = ch.current.effect_param;
        switch (ch.current.effect_type) {
        case 0:
            if (p > 0) {
                const int arp_offset = tempo_ % 3;
                if (arp_offset == 2 && current_tick_ == 1) {
                    ch.arp_in_progress = true;
                    ch.arp_note_offset = p >> 4;
                    update_frequency(ch);
                } else if (arp_offset >= 1 && current_tick_ == 0) {
                    ch.arp_in_progress = false;
                    ch.arp_note_offset = 0;
                    update_frequency(ch);
                } else {
                    arpeggio(ch, p, (uint16_t)(current_tick_ - arp_offset));
                }
            }
            break;
        case 1: if (current_tick_ != 0) pitch_slide(ch, (float)-(int)ch.portamento_up_param); break;
        case 2: if (current_tick_ != 0) pitch_slide(ch, ch.portamento_down_param); break;
        case 3: if (current_tick_ != 0) tone_portamento(ch); break;
        case 4:
            if (current_tick_ == 0) break;
            ch.vibrato_in_progress = true;
            vibrato(ch, ch.vibrato_param);
            break;
        case 5:
            if (current_tick_ == 0) break;
            tone_portamento(ch);
            volume_slide(ch.volume, ch.volume_slide_param);
            break;
        case 6:
            if (current_tick_ == 0) break;
            ch.vibrato_in_progress = true;
            vibrato(ch, ch.vibrato_param);
            volume_slide(ch.volume, ch.volume_slide_param);
            break;
        case 7: if (current_tick_ != 0) tremolo(ch, ch.tremolo_param, ch.tremolo_ticks++); break;
        case 0xA: if (current_tick_ != 0) volume_slide(ch.volume, ch.volume_slide_param); break;
        case 0xE:
            switch (p >> 4) {
            case 0x9:
                if (current_tick_ != 0 && (p & 0x0F)) {
                    if (!(current_tick_ % (p & 0x0F))) {
                        trigger_note(ch, kKeepVolume);
                        envelopes(ch);
                    }
                }
                break;
            case 0xC: if ((p & 0x0F) == current_tick_) ch.volume = .0f; break;
            case 0xD:
                if (ch.note_delay_param == current_tick_) {
                    handle_note_and_instrument(ch, ch.current);
                    envelopes(ch);
                }
                break;
            default: break;
            }
            break;
        case 17:
            if (current_tick_ == 0) break;
            if ((ch.global_volume_slide_param & 0xF0) && (ch.global_volume_slide_param & 0x0F)) break;
            if (ch.global_volume_slide_param & 0xF0) {
                const float f = (float)(ch.global_volume_slide_param >> 4) / (float)0x40;
                global_volume_ += f;
                if (global_volume_ > 1) global_volume_ = 1;
            } else {
                const float f = (float)(ch.global_volume_slide_param & 0x0F) / (float)0x40;
                global_volume_ -= f;
                if (global_volume_ < 0) global_volume_ = 0;
            }
            break;
        case 20:
            if (current_tick_ == p) key_off(ch.sustained, ch.volume, ch.instrument != nullptr && ch.instrument->volume_envelope.enabled);
            break;
        case 25: if (current_tick_ != 0) panning_slide(ch.panning, ch.panning_slide_param); break;
        case 27:
            if (current_tick_ == 0) break;
            if ((ch.multi_retrig_param & 0x0F) == 0) break;
            if ((current_tick_ % (ch.multi_retrig_param & 0x0F)) == 0) {
                trigger_note(ch, kKeepVolume | kKeepEnvelope);
                // (the reference reads the instrument without checking it; no instrument counts as no envelope here)
                if (!ch.current.volume_column && !(ch.instrument != nullptr && ch.instrument->volume_envelope.enabled)) {
                    float v = ch.volume * kMultiRetrigMultiply[ch.multi_retrig_param >> 4] + kMultiRetrigAdd[ch.multi_retrig_param >> 4] / (float)0x40;
                    if (v < 0) v = 0;
                    if (v > 1) v = 1;
                    ch.volume = v;
                }
            }
            break;
        case 29:
            if (current_tick_ == 0) break;
            ch.tremor_on = ((current_tick_ - 1) % ((ch.tremor_param >> 4) + (ch.tremor_param & 0x0F) + 2)) > (ch.tremor_param >> 4);
            break;
        default: break;
        }

        const float panning = ch.panning + (ch.panning_envelope_panning - .5f) * (.5f - std::fabs(ch.panning - .5f)) * 2.0f;
        float volume;
        if (ch.tremor_on) {
            volume = .0f;
        } else {
            volume = ch.volume + ch.tremolo_volume;
            if (volume < 0) volume = 0;
            if (volume > 1) volume = 1;
            volume *= ch.fadeout_volume * ch.volume_envelope_volume;
        }
        ch.target_volume[0] = volume * sqrtf(1.0f - panning);
        ch.target_volume[1] = volume * sqrtf(panning);
    }

    current_tick_++;
    if (current_tick_ >= tempo_ + extra_ticks_) {
        current_tick_ = 0;
        extra_ticks_ = 0;
    }
    remaining_ += (float)kRate / ((float)bpm_ * 0.4f);
}

namespace {

// the index xm_sample_at reads for a position of a playing channel; a position at or past the sample's end (only a ping-pong
// turn with a step of more than the loop can leave one) reads the last sample, and a NaN reads the first
uint32_t index_of(float position, uint32_t length)
{
    if (!(position >= 0.0f)) return 0;
    if (position >= (float)length) return length - 1;
    return std::min((uint32_t)position, length - 1);
}

}  // namespace

// The position part of xm_next_of_sample (libxm.d:2344-2413) for one frame.  True when the frame took one of its branches
// (wrap, turn, end): a segment ends behind such a frame.
template <class S, class C>
static bool advance(const S &sm, C &ch)
{
    bool event = false;
    switch (sm.loop_type) {
    case kNoLoop:
        ch.sample_position += ch.step;
        if (ch.sample_position >= (float)sm.length) { ch.sample_position = -1; event = true; }
        break;
    case kForwardLoop:
        ch.sample_position += ch.step;
        while (ch.sample_position >= (float)sm.loop_end && ch.sample_position != INFINITY) {
            ch.sample_position -= (float)sm.loop_length;
            event = true;
        }
        break;
    default:
        if (ch.ping) {
            ch.sample_position += ch.step;
            if (ch.sample_position >= (float)sm.loop_end) {
                ch.ping = false;
                ch.sample_position = (float)(sm.loop_end << 1) - ch.sample_position;
                event = true;
            }
            if (ch.sample_position >= (float)sm.length) {
                ch.ping = false;
                ch.sample_position -= (float)(sm.length - 1);
                event = true;
            }
        } else {
            ch.sample_position -= ch.step;
            if (ch.sample_position <= (float)sm.loop_start) {
                ch.ping = true;
                ch.sample_position = (float)(sm.loop_start << 1) - ch.sample_position;
                event = true;
            }
            if (ch.sample_position <= .0f) {
                ch.ping = true;
                ch.sample_position = .0f;
                event = true;
            }
        }
        break;
    }
    return event;
}

float Song::next_of_sample(Chan &ch)
{
    if (ch.instrument == nullptr || ch.sample == nullptr || ch.sample_position < 0) {
        if (ch.frame_count < (uint64_t)kRampPoints)
            return lerp(ch.end_of_previous_sample[ch.frame_count], .0f, (float)ch.frame_count / (float)kRampPoints);
        return .0f;
    }
    const Sample &sm = *ch.sample;
    if (sm.length == 0) return .0f;
    const uint32_t a = index_of(ch.sample_position, sm.length);
    const float u = sm.bits == 8 ? ((const int8_t *)(data_.data() + sm.off))[a] / 128.0f
                                 : ((const int16_t *)(data_.data() + sm.off))[a] / 32768.0f;
    advance(sm, ch);
    if (ch.frame_count < (uint64_t)kRampPoints)
        return lerp(ch.end_of_previous_sample[ch.frame_count], u, (float)ch.frame_count / (float)kRampPoints);
    return u;
}

void Song::mix_channel(int index, Chan &ch, uint32_t frames, uint32_t frame, Records &rec)
{
    const Sample &sm = *ch.sample;
    auto steady = [&]() {
        return !(ch.actual_volume[0] > ch.target_volume[0]) && !(ch.actual_volume[0] < ch.target_volume[0]) &&
               !(ch.actual_volume[1] > ch.target_volume[1]) && !(ch.actual_volume[1] < ch.target_volume[1]);
    };
    uint32_t left = frames;
    if (sm.length == 0) {
        // xm_next_of_sample returns 0 and steps nothing: the frames add +0 * volume; the ramp and frame_count go on
        for (uint32_t k = 0; k < left && !steady(); k++) {
            slide_towards(ch.actual_volume[0], ch.target_volume[0], kVolumeRamp);
            slide_towards(ch.actual_volume[1], ch.target_volume[1], kVolumeRamp);
        }
        ch.frame_count += left;
        return;
    }
    while (left > 0 && !(ch.sample_position < 0)) {
        const bool fade = ch.frame_count < (uint64_t)kRampPoints;
        const bool ramp = !steady();
        uint32_t cap = left;
        if (fade) cap = std::min<uint32_t>(cap, (uint32_t)(kRampPoints - ch.frame_count));
        if (ramp) {
            // slides until both volumes rest: frames 0 .. k-1 are mixed with moving volumes
            float a0 = ch.actual_volume[0], a1 = ch.actual_volume[1];
            uint32_t k = 0;
            while (k < cap) {
                slide_towards(a0, ch.target_volume[0], kVolumeRamp);
                slide_towards(a1, ch.target_volume[1], kVolumeRamp);
                k++;
                if (!(a0 > ch.target_volume[0]) && !(a0 < ch.target_volume[0]) && !(a1 > ch.target_volume[1]) && !(a1 < ch.target_volume[1])) break;
            }
            cap = k;
        }
        afg_xm_segment g;
        std::memset(&g, 0, sizeof(g));
        g.frame = frame;
        g.sample_off = sm.off;
        g.last = sm.length - 1;
        g.flags = sm.bits == 16 ? AFG_XM_SEG_16BIT : 0u;
        g.channel = (uint32_t)index;
        g.position = ch.sample_position;
        g.step = ch.step;
        g.vol_l = ch.actual_volume[0];
        g.vol_r = ch.actual_volume[1];
        g.fade_count = (uint32_t)std::min<uint64_t>(ch.frame_count, 0xffffffffu);
        const bool forward = sm.loop_type != kPingPongLoop || ch.ping;
        const bool regular = forward && ch.step >= 0.0f && ch.step < INFINITY && ch.sample_position < INFINITY;
        uint32_t m;
        if (regular) {
            // the chain runs forward: the first k with position_k >= limit (the chain never decreases: a search)
            const float limit = (float)(sm.loop_type == kNoLoop ? sm.length : sm.loop_end);
            const float p0 = ch.sample_position;
            m = cap;
            float pm = afg_mod::chain_jump(p0, ch.step, cap);
            if (pm >= limit) {
                uint32_t lo = 1, hi = cap;                   // position_hi >= limit
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (afg_mod::chain_jump(p0, ch.step, mid) >= limit) hi = mid; else lo = mid + 1;
                }
                m = lo;
                // the last frame's own step, with its branch
                ch.sample_position = afg_mod::chain_jump(p0, ch.step, m - 1);
                advance(sm, ch);
            } else {
                ch.sample_position = pm;
            }
        } else {
            // backwards, or a step that is not a finite number >= 0: frame by frame, the start of every group of 16 noted
            g.flags |= AFG_XM_SEG_TABLE | (forward ? 0u : AFG_XM_SEG_BACK);
            g.aux_pos = (uint32_t)rec.aux.size();
            m = 0;
            while (m < cap) {
                if (m == 0 || ((frame + m) & 15u) == 0) rec.aux.push_back(ch.sample_position);
                m++;
                if (advance(sm, ch) || ch.sample_position < 0) break;
            }
        }
        g.frames = m;
        if (ramp) {
            g.flags |= AFG_XM_SEG_RAMP;
            g.aux_vol = (uint32_t)rec.aux.size();
            for (uint32_t k = 0; k < m; k++) {
                rec.aux.push_back(ch.actual_volume[0]);
                rec.aux.push_back(ch.actual_volume[1]);
                slide_towards(ch.actual_volume[0], ch.target_volume[0], kVolumeRamp);
                slide_towards(ch.actual_volume[1], ch.target_volume[1], kVolumeRamp);
            }
        }
        if (fade) {
            g.flags |= AFG_XM_SEG_FADE;
            g.aux_fade = (uint32_t)rec.aux.size();
            for (uint32_t k = 0; k < m; k++) rec.aux.push_back(ch.end_of_previous_sample[ch.frame_count + k]);
        }
        rec.segs.push_back(g);
        ch.frame_count += m;
        frame += m;
        left -= m;
    }
}

uint64_t Song::render(uint64_t frames, bool stop_at_loop, Records &rec)
{
    uint64_t produced = 0;
    while (produced < frames) {
        if (remaining_ <= 0) {
            tick();
            if (stop_at_loop && loop_count_ >= 1) break;     // the batch path ends before the tick that raised the loop count
        }
        // frames until remaining_samples_in_tick, decremented per frame, is <= 0: ceil(remaining); the decrements are exact
        // while the result stays >= 0, so only a tick's last one is a real subtraction
        uint64_t avail;
        const bool endless = !(remaining_ < 1.0e9f);
        if (endless) avail = frames - produced;
        else {
            const float fl = std::floor(remaining_);
            avail = (uint64_t)fl + (fl == remaining_ ? 0 : 1);
        }
        // a tick record covers at most kMaxTickFrames: the mixer walks a record's segments once per 1024 frames, and a tick
        // may be endless (a BPM of 0); the pieces of a long tick are mixed like the pieces a read's end makes
        const uint32_t n = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(avail, frames - produced), kMaxTickFrames);
        afg_xm_tick t;
        std::memset(&t, 0, sizeof(t));
        t.frame = (uint32_t)produced;
        t.frames = n;
        t.seg = (uint32_t)rec.segs.size();
        t.scale = global_volume_ * kAmplification;
        t.table_index = table_index_;
        t.row = row_;
        t.loop_count = loop_count_;
        if (loop_count_ < 1) {
            for (int i = 0; i < num_channels_; i++) {
                Chan &ch = ch_[(size_t)i];
                if (ch.instrument == nullptr || ch.sample == nullptr || ch.sample_position < 0) continue;
                mix_channel(i, ch, n, t.frame, rec);
            }
        }
        t.n_seg = (uint32_t)rec.segs.size() - t.seg;
        rec.ticks.push_back(t);
        if (!endless) {
            if (n == avail) { remaining_ = remaining_ - (float)(n - 1); remaining_ = remaining_ - 1.0f; }
            else remaining_ = remaining_ - (float)n;
        }
        produced += n;
        if (rec.bytes() > kMaxRecordBytes) { rec.overflow = true; break; }
    }
    return produced;
}

const char *const kMessageTooManyRecords = "XM: the song needs more than 1 GiB of mixing records (kMaxRecordBytes)";

uint64_t render_song(Song &song, Records &rec, bool *capped)
{
    const uint64_t n = song.render((uint64_t)AFG_MOD_MAX_FRAMES, true, rec);
    if (capped) *capped = n >= (uint64_t)AFG_MOD_MAX_FRAMES && song.loop_count() < 1;
    return n;
}

}  // namespace afg_xm
