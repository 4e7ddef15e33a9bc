// afg_xm_front.h -- FastTracker II XM on the host: the loader (libxm.d:360-855) and the control layer (libxm.d:1154-2311)
// as a tick-by-tick state machine that emits the mixer's work as afg_xm_tick / afg_xm_segment records and a side table of
// floats (include/afg.h).  The device mixer is csrc/xm_mix.hip; forward position chains are jumped with csrc/mod_chain.h.
#pragma once
#include "afg_mod_front.h"                                  // kMessageCapped
#include "afg_stage.h"

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace afg_xm {

constexpr int kRate = 44100;             // stream.d:1765: xm_create_context_safe(..., 44100)
constexpr int kMaxChannels = 32;
constexpr int kRampPoints = 32;          // XM_SAMPLE_RAMPING_POINTS
// What one render call may write down.  A loaded file bounds its patterns and samples, not its records: a header BPM of 65535
// makes ticks of under two frames, and 32 channels in loops of a few samples then write about 1 KB of records per output
// frame.  1 GiB also keeps every 32-bit record and side-table index far below 2^32.
constexpr size_t kMaxRecordBytes = (size_t)1 << 30;
extern const char *const kMessageTooManyRecords;

// What one render call writes down: ticks, segments and the side table, all relative to the call's first frame
struct Records {
    std::vector<afg_xm_tick> ticks;
    std::vector<afg_xm_segment> segs;
    std::vector<float> aux;
    bool overflow = false;                                  // the call stopped at kMaxRecordBytes
    size_t bytes() const { return ticks.size() * sizeof(afg_xm_tick) + segs.size() * sizeof(afg_xm_segment) + aux.size() * sizeof(float); }
    void clear() { ticks.clear(); segs.clear(); aux.clear(); overflow = false; }
};

class Song;
// True when the stream probe opens the file as an XM: xm_create_context_safe returns 0 (libxm.d:856-932), within the
// bounds INTEGRATION.md lists.  `song` (optional) receives the loaded module, ready to play.
bool probe(const uint8_t *data, size_t size, Song *song = nullptr);

class Song {
public:
    bool load(const uint8_t *data, size_t size);            // the file bytes are not kept

    // xm_generate_samples(ctx, out, frames) (libxm.d:2429-2483) without the mixing: appends the call's records and returns
    // the frames it covers.  stop_at_loop: return before the tick that finds the loop count >= 1 (the batch path).
    // Stops early, with rec.overflow set, once the records pass kMaxRecordBytes: the caller refuses the song.
    uint64_t render(uint64_t frames, bool stop_at_loop, Records &rec);

    bool seek(int pot, int row);                            // xm_seek(ctx, pot, row, 0), libxm.d:951-959

    int loop_count() const { return loop_count_; }
    int num_channels() const { return num_channels_; }
    int num_patterns() const { return num_patterns_; }
    int num_instruments() const { return (int)instruments_.size(); }
    int length() const { return length_; }
    int restart() const { return restart_; }
    int rows(int pattern) const { return (pattern < 0 || pattern >= num_patterns_) ? -1 : (int)patterns_[(size_t)pattern].num_rows; }
    int table_index() const { return table_index_; }
    int row() const { return row_; }
    // every sample delta-decoded: int8, or int16 in host byte order at even offsets
    const std::vector<uint8_t> &sample_data() const { return data_; }

private:
    struct Envelope {
        uint16_t frame[12] = {}, value[12] = {};
        uint8_t num_points = 0, sustain_point = 0, loop_start_point = 0, loop_end_point = 0;
        bool enabled = false, sustain_enabled = false, loop_enabled = false;
    };
    struct Sample {
        uint8_t bits = 8;
        uint32_t length = 0, loop_start = 0, loop_length = 0, loop_end = 0;
        float volume = 0.0f, panning = 0.0f;
        int8_t finetune = 0, relative_note = 0;
        int loop_type = 0;
        uint32_t off = 0;                                   // in data_
    };
    struct Instrument {
        uint16_t num_samples = 0;
        uint8_t sample_of_notes[96] = {};
        Envelope volume_envelope, panning_envelope;
        int vibrato_type = 0;
        uint8_t vibrato_sweep = 0, vibrato_depth = 0, vibrato_rate = 0;
        uint16_t volume_fadeout = 0;
        std::vector<Sample> samples;
    };
    struct Slot {
        uint8_t note = 0, instrument = 0, volume_column = 0, effect_type = 0, effect_param = 0;
        bool has_tone_portamento() const { return effect_type == 3 || effect_type == 5 || (volume_column >> 4) == 0xF; }
        bool has_arpeggio() const { return effect_param != 0; }
        bool has_vibrato() const { return effect_type == 4 || effect_type == 6 || (volume_column >> 4) == 0xB; }
    };
    struct Pattern { uint16_t num_rows = 0; std::vector<Slot> slots; };
    struct Chan {
        float note = 0, orig_note = 0;
        const Instrument *instrument = nullptr;
        const Sample *sample = nullptr;
        Slot current;
        float sample_position = 0, period = 0, frequency = 0, step = 0;
        bool ping = true;
        float volume = 1.0f, panning = 0.5f;
        uint16_t autovibrato_ticks = 0;
        bool sustained = false;
        float fadeout_volume = 1.0f, volume_envelope_volume = 1.0f, panning_envelope_panning = 0.5f;
        uint16_t volume_envelope_frame_count = 0, panning_envelope_frame_count = 0;
        float autovibrato_note_offset = 0;
        bool arp_in_progress = false;
        uint8_t arp_note_offset = 0, volume_slide_param = 0, fine_volume_slide_param = 0, global_volume_slide_param = 0;
        uint8_t panning_slide_param = 0, portamento_up_param = 0, portamento_down_param = 0;
        uint8_t fine_portamento_up_param = 0, fine_portamento_down_param = 0;
        uint8_t extra_fine_portamento_up_param = 0, extra_fine_portamento_down_param = 0, tone_portamento_param = 0;
        float tone_portamento_target_period = 0;
        uint8_t multi_retrig_param = 0, note_delay_param = 0, pattern_loop_origin = 0, pattern_loop_count = 0;
        bool vibrato_in_progress = false;
        int vibrato_waveform = 0;
        bool vibrato_waveform_retrigger = true;
        uint8_t vibrato_param = 0;
        uint16_t vibrato_ticks = 0;
        float vibrato_note_offset = 0;
        int tremolo_waveform = 0;
        bool tremolo_waveform_retrigger = true;
        uint8_t tremolo_param = 0, tremolo_ticks = 0;
        float tremolo_volume = 0;
        uint8_t tremor_param = 0;
        bool tremor_on = false;
        float target_volume[2] = { 0, 0 };
        uint64_t frame_count = 0;
        float end_of_previous_sample[kRampPoints] = {};
        float actual_volume[2] = { 0, 0 };
    };

    float waveform(int type, uint8_t step);
    void autovibrato(Chan &ch);
    void vibrato(Chan &ch, uint8_t param);
    void tremolo(Chan &ch, uint8_t param, uint16_t pos);
    void arpeggio(Chan &ch, uint8_t param, uint16_t tick);
    void tone_portamento(Chan &ch);
    void pitch_slide(Chan &ch, float period_offset);
    float period_of(float note) const;
    float frequency_of(float period, float note_offset, float period_offset) const;
    void update_frequency(Chan &ch);
    void handle_note_and_instrument(Chan &ch, const Slot &s);
    void trigger_note(Chan &ch, unsigned flags);
    void post_pattern_change();
    void row_step();
    void envelopes(Chan &ch);
    void tick();
    float next_of_sample(Chan &ch);
    void mix_channel(int index, Chan &ch, uint32_t frames, uint32_t frame, Records &rec);

    std::vector<uint8_t> data_;
    std::vector<Pattern> patterns_;
    std::vector<Instrument> instruments_;
    uint8_t pattern_table_[256] = {};
    int length_ = 0, restart_ = 0, num_channels_ = 0, num_patterns_ = 0;
    bool linear_ = true;

    uint16_t tempo_ = 0, bpm_ = 0;
    float global_volume_ = 1.0f;
    uint32_t next_rand_ = 24492;
    uint8_t table_index_ = 0, row_ = 0;
    uint16_t current_tick_ = 0;
    float remaining_ = 0.0f;
    bool position_jump_ = false, pattern_break_ = false;
    uint8_t jump_dest_ = 0, jump_row_ = 0;
    uint16_t extra_ticks_ = 0;
    std::vector<uint8_t> row_loop_count_;
    uint8_t loop_count_ = 0;
    std::vector<Chan> ch_;
};

// The batch path's definition of a whole song (afg.h): the frames before the tick that finds the loop count at 1, cut at
// AFG_MOD_MAX_FRAMES (*capped set).
uint64_t render_song(Song &song, Records &rec, bool *capped);

// An XM stream: each read runs the control layer for exactly the read's frames and mixes them on the device.
class StreamMix {
public:
    int read(void *out, int frames, bool f64 = false);      // -1: device error (afg_last_error says which); f64: doubles (stream.d:732-739)
    Song song;
private:
    afg_front::DevBuf data_, recs_, out_;
    bool uploaded_ = false;
    afg_front::HandleStream stream_;
    Records rec_;
    std::vector<uint8_t> staging_;
    afg_front::PlaneFetch fetch_;
};

// The batch path's XM stage, shaped like afg_mod::batch_stage: the files of `which` that pass the probe are simulated on
// the helper threads, mixed in chunks with mix and download overlapped, and their items filled in.
int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so = afg_front::SampleOut());   // f64: items point at doubles (afg_batch_opts.sample_type)

}  // namespace afg_xm
