// afg_mod_front.h -- ProTracker MOD on the host: probe, init and the control layer of pocketmod.d as a tick-by-tick state
// machine that emits the mixer's work as afg_mod_tick / afg_mod_segment records (include/afg.h).  The device mixer is
// csrc/mod_mix.hip; the position chain both sides share is csrc/mod_chain.h.
#pragma once
#include "afg_stage.h"

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace afg_mod {

constexpr int kRate = 44100;             // stream.d:1816: pocketmod_init(..., 44100)
constexpr int kMaxChannels = 32;         // POCKETMOD_MAX_CHANNELS
constexpr int kPlanePad = 16;            // zero bytes after the sample area: the mixer may read one byte past the last sample

// True when the stream probe would open the file as a MOD: at least 600 bytes, _pocketmod_ident on the first 1084
// (pocketmod.d:724-811), then pocketmod_init (:813-906) -- and not a file the WAV or XM probe claims first.
// `song` (optional) receives the initialised module, ready to play.
class Song;
bool probe(const uint8_t *data, size_t size, Song *song = nullptr);

// One module being played.  The file bytes are not copied: they must outlive the Song.
class Song {
public:
    bool init(const uint8_t *data, size_t size);           // pocketmod_init(c, data, size, 44100)

    // pocketmod_render(c, buffer, frames * 8) (pocketmod.d:908-952) without the mixing: appends the read's ticks and segments
    // (frames relative to `frame0`, segment indexes relative to `seg0`) and returns the frames the read produces.
    int render(int frames, uint32_t frame0, uint32_t seg0, std::vector<afg_mod_tick> &ticks, std::vector<afg_mod_segment> &segs);

    void seek(int pattern, int row, int tick);              // pocketmod_seek (pocketmod.d:954-962)

    int loop_count() const { return loop_count_; }
    int num_channels() const { return num_channels_; }
    int num_patterns() const { return num_patterns_; }
    int length() const { return length_; }
    int pattern() const { return pattern_; }
    int line() const { return line_; }
    // the sample area of the file followed by kPlanePad zero bytes: what segments' sample_off index
    const std::vector<uint8_t> &plane() const { return plane_; }

private:
    struct Chan {
        uint8_t dirty = 0, sample = 0, volume = 0, balance = 0;
        uint16_t period = 0, delayed = 0, target = 0;
        uint8_t finetune = 0, loop_count = 0, loop_line = 0, lfo_step = 0;
        uint8_t lfo_type[2] = { 0, 0 };
        uint8_t effect = 0, param = 0, param3 = 0, param4 = 0, param7 = 0, param9 = 0;
        uint8_t paramE1 = 0, paramE2 = 0, paramEA = 0, paramEB = 0, real_volume = 0;
        float position = 0.0f, increment = 0.0f;
    };
    struct SampleSlot { uint32_t off = 0, length = 0; };    // off: in the plane

    uint8_t byte(size_t off) const { return off < size_ ? data_[off] : 0; }
    const uint8_t *header(int sample) const { return data_ + 12 + 30 * sample; }   // POCKETMOD_SAMPLE (sample >= 1)
    uint8_t order(int pattern) const;

    void next_line();                                       // pocketmod.d:354-530
    void next_tick();                                       // pocketmod.d:532-662
    void update_pitch(Chan &ch);                            // pocketmod.d:227-258
    void update_volume(Chan &ch);                           // pocketmod.d:260-269
    int lfo(const Chan &ch, int step) const;                // pocketmod.d:216-225
    void mix_channel(int index, Chan &ch, int frames, uint32_t frame, std::vector<afg_mod_segment> &segs);   // :664-721

    const uint8_t *data_ = nullptr;
    size_t size_ = 0;
    size_t order_at_ = 0, patterns_at_ = 0;
    int length_ = 0, reset_ = 0, num_patterns_ = 0, num_samples_ = 0, num_channels_ = 0;
    SampleSlot samples_[31];
    std::vector<uint8_t> plane_;

    int ticks_per_line_ = 6;
    float samples_per_tick_ = 0.0f;
    uint8_t visited_[32] = {};
    int loop_count_ = 0;
    Chan ch_[kMaxChannels];
    uint8_t pattern_delay_ = 0;
    uint32_t lfo_rng_ = 0;
    int8_t pattern_ = 0, line_ = 0;
    int16_t tick_ = 0;
    float sample_ = 0.0f;
};

// The batch path's definition of a whole song (afg.h): reads of AFG_MOD_MAX_FRAMES minus the frames so far until the song
// has looped once or the cap is reached.  Appends song-relative records; returns the frames; *capped set when cut.
uint64_t render_song(Song &song, std::vector<afg_mod_tick> &ticks, std::vector<afg_mod_segment> &segs, bool *capped);

}  // namespace afg_mod

// ---------------------------------------------------------------------------------------------
// The device side of MOD decoding (afg_mod_stage.cpp)
// ---------------------------------------------------------------------------------------------
namespace afg_mod {

// A MOD stream: each read runs the control layer for exactly the read's frames and mixes them on the device.
class StreamMix {
public:
    // pocketmod_render(c, out, frames * 8) behind stream.d:611-620; -1: device error (afg_last_error says which)
    int read(void *out, int frames, bool f64 = false);   // f64: doubles, widened on the device (stream.d:732-739)
    Song song;
private:
    afg_front::DevBuf plane_, recs_, out_;
    bool uploaded_ = false;
    afg_front::HandleStream stream_;
    std::vector<afg_mod_tick> ticks_;
    std::vector<afg_mod_segment> segs_;
    std::vector<uint8_t> staging_;
    afg_front::PlaneFetch fetch_;
};

// The batch path's MOD stage: the files listed in `which` that pass the probe are simulated on the helper threads
// (n_threads as afg_front::parallel_run takes it), mixed on the current device in chunks with upload, mix and download overlapped,
// and their items filled in (2-channel float PCM in page-locked memory that `keep` owns).  Other files are left alone.
int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so = afg_front::SampleOut());   // f64: items point at doubles (afg_batch_opts.sample_type)

// What the stage reports on a song cut at AFG_MOD_MAX_FRAMES (status AFG_OK)
extern const char *const kMessageCapped;

}  // namespace afg_mod
