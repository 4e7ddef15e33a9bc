// afg_stream.cpp -- the AudioStream-shaped surface of the C ABI (stream.d:150-170 openFromMemory, :295-412 getters,
// :429-637 readSamplesFloat): open probes the formats in the reference's order, a read decodes the next chunk of the file
// through decode_parsed (afg_batch.cpp) on the device and serves interleaved samples.
#include "afg_batch.h"
#include "afg_mod_front.h"
#include "afg_wav_front.h"
#include "afg_write_stream.h"
#include "afg_xm_front.h"

#include <new>

using namespace afg_front;

// The AudioStream surface decodes as the caller pulls (stream.d:429-637 keeps O(1) state per stream): open parses
// the container only, a read decodes the next chunk of frames (about 1.5 s of audio) on the device when the FIFO of
// delivered samples runs dry.  Memory per handle: the file bytes (the reference copies them too, stream.d:2031-2041),
// one chunk of PCM, and for MP3 the 6 KB decoder state that lives on the device between chunks.
struct afg_stream {
    const char *error = kErrorNotInitialized;      // stream.d:1379
    int format = AFG_FORMAT_UNKNOWN, channels = 0;
    float samplerate = 0;
    int64_t declared_frames = AFG_UNKNOWN_LENGTH;
    std::vector<uint8_t> bytes;
    // per-format readers
    FlacInfo fi;
    size_t flac_pos = 0;
    QoaInfo qi;
    std::vector<afg_qoa_frame> qoa;
    size_t qoa_next = 0;
    std::unique_ptr<afg_mp3::Reader> mp3;
    std::unique_ptr<afg_vorbis::Reader> ogg;
    std::unique_ptr<afg_opus::Reader> opus;
    std::unique_ptr<afg_mod::StreamMix> mod;
    std::unique_ptr<afg_xm::StreamMix> xm;
    std::unique_ptr<afg_wav::StreamConv> wav;
    bool wav_failed = false;            // a WAV read has failed: the stream is in error state and still tells its position
    Mp3Carry carry;
    OpusCarry opus_carry;
    int opus_gain_i = 0;
    float opus_gain = 1.0f;
    int64_t opus_decoded = 0;           // frames decoded so far (the declared length cuts the delivery, stream.d:439-442)
    bool opus_failed = false;           // a packet could not be framed: the next refill reports it (stream.d:452-456)
    // delivered samples not yet read
    std::vector<uint8_t> fifo;          // samples of fifo_es bytes: floats, or doubles once afg_read_samples_double is in use
    size_t fifo_es = sizeof(float);
    size_t fifo_at = 0;                 // samples of `fifo` already handed out
    bool decoded = false;               // a chunk has been decoded since the readers were (re)started
    size_t fifo_samples() const { return fifo.size() / fifo_es; }
    int64_t position = 0;               // frames handed out so far (tellPosition)
    bool ended = false;                 // nothing further can be decoded
    afg_write::Writer *writer = nullptr;    // opened for writing (afg_write_stream.cpp): nothing above is in use
    ~afg_stream() { if (writer) afg_write::destroy(writer); }

    static constexpr int kMp3Frames = 64, kOggPackets = 64, kFlacFrames = 16, kQoaFrames = 16, kOpusPackets = 64;

    // (re)start the readers at the head of the stream
    bool rewind()
    {
        fifo.clear();
        fifo_at = 0;
        position = 0;
        ended = false;
        decoded = false;
        flac_pos = 0;
        qoa_next = 0;
        carry.valid = carry.continues = false;
        opus_carry.valid = false;
        opus_decoded = 0;
        opus_failed = false;
        if (format == AFG_FORMAT_OPUS) {
            afg_opus::File meta;
            opus.reset(new afg_opus::Reader);
            return opus->open(bytes.data(), bytes.size(), meta) == afg_opus::kOpened;
        }
        if (format == AFG_FORMAT_MP3) {
            afg_mp3::File meta;
            mp3.reset(new afg_mp3::Reader);
            return mp3->open(bytes.data(), bytes.size(), meta);
        }
        if (format == AFG_FORMAT_OGG) {
            afg_vorbis::File meta;
            ogg.reset(new afg_vorbis::Reader);
            return ogg->open(bytes.data(), bytes.size(), meta, vorbis_floor_on_device());
        }
        return true;
    }

    // decode the next chunk into the FIFO; false: end of stream (or error state set)
    bool refill()
    {
        if (ended) return false;
        if (fifo_at == fifo_samples()) { fifo.clear(); fifo_at = 0; }
        decoded = true;
        std::vector<Parsed> parsed(1);
        Parsed &p = parsed[0];
        const uint8_t *dp[1] = { bytes.data() };
        size_t lp[1] = { bytes.size() };
        Mp3Decode mp3_stage;
        OpusDecode opus_stage;
        if (format == AFG_FORMAT_OPUS) {
            if (opus_failed) { error = kErrorDecoderInitializationFailed; ended = true; return false; }      // stream.d:454
            if (opus_decoded >= declared_frames || !opus->more(p.opus, kOpusPackets)) { ended = true; return false; }
            if (p.opus.error) opus_failed = true;
            p.opus.error = false;                               // this chunk's good frames are delivered first
            if (p.opus.frames.empty()) { error = kErrorDecoderInitializationFailed; ended = true; return false; }
            p.opus.channels = channels;
            p.opus.gain_i = opus_gain_i;
            p.opus.gain = opus_gain;
            p.opus.declared_frames = declared_frames - opus_decoded;
            opus_decoded += (int64_t)p.opus.pcm_frames;
            opus_stage.carry = &opus_carry;
            p.format = AFG_FORMAT_OPUS;
        } else if (format == AFG_FORMAT_FLAC) {
            bool done = false;
            p.fi = fi;
            p.flac.pack16 = flac_rows_int16();
            const int got = flac_parse_frames(bytes.data(), bytes.size(), fi, p.flac, &flac_pos, kFlacFrames, &done);
            if (done) ended = true;
            if (!got) { ended = true; return false; }
            p.format = AFG_FORMAT_FLAC;
        } else if (format == AFG_FORMAT_QOA) {
            if (qoa_next >= qoa.size()) { ended = true; return false; }
            const size_t k1 = std::min(qoa.size(), qoa_next + (size_t)kQoaFrames);
            const uint64_t byte0 = qoa[qoa_next].byte_off, out0 = qoa[qoa_next].out_off;
            for (size_t k = qoa_next; k < k1; k++) {
                afg_qoa_frame f = qoa[k];
                f.byte_off -= byte0;
                f.out_off -= out0;
                p.qoa.push_back(f);
            }
            const uint64_t byte1 = k1 < qoa.size() ? qoa[k1].byte_off : (uint64_t)bytes.size();
            dp[0] = bytes.data() + byte0;
            lp[0] = (size_t)(byte1 - byte0);
            p.qi = qi;
            p.format = AFG_FORMAT_QOA;
            qoa_next = k1;
            if (qoa_next >= qoa.size()) ended = true;
        } else if (format == AFG_FORMAT_OGG) {
            if (!ogg->more(p.ogg, kOggPackets)) { ended = true; return false; }
            p.format = AFG_FORMAT_OGG;
        } else if (format == AFG_FORMAT_MP3) {
            bool continues = false;
            if (!mp3->more(p.mp3, kMp3Frames, &continues)) { ended = true; return false; }
            carry.continues = continues;
            mp3_stage.carry = &carry;
            p.format = AFG_FORMAT_MP3;
        } else {
            ended = true;
            return false;
        }
        BatchOut out;
        StageCtx ctx = stage_ctx(parsed, dp, lp, nullptr, 1, fifo_es == sizeof(double), out);
        FlacDecode flac_stage;
        VorbisDecode ogg_stage;
        if (decode_parsed(ctx, flac_stage, mp3_stage, ogg_stage, opus_stage) != AFG_OK || out.files[0].status != AFG_OK) {
            error = kErrorDecodingError;
            ended = true;
            return false;
        }
        const Decoded &d = out.files[0];
        const size_t want = (size_t)std::max<int64_t>(d.frames, 0) * (size_t)channels;
        if (want) {
            if (d.pcm_off + want > out.plane_floats) { error = kErrorDecodingError; ended = true; return false; }
            const uint8_t *src = (const uint8_t *)out.plane.p + d.pcm_off * fifo_es;
            fifo.insert(fifo.end(), src, src + want * fifo_es);
        }
        return true;
    }

    // decode and drop until `frame` (or the end of what decodes)
    void skip_to(int64_t frame)
    {
        const size_t C = (size_t)std::max(1, channels);
        while (position < frame) {
            if (fifo_at == fifo_samples() && !refill()) break;
            const size_t avail = (fifo_samples() - fifo_at) / C;
            const size_t n = std::min<size_t>(avail, (size_t)(frame - position));
            fifo_at += n * C;
            position += (int64_t)n;
        }
    }

    // Reads of the other sample type from here on.  A change of type is a seek to the current position: what the FIFO
    // holds was decoded in the old type and is dropped, the readers start over and the chunks up to the position are
    // decoded again, so that the next read returns what a handle that only ever used the new type returns there.
    bool set_sample_bytes(size_t es)
    {
        if (fifo_es == es) return true;
        const int64_t at = position;
        const bool start_over = decoded;
        fifo.clear();
        fifo_at = 0;
        fifo_es = es;
        if (!start_over) return true;
        if (!rewind()) return false;
        skip_to(at);
        return !error && position == at;
    }
};

extern "C" {

afg_stream *afg_open_from_memory(const uint8_t *data, size_t length)
{
    afg_stream *s = new (std::nothrow) afg_stream;
    if (!s) return nullptr;
    if (!data || length == 0) { s->error = kErrorUnknownFormat; return s; }
    try {
        s->bytes.assign(data, data + length);
        const uint8_t *d = s->bytes.data();
        // startDecoding's probe order for the formats handled here (stream.d:1586-1838): FLAC, QOA, OGG, then MP3
        afg_mp3::File m3;
        afg_vorbis::File og;
        afg_opus::File op;
        // the reference tries Opus before anything else (stream.d:1596-1614)
        afg_opus::Status ost = afg_opus::kNotOpus;
        if (length >= 4 && std::memcmp(d, "OggS", 4) == 0) {
            s->opus.reset(new afg_opus::Reader);
            ost = s->opus->open(d, length, op);
        }
        if (ost == afg_opus::kUnsupported) {
            s->error = kErrorOpusMode;
            return s;
        }
        if (ost == afg_opus::kOpened) {
            s->format = AFG_FORMAT_OPUS;
            s->channels = op.channels;
            s->samplerate = 48000.0f;                                     // OpusFileCtx.rate, stream.d:1607
            s->declared_frames = op.declared_frames;                      // smpduration(), stream.d:1609
            s->opus_gain_i = op.gain_i;
            s->opus_gain = op.gain;
        } else if (flac_open_info(d, length, s->fi)) {
            s->format = AFG_FORMAT_FLAC;
            s->channels = (int)s->fi.channels;
            s->samplerate = (float)s->fi.sample_rate;
            s->declared_frames = (int64_t)s->fi.total_samples;            // totalSampleCount / channels, stream.d:1631
        } else if ((s->wav.reset(new afg_wav::StreamConv), afg_wav::scan(d, length, &s->wav->info) == nullptr)) {   // stream.d:1638-1655
            s->format = AFG_FORMAT_WAV;
            s->channels = s->wav->info.channels;
            s->samplerate = (float)s->wav->info.sample_rate;
            s->declared_frames = (int64_t)s->wav->info.frames;
        } else if ((s->wav.reset(), qoa_parse(d, length, s->qi, s->qoa))) {
            s->format = AFG_FORMAT_QOA;
            s->channels = (int)s->qi.channels;
            s->samplerate = (float)s->qi.samplerate;
            s->declared_frames = (int64_t)s->qi.samples;
        } else if ((s->ogg.reset(new afg_vorbis::Reader), s->ogg->open(d, length, og, vorbis_floor_on_device()))) {
            s->format = AFG_FORMAT_OGG;
            s->channels = og.channels;
            s->samplerate = (float)og.sample_rate;
            s->declared_frames = (int64_t)og.total_samples;               // stb_vorbis_stream_length_in_samples, stream.d:1696
        } else if (afg_mp3::looks_like_mp3(d, length) && (s->mp3.reset(new afg_mp3::Reader), s->mp3->open(d, length, m3))) {
            s->format = AFG_FORMAT_MP3;
            s->channels = m3.channels;
            s->samplerate = (float)m3.hz;
            s->declared_frames = (int64_t)(m3.declared_samples / (uint64_t)std::max(1, m3.channels));   // stream.d:1737
        } else if ((s->xm.reset(new afg_xm::StreamMix), afg_xm::probe(d, length, &s->xm->song))) {   // stream.d:1751-1793
            s->format = AFG_FORMAT_XM;
            s->channels = 2;
            s->samplerate = 44100.0f;
            s->declared_frames = AFG_UNKNOWN_LENGTH;
        } else if ((s->xm.reset(), s->mod.reset(new afg_mod::StreamMix), afg_mod::probe(d, length, &s->mod->song))) {   // tried last (stream.d:1796-1830)
            s->format = AFG_FORMAT_MOD;
            s->channels = 2;
            s->samplerate = 44100.0f;
            s->declared_frames = AFG_UNKNOWN_LENGTH;
        } else {
            s->error = kErrorUnknownFormat;
            return s;
        }
        if (afg::require_device() != AFG_OK) { s->error = kErrorDecoderInitializationFailed; return s; }
        s->error = nullptr;
    } catch (...) {
        s->error = kErrorDecoderInitializationFailed;      // out of memory
    }
    return s;
}

int afg_is_error(const afg_stream *s) { return !s || s->error != nullptr; }
const char *afg_error_message(const afg_stream *s) { return s ? s->error : kErrorNotInitialized; }
int afg_get_format(const afg_stream *s) { return (s && !s->error) ? s->format : AFG_FORMAT_UNKNOWN; }
int afg_get_num_channels(const afg_stream *s) { return (s && !s->error) ? s->channels : 0; }
float afg_get_samplerate(const afg_stream *s) { return (s && !s->error) ? s->samplerate : 0.0f; }

int64_t afg_get_length_in_frames(const afg_stream *s)
{
    if (!s || s->error) return AFG_UNKNOWN_LENGTH;
    return s->declared_frames;         // stream.d:404-407: whatever the container declares (FLAC: may be 0)
}

static int read_samples(afg_stream *s, void *out, int frames, bool f64)
{
    if (!s || s->error || s->writer || frames <= 0) return 0;
    // stream.d:498 / :705: a FLAC stream stops once the position equals the declared length (a STREAMINFO that
    // declares 0 samples therefore reads nothing); the check is made on entry only, like the reference's.
    if (s->format == AFG_FORMAT_FLAC && s->position == s->declared_frames) return 0;
    const size_t es = f64 ? sizeof(double) : sizeof(float);
    try {
        if (s->format == AFG_FORMAT_WAV) {                       // stream.d:557-570, :719-730
            bool failed = false;
            const int n = s->wav->read(s->bytes.data(), s->bytes.size(), out, frames, &failed, f64);
            s->position = s->wav->tell();
            if (n < 0 || failed) { s->error = kErrorDecodingError; s->wav_failed = true; return 0; }
            return n;
        }
        if (s->format == AFG_FORMAT_MOD || s->format == AFG_FORMAT_XM) {
            const int n = s->format == AFG_FORMAT_XM ? s->xm->read(out, frames, f64) : s->mod->read(out, frames, f64);
            if (n < 0) { s->error = kErrorDecodingError; return 0; }
            s->position += n;
            return n;
        }
        if (!s->set_sample_bytes(es)) {
            if (!s->error) s->error = kErrorDecodingError;
            return 0;
        }
        const size_t C = (size_t)std::max(1, s->channels);
        int done = 0;
        while (done < frames) {
            if (s->fifo_at == s->fifo_samples() && !s->refill()) break;
            const size_t avail = (s->fifo_samples() - s->fifo_at) / C;
            const size_t n = std::min<size_t>(avail, (size_t)(frames - done));
            if (out && n) std::memcpy((uint8_t *)out + (size_t)done * C * es, s->fifo.data() + s->fifo_at * es, n * C * es);
            s->fifo_at += n * C;
            done += (int)n;
        }
        if (s->error && s->format == AFG_FORMAT_OPUS) return 0;   // stream.d:452-456: the failing read returns 0
        s->position += done;
        return done;
    } catch (...) {
        s->error = kErrorDecodingError;
        return 0;
    }
}

int afg_read_samples_float(afg_stream *s, float *out, int frames) { return read_samples(s, out, frames, false); }
int afg_read_samples_double(afg_stream *s, double *out, int frames) { return read_samples(s, out, frames, true); }

int afg_can_seek(const afg_stream *s) { return s && !s->error && !s->writer; }

int afg_seek_position(afg_stream *s, int frame)
{
    if (!s || s->error || s->writer) return 0;
    if (s->format == AFG_FORMAT_MOD || s->format == AFG_FORMAT_XM) return 0;   // a module seeks by pattern and row (afg_module_seek; stream.d:1097)
    if (s->format == AFG_FORMAT_WAV) {                           // stream.d:1197-1199
        if (!s->wav->seek(frame)) return 0;
        s->position = frame;
        return 1;
    }
    // the reference bounds a seek by the declared length (stream.d:1104, :1113, :1137); what can actually be reached is
    // bounded by what decodes.  Backwards: the readers start over; forwards: chunks are decoded and dropped (a chunk
    // is ~1.5 s of audio and takes about a millisecond on the device).
    const int64_t limit = std::max<int64_t>(s->declared_frames, 0);
    if (frame < 0 || frame > limit) return 0;
    try {
        if (frame < s->position) {
            // still inside the FIFO?  then just step back
            const size_t C = (size_t)std::max(1, s->channels);
            const int64_t fifo_first = s->position - (int64_t)(s->fifo_at / C);
            if (frame >= fifo_first) {
                s->fifo_at -= (size_t)(s->position - frame) * C;
                s->position = frame;
                return 1;
            }
            if (!s->rewind()) { s->error = kErrorDecodingError; return 0; }
        }
        s->skip_to(frame);
        return s->error ? 0 : 1;
    } catch (...) {
        s->error = kErrorDecodingError;
        return 0;
    }
}

int afg_tell_position(const afg_stream *s)
{
    if (s && s->wav_failed && s->wav) return s->wav->tell();    // wav.d:253: the failed read has moved the position
    return (s && !s->error) ? (int)s->position : -1;
}

void afg_close(afg_stream *s) { delete s; }
int afg_is_open_for_reading(const afg_stream *s) { return s && !s->writer && s->error != kErrorNotInitialized; }   // stream.d:377-391
int afg_is_open_for_writing(const afg_stream *s) { return s && s->writer; }

// the module functions of AudioStream (stream.d:330-345, :906-1080)
static const afg_mod::Song *module_of(const afg_stream *s) { return (s && !s->error && s->format == AFG_FORMAT_MOD && s->mod) ? &s->mod->song : nullptr; }
static afg_xm::Song *xm_of(const afg_stream *s) { return (s && !s->error && s->format == AFG_FORMAT_XM && s->xm) ? &s->xm->song : nullptr; }
int afg_is_module(const afg_stream *s) { return (module_of(s) || xm_of(s)) ? 1 : 0; }
int afg_module_pattern_count(const afg_stream *s)
{
    if (const afg_xm::Song *x = xm_of(s)) return x->num_patterns();
    const afg_mod::Song *m = module_of(s);
    return m ? m->num_patterns() : -1;
}
int afg_module_length(const afg_stream *s)
{
    if (const afg_xm::Song *x = xm_of(s)) return x->length();
    const afg_mod::Song *m = module_of(s);
    return m ? m->length() : -1;
}
int afg_module_rows_in_pattern(const afg_stream *s, int pattern)
{
    if (const afg_xm::Song *x = xm_of(s)) return x->rows(pattern);   // stream.d:977-984
    return module_of(s) ? 64 : -1;                                    // stream.d:971-975
}
int afg_module_tell_pattern(const afg_stream *s)
{
    if (const afg_xm::Song *x = xm_of(s)) return x->table_index();
    const afg_mod::Song *m = module_of(s);
    return m ? m->pattern() : -1;
}
int afg_module_tell_row(const afg_stream *s)
{
    if (const afg_xm::Song *x = xm_of(s)) return x->row();
    const afg_mod::Song *m = module_of(s);
    return m ? m->line() : -1;
}
int afg_module_seek(afg_stream *s, int pattern, int row)
{
    if (afg_xm::Song *x = xm_of(s)) return x->seek(pattern, row) ? 1 : 0;   // stream.d:1078
    if (!module_of(s)) return 0;
    s->mod->song.seek(pattern, row, 0);                 // stream.d:1075
    return 1;
}

}  // extern "C"

// the handle's side of a write stream, and the helper threads for the batch encoder (afg_write_stream.h)
namespace afg_front {
afg_stream *stream_for_writing(afg_write::Writer *w, int format, int channels, float samplerate, const char *error)
{
    afg_stream *s = new (std::nothrow) afg_stream;
    if (!s) return nullptr;
    s->writer = w;
    s->format = format;
    s->channels = channels;
    s->samplerate = samplerate;
    s->error = error;
    return s;
}
afg_write::Writer *stream_writer(const afg_stream *s) { return s ? s->writer : nullptr; }
void stream_set_error(afg_stream *s, const char *message) { if (s) s->error = message; }
}  // namespace afg_front
