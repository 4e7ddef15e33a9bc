// afg_write_stream.cpp -- the writing half of AudioStream (stream.d:216-286, :762-902, :1282-1349) for WAV and QOA.
//
// WAV: the header goes out at open; writes queue floats, and whenever about 2^18 samples are queued, and at finalize,
// one upload, one afg_wav_pack_hip launch (csrc/wav_encode.hip) and one download append their bytes.  The dither's draw
// index runs on across writes, so the bytes do not depend on how the caller cuts the signal into writes.
// AFG_DITHER_LIBC with an integer format is the only case that stays on the host writer's loop (afg_wav.cpp, through
// afg_wav_encode_dithered): the reference's draws come from libc rand(), a serial, process-global sequence that no
// lane can enter in the middle.  Doubles written to an fp64 stream are stored as they are (wav.d:538-546).
// QOA: writes queue frames and finalize encodes the stream with one afg_qoa_encode_hip call: the encoder's LMS state
// runs through the whole stream, so there is nothing to win by encoding earlier.
#include "afg_stage.h"
#include "afg_write_stream.h"
#include "../csrc/afg_common.h"
#include "../csrc/qoa_sample.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace afg_write {

namespace {
const char *const kErrorUnsupportedEncodingFormat = "Unsupported encoding format, maybe check your audio-formats configuration";
const char *const kErrorEncodingError = "Encoder encountered an error";
constexpr size_t kFlushSamples = (size_t)1 << 18;
void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
}  // namespace

struct Writer {
    int format = AFG_FORMAT_UNKNOWN, channels = 0, sample_format = AFG_WAV_FP32LE, dither = AFG_DITHER_LIBC;
    uint32_t rate = 0, seed = 0;
    // the sink: a buffer the stream owns, or the caller's memory
    bool to_memory = false;
    uint8_t *mem = nullptr;
    size_t mem_cap = 0, mem_pos = 0;
    std::vector<uint8_t> buf;
    bool finalized = false;
    // WAV
    std::vector<float> queue;           // samples not yet packed
    uint64_t packed = 0;                // samples packed so far: the next draw is 2 * packed
    uint64_t written_frames = 0;
    // QOA: the whole stream, as floats until a write brings doubles, as int16 from then on
    std::vector<float> qoa_f32;
    std::vector<int16_t> qoa_i16;
    bool qoa_int = false;
    uint64_t qoa_frames = 0;
    afg_front::DevBuf d_in, d_out, d_recs;
    std::vector<uint8_t> scratch;
    afg_front::HandleStream own_stream;     // follows the caller's device from write to write

    size_t size() const { return to_memory ? mem_pos : buf.size(); }
    uint8_t *data() { return to_memory ? mem : buf.data(); }
    bool fits(size_t more) const { return !to_memory || more <= mem_cap - mem_pos; }
    // all of it or nothing: memory_write_limited fails the write that would pass the end
    bool append(const uint8_t *p, size_t n)
    {
        if (!fits(n)) return false;
        if (to_memory) {
            if (n) std::memcpy(mem + mem_pos, p, n);
            mem_pos += n;
        } else {
            buf.insert(buf.end(), p, p + n);
        }
        return true;
    }

    // packs the queued samples and appends their bytes
    int flush_wav()
    {
        const size_t count = queue.size();
        if (count == 0) return AFG_OK;
        const size_t bytes = count * (size_t)sample_size(sample_format);
        if (!fits(bytes)) return AFG_ERR_INVALID;
        const bool integer = sample_format <= AFG_WAV_S24LE;
        if (integer && dither == AFG_DITHER_LIBC) {
            // the host writer's loop over a one-channel file of these samples; its header is dropped
            scratch.resize(kWavHeader + bytes);
            if (afg_wav_encode_dithered(queue.data(), count, 1, rate, sample_format, nullptr, nullptr, 0, scratch.data(), scratch.size()) !=
                scratch.size())
                return AFG_ERR_INVALID;
            append(scratch.data() + kWavHeader, bytes);
        } else {
            hipStream_t stream = nullptr;
            if (int rc = own_stream.current(&stream)) return rc;
            afg_wav_pack_span span;
            std::memset(&span, 0, sizeof(span));
            span.count = count;
            span.draw0 = 2 * packed;
            span.seed = seed;
            span.format = (uint8_t)sample_format;
            span.dither = (integer && dither == AFG_DITHER_LCG31) ? 1 : 0;
            const uint64_t tiles = afg_wav_pack_layout(&span, 1);
            const size_t in_floats = (count + 3) & ~(size_t)3, out_bytes = (bytes + 15) & ~(size_t)15;
            if (d_in.alloc(in_floats * sizeof(float)) || d_out.alloc(out_bytes) || d_recs.alloc(sizeof(span))) return AFG_ERR_OOM;
            scratch.resize(bytes);
            AFG_HIP_CHECK(hipMemcpyAsync(d_recs.p, &span, sizeof(span), hipMemcpyHostToDevice, stream));
            AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, queue.data(), count * sizeof(float), hipMemcpyHostToDevice, stream));
            if (int rc = afg_wav_pack_hip(1, (const afg_wav_pack_span *)d_recs.p, tiles, (const float *)d_in.p, in_floats, (uint8_t *)d_out.p,
                                          out_bytes, stream))
                return rc;
            AFG_HIP_CHECK(hipMemcpyAsync(scratch.data(), d_out.p, bytes, hipMemcpyDeviceToHost, stream));
            AFG_HIP_CHECK(hipStreamSynchronize(stream));
            append(scratch.data(), bytes);
        }
        packed += count;
        queue.clear();
        return AFG_OK;
    }

    // bytes the queued samples will take: a write is refused as soon as the file would pass the caller's memory
    size_t pending_bytes() const { return queue.size() * (size_t)sample_size(sample_format); }

    int finalize_wav()
    {
        if (int rc = flush_wav()) return rc;
        // wav.d:572-603, with its 32-bit casts
        const uint64_t data_bytes = (uint64_t)(uint32_t)(sample_size(sample_format) * channels) * written_frames;
        put32(data() + 4, (uint32_t)(4 + (4 + 4 + 16) + (4 + 4 + data_bytes)));
        put32(data() + 40, (uint32_t)data_bytes);
        return AFG_OK;
    }

    int finalize_qoa()
    {
        if (qoa_frames > 0xffffffffull) return AFG_ERR_INVALID;                 // qoa.d:660: the frame count is 32 bits
        const uint64_t size = afg_qoa_encoded_size((uint32_t)qoa_frames, (uint32_t)channels);
        if (to_memory && size > mem_cap) return AFG_ERR_INVALID;
        hipStream_t stream = nullptr;
        if (int rc = own_stream.current(&stream)) return rc;
        afg_qoa_enc_stream rec;
        std::memset(&rec, 0, sizeof(rec));
        rec.samples = (uint32_t)qoa_frames;
        rec.samplerate = rate;
        rec.channels = (uint8_t)channels;
        const size_t n = (size_t)qoa_frames * (size_t)channels, in_bytes = n * (qoa_int ? sizeof(int16_t) : sizeof(float));
        const size_t out_bytes = (size_t)((size + 7) & ~(uint64_t)7);
        if (d_in.alloc(std::max<size_t>(in_bytes, 16)) || d_out.alloc(out_bytes) || d_recs.alloc(sizeof(rec))) return AFG_ERR_OOM;
        AFG_HIP_CHECK(hipMemcpyAsync(d_recs.p, &rec, sizeof(rec), hipMemcpyHostToDevice, stream));
        if (in_bytes)
            AFG_HIP_CHECK(hipMemcpyAsync(d_in.p, qoa_int ? (const void *)qoa_i16.data() : (const void *)qoa_f32.data(), in_bytes,
                                         hipMemcpyHostToDevice, stream));
        if (int rc = afg_qoa_encode_hip(1, (const afg_qoa_enc_stream *)d_recs.p, qoa_int ? (const int16_t *)d_in.p : nullptr,
                                        qoa_int ? nullptr : (const float *)d_in.p, (uint8_t *)d_out.p, stream))
            return rc;
        if (to_memory) {
            AFG_HIP_CHECK(hipMemcpyAsync(mem, d_out.p, (size_t)size, hipMemcpyDeviceToHost, stream));
            mem_pos = (size_t)size;
        } else {
            buf.resize((size_t)size);
            AFG_HIP_CHECK(hipMemcpyAsync(buf.data(), d_out.p, (size_t)size, hipMemcpyDeviceToHost, stream));
        }
        AFG_HIP_CHECK(hipStreamSynchronize(stream));
        return AFG_OK;
    }
};

void destroy(Writer *w) { delete w; }

namespace {

afg_stream *open_any(bool to_memory, uint8_t *data, size_t max_length, int format, float samplerate, int channels,
                     const afg_encoding_options *opts)
{
    Writer *w = new (std::nothrow) Writer;
    if (!w) return nullptr;
    const char *error = nullptr;
    try {
        w->format = format;
        w->channels = channels;
        w->to_memory = to_memory;
        w->mem = data;
        w->mem_cap = data ? max_length : 0;
        const float biased = samplerate + 0.5f;                                // stream.d:1852
        const bool rate_ok = biased > -2147483648.0f && biased < 2147483648.0f;
        const int rate = rate_ok ? (int)biased : 0;
        w->rate = (uint32_t)rate;
        if (opts) {
            w->sample_format = opts->sample_format;
            w->dither = opts->dither;
            w->seed = opts->dither_seed;
        }
        if (format != AFG_FORMAT_WAV && format != AFG_FORMAT_QOA) {
            error = kErrorUnsupportedEncodingFormat;                            // stream.d:1856-1863 (and 'unknown')
        } else if ((opts && opts->struct_size != sizeof(afg_encoding_options)) || (to_memory && !data) || !rate_ok) {
            error = kErrorEncodingError;
        } else if (format == AFG_FORMAT_QOA) {
            // QOAEncoder.initialize, qoa.d:592; the 8-byte file header it leaves room for must fit the caller's memory
            if (rate <= 0 || rate > 0xffffff || channels <= 0 || channels > 8 || (to_memory && max_length < 8)) error = kErrorEncodingError;
        } else {
            if (channels < 0 || channels > 1024 || !sample_size(w->sample_format) || w->dither < AFG_DITHER_OFF ||
                w->dither > AFG_DITHER_LCG31) {                                 // wav.d:400
                error = kErrorEncodingError;
            } else {
                // the header, lengths 0 until finalize (wav.d:407-469)
                uint8_t h[kWavHeader];
                const uint32_t ss = (uint32_t)sample_size(w->sample_format), frame_size = ss * (uint32_t)channels;
                std::memcpy(h, "RIFF\0\0\0\0WAVEfmt ", 16);
                put32(h + 16, 16);
                h[20] = w->sample_format <= AFG_WAV_S24LE ? 1 : 3; h[21] = 0;
                h[22] = (uint8_t)channels; h[23] = (uint8_t)(channels >> 8);
                put32(h + 24, (uint32_t)rate);
                put32(h + 28, (uint32_t)((uint64_t)(uint32_t)rate * frame_size));
                h[32] = (uint8_t)frame_size; h[33] = (uint8_t)(frame_size >> 8);
                h[34] = (uint8_t)(ss * 8); h[35] = 0;
                std::memcpy(h + 36, "data\0\0\0\0", 8);
                if (!w->append(h, kWavHeader)) error = kErrorEncodingError;
            }
        }
        if (!error && afg::require_device() != AFG_OK) error = kErrorEncodingError;
    } catch (...) {
        error = kErrorEncodingError;
    }
    afg_stream *s = afg_front::stream_for_writing(w, format, channels, samplerate, error);
    if (!s) delete w;
    return s;
}

// T = float or double
template <typename T> int write_any(afg_stream *s, const T *in, int frames)
{
    Writer *w = afg_front::stream_writer(s);
    if (!w || afg_is_error(s)) return 0;
    if (w->finalized) { afg_front::stream_set_error(s, kErrorEncodingError); return 0; }
    if (frames <= 0) return 0;
    if (!in) { afg_front::stream_set_error(s, kErrorEncodingError); return 0; }
    try {
        const size_t n = (size_t)frames * (size_t)w->channels;
        if (w->format == AFG_FORMAT_QOA) {
            if (sizeof(T) == sizeof(double) && !w->qoa_int) {
                // doubles are converted in double (qoa.d:632-634): what was queued as floats follows, by the same function
                // the kernel converts floats with (csrc/qoa_sample.h)
                w->qoa_i16.resize(w->qoa_f32.size());
                for (size_t i = 0; i < w->qoa_f32.size(); i++) w->qoa_i16[i] = afg_qoa_sample((double)w->qoa_f32[i]);
                std::vector<float>().swap(w->qoa_f32);
                w->qoa_int = true;
            }
            if (w->qoa_int) {
                const size_t at = w->qoa_i16.size();
                w->qoa_i16.resize(at + n);
                for (size_t i = 0; i < n; i++) w->qoa_i16[at + i] = afg_qoa_sample((double)in[i]);
            } else {
                w->qoa_f32.insert(w->qoa_f32.end(), (const float *)(const void *)in, (const float *)(const void *)in + n);
            }
            w->qoa_frames += (uint64_t)frames;
            return frames;
        }
        const size_t bytes = n * (size_t)sample_size(w->sample_format);
        if (!w->fits(w->pending_bytes()) || !w->fits(w->pending_bytes() + bytes)) {
            w->queue.clear();                                                   // nothing goes past the end
            afg_front::stream_set_error(s, kErrorEncodingError);
            return 0;
        }
        if (sizeof(T) == sizeof(double) && w->sample_format == AFG_WAV_FP64LE) {
            // wav.d:538-546: the doubles as they are, behind whatever floats are queued
            if (w->flush_wav() != AFG_OK) { afg_front::stream_set_error(s, kErrorEncodingError); return 0; }
            w->append((const uint8_t *)in, bytes);
            w->packed += n;
        } else {
            const size_t at = w->queue.size();
            w->queue.resize(at + n);
            for (size_t i = 0; i < n; i++) w->queue[at + i] = (float)in[i];    // stream.d:886-894 narrows doubles first
            if (w->queue.size() >= kFlushSamples && w->flush_wav() != AFG_OK) {
                afg_front::stream_set_error(s, kErrorEncodingError);
                return 0;
            }
        }
        w->written_frames += (uint64_t)frames;
        return frames;
    } catch (...) {
        afg_front::stream_set_error(s, kErrorEncodingError);
        return 0;
    }
}

}  // namespace
}  // namespace afg_write

extern "C" {

afg_stream *afg_open_to_buffer(int format, float samplerate, int channels, const afg_encoding_options *opts)
{
    return afg_write::open_any(false, nullptr, 0, format, samplerate, channels, opts);
}

afg_stream *afg_open_to_memory(uint8_t *data, size_t max_length, int format, float samplerate, int channels,
                               const afg_encoding_options *opts)
{
    return afg_write::open_any(true, data, max_length, format, samplerate, channels, opts);
}

int afg_write_samples_float(afg_stream *s, const float *in, int frames) { return afg_write::write_any<float>(s, in, frames); }
int afg_write_samples_double(afg_stream *s, const double *in, int frames) { return afg_write::write_any<double>(s, in, frames); }

int afg_finalize_encoding(afg_stream *s)
{
    afg_write::Writer *w = afg_front::stream_writer(s);
    if (!w || afg_is_error(s)) return 0;
    if (w->finalized) return 1;
    int rc = AFG_ERR_OOM;
    try {
        rc = w->format == AFG_FORMAT_QOA ? w->finalize_qoa() : w->finalize_wav();
    } catch (...) {
    }
    if (rc != AFG_OK) { afg_front::stream_set_error(s, afg_write::kErrorEncodingError); return 0; }
    w->finalized = true;
    return 1;
}

int afg_finalize_and_get_encoded(afg_stream *s, const uint8_t **bytes, size_t *length)
{
    if (bytes) *bytes = nullptr;
    if (length) *length = 0;
    afg_write::Writer *w = afg_front::stream_writer(s);
    if (!w || w->to_memory || !bytes || !length || !afg_finalize_encoding(s)) return 0;
    *bytes = w->buf.data();
    *length = w->buf.size();
    return 1;
}

}  // extern "C"
