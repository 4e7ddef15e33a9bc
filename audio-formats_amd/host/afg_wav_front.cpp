// afg_wav_front.cpp -- WAVDecoder.scan (wav.d:53-217) statement for statement over a memory cursor, as a release build
// of the reference behaves: io.d's readers (:33-268) on stream.d's memory callbacks (:2084-2190).  The habits a cleaner
// parser would not have are kept and listed in INTEGRATION.md ("WAV"); so are the two rules of our own.
#include "afg_wav_front.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cstring>

namespace afg_wav {

const char *const kReasonSkip = "chunk size is negative as a 32-bit int (refused by this library)";
const char *const kReasonChannels = "'data' chunk of a format with 0 channels (refused by this library)";

namespace {

constexpr uint32_t riff_id(const char (&s)[5])
{
    return ((uint32_t)(uint8_t)s[0] << 24) | ((uint32_t)(uint8_t)s[1] << 16) | ((uint32_t)(uint8_t)s[2] << 8) | (uint32_t)(uint8_t)s[3];
}

const uint8_t kIeeeFloatGuid[16] = { 3, 0, 0, 0, 0, 0, 16, 0, 128, 0, 0, 170, 0, 56, 155, 113 };   // wav.d:43

// MemoryContext (stream.d:2084-2190): the cursor may stand behind the end after a skip
struct Cursor {
    const uint8_t *buf;
    size_t size, at = 0;

    int64_t remaining() const { return (int64_t)size - (int64_t)at; }      // io.d:38-44
    // memory_read: what is there is consumed even when it is not enough
    bool read(void *out, size_t n)
    {
        const size_t avail = at < size ? size - at : 0;
        if (n <= avail) { std::memcpy(out, buf + at, n); at += n; return true; }
        at = std::max(at, size);
        return false;
    }
    uint32_t u16(bool *err) { uint8_t v[2]; if (!read(v, 2)) { *err = true; return 0; } *err = false; return (uint32_t)v[0] | ((uint32_t)v[1] << 8); }
    uint32_t u32le(bool *err)
    {
        uint8_t v[4];
        if (!read(v, 4)) { *err = true; return 0; }
        *err = false;
        return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    }
    uint32_t u32be(bool *err)
    {
        uint8_t v[4];
        if (!read(v, 4)) { *err = true; return 0; }
        *err = false;
        return ((uint32_t)v[0] << 24) | ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | (uint32_t)v[3];
    }
    void chunk_header(uint32_t *id, uint32_t *bytes, bool *err)             // io.d:256-268
    {
        *id = u32be(err);
        if (*err) return;
        *bytes = u32le(err);
    }
    // skip(int) on memory_skip: the cursor moves whatever the size.  False: the amount is negative as an int, where the
    // reference would move backwards -- this library refuses the file instead.
    bool skip(uint32_t amount)
    {
        if ((int32_t)amount < 0) return false;
        at += amount;
        return true;
    }
};

}  // namespace

const char *scan(const uint8_t *data, size_t size, Info *out)
{
    Cursor io{ data, size };
    Info w;
    {
        uint32_t id = 0, bytes = 0;
        bool err = false;
        io.chunk_header(&id, &bytes, &err);
        if (err) return "Cannot read RIFF header";
        if (id != riff_id("RIFF")) return "Expected RIFF chunk.";
        if (bytes < 4) return "RIFF chunk is too small to contain a format.";
        if (io.u32be(&err) != riff_id("WAVE")) return "Expected WAVE format.";
    }
    bool found_fmt = false, found_data = false;
    int bits = 0;
    while (io.remaining() > 0) {
        // "Some corrupted WAV files in the wild finish with one extra 0 byte" (wav.d:81-91)
        if (io.remaining() == 1 && io.buf[io.at] == 0) break;
        uint32_t id = 0, bytes = 0;
        bool err = false;
        io.chunk_header(&id, &bytes, &err);
        if (err) return "Cannot read RIFF header";
        if (id == riff_id("fmt ")) {
            if (found_fmt) return "Found several 'fmt ' chunks in RIFF file.";
            found_fmt = true;
            if (bytes < 16) return "Expected at least 16 bytes in 'fmt ' chunk.";
            w.tag = (int)io.u16(&err);
            if (err) return "Cannot read WAV format";
            const bool wfe = w.tag == 0xFFFE;
            if (w.tag != 1 && w.tag != 3 && !wfe)
                return "Unsupported audio format, only PCM and IEEE float and WAVE_FORMAT_EXTENSIBLE are supported.";
            w.channels = (int)io.u16(&err);
            if (err) return "Cannot read number of channels";
            w.sample_rate = (int)io.u32le(&err);                             // (err is not looked at: wav.d:121)
            if (w.sample_rate <= 0) return "Unsupported sample-rate.";
            (void)io.u32le(&err);
            if (err) return "Cannot read bytesPerSec";
            const int bytes_per_frame = (int)io.u16(&err);
            if (err) return "Cannot read bytesPerFrame";
            bits = (int)io.u16(&err);
            if (err) return "Cannot read bitsPerSample";
            if (bits != 8 && bits != 16 && bits != 24 && bits != 32 && bits != 64) return "Unsupported bitdepth";
            if (bytes_per_frame != (bits / 8) * w.channels) return "Invalid bytes-per-second, data might be corrupted.";
            if (bytes >= 18) {
                const uint32_t cb = io.u16(&err);
                if (err) return "Cannot read cbSize";
                if (wfe) {
                    if (cb < 22) return "Unsupported WAVE_FORMAT_EXTENSIBLE.";
                    (void)io.u16(&err);
                    if (err) return "Cannot read wReserved";
                    (void)io.u32le(&err);
                    if (err) return "Cannot read dwChannelMask";
                    uint8_t guid[16];
                    if (!io.read(guid, 16)) return "Cannot read SubFormat";
                    if (std::memcmp(guid, kIeeeFloatGuid, 16) != 0) return "Unsupported GUID in WAVE_FORMAT_EXTENSIBLE.";
                    w.tag = 3;
                    if (!io.skip(bytes - 40u)) return kReasonSkip;
                } else if (!io.skip(bytes - 18u)) {
                    return kReasonSkip;
                }
            } else if (!io.skip(bytes - 16u)) {
                return kReasonSkip;
            }
        } else if (id == riff_id("data")) {
            if (found_data) return "Found several 'data' chunks in RIFF file.";
            if (!found_fmt) return "'fmt ' chunk expected before the 'data' chunk.";
            const uint32_t frame_size = (uint32_t)w.channels * (uint32_t)(bits / 8);
            if (frame_size == 0) return kReasonChannels;                     // the reference divides by it (wav.d:188)
            if (bytes % frame_size != 0) return "Remaining bytes in 'data' chunk, inconsistent with audio data type.";
            w.frames = bytes / frame_size;
            w.samples_off = io.at;
            if (!io.skip(bytes)) return kReasonSkip;
            found_data = true;
        } else if (!io.skip(bytes)) {                                        // "ignore unknown chunks"
            return kReasonSkip;
        }
    }
    if (!found_fmt) return "'fmt ' chunk not found.";
    if (!found_data) return "'data' chunk not found.";
    w.bits = bits;
    const uint64_t there = w.samples_off < size ? (uint64_t)size - w.samples_off : 0;
    w.present = std::min<uint64_t>(there / (uint64_t)(bits / 8), (uint64_t)w.frames * (uint64_t)w.channels);
    if (out) *out = w;
    return nullptr;
}

int kind_of(const Info &info)
{
    if (info.tag == 3) return info.bits == 32 ? AFG_WAV_KIND_F32 : info.bits == 64 ? AFG_WAV_KIND_F64 : -1;   // wav.d:260-286
    switch (info.bits) {                                                                                       // wav.d:288-337
    case 8: return AFG_WAV_KIND_U8;
    case 16: return AFG_WAV_KIND_S16;
    case 24: return AFG_WAV_KIND_S24;
    case 32: return AFG_WAV_KIND_S32;
    default: return -1;
    }
}

}  // namespace afg_wav

extern "C" int afg_wav_parse(const uint8_t *data, size_t length, afg_wav_parsed *out)
{
    if (!out || (!data && length)) {
        afg::set_error("afg_wav_parse: NULL argument");
        return AFG_ERR_INVALID;
    }
    std::memset(out, 0, sizeof(*out));
    afg_wav::Info w;
    if (const char *why = afg_wav::scan(data, length, &w)) {
        afg::set_error("afg_wav_parse: %s", why);
        return AFG_ERR_UNSUPPORTED;
    }
    out->tag = (uint32_t)w.tag;
    out->channels = (uint32_t)w.channels;
    out->bits = (uint32_t)w.bits;
    out->sample_rate = (uint32_t)w.sample_rate;
    out->frames = w.frames;
    out->kind = afg_wav::kind_of(w);
    out->samples_offset = w.samples_off;
    out->present_samples = w.present;
    return AFG_OK;
}
