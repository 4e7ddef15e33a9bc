// afg_encode_stage.cpp -- afg_batch_encode: interleaved float PCM in host memory to WAV or QOA files in host memory; and
// afg_batch_transcode: compressed files in host memory to WAV files in host memory (at the end of this file).
//
// Helper threads copy the PCM into leased page-locked staging (that copy puts every piece on a 4-float boundary),
// chunks go through two stagings and two pairs of device buffers with upload, kernel and download on the kept stream
// pair (afg_front::run_chunks), and the bytes come back into one page-locked plane that the items point into.  The plane
// has the device buffers' layout, so a chunk is one download: a WAV file starts 4 bytes past a 16-byte boundary, which
// puts its samples -- 44 bytes on -- on one; headers are written by the host once the last chunk is back.
// WAV: one afg_wav_pack_hip launch per chunk, whatever it holds; a long file is cut at tile boundaries and draw0 carries
// its dither position across the cuts.  QOA: afg_qoa_encode_hip over the streams of a chunk; the encoder's LMS state runs
// through a stream, so a file is never cut.
#include "afg_stage.h"
#include "afg_write_stream.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

namespace {

using afg_front::align16;
using afg_front::DevBuf;
using afg_write::kWavHeader;
using afg_write::sample_size;

const char *const kMessageChannels = "Encoder: unsupported channel count";
const char *const kMessageRate = "Encoder: sample rate out of range";
const char *const kMessageNoPcm = "Encoder: no samples given";
const char *const kMessageTooLong = "Encoder: too many frames for the format";

constexpr uint64_t kChunkSamples = (uint64_t)8 << 20;          // a chunk: 32 MB of floats up, 8-64 MB of file bytes down
static_assert(kChunkSamples % AFG_WAV_TILE_SAMPLES == 0, "files are cut at tile boundaries");

struct EncodeOwner {
    std::vector<afg_encoded_item> items;
    std::shared_ptr<void> plane;
};

struct File {
    bool ok = false;
    uint32_t rate = 0;
    uint64_t count = 0;        // samples
    uint64_t at = 0;           // first byte of the file in the plane
    uint64_t size = 0;
};

// a piece of one file inside a chunk: `src` is its first sample in the file's PCM, `in_off` / `count` its place in the staging
struct Piece { size_t file; uint64_t src, in_off, count; };

// The pipeline both formats share.  Chunk c owns pieces [first[c], first[c + 1]), uploads in_floats[c] floats, runs
// launch(c, d_in, d_out, stream) and brings out_bytes[c] bytes back to plane + plane_at[c].
template <typename Launch>
int run_pieces(const afg_encode_input *in, int n_threads, const std::vector<Piece> &pieces, const std::vector<size_t> &first,
               const std::vector<uint64_t> &in_floats, const std::vector<uint64_t> &out_bytes, const std::vector<uint64_t> &plane_at,
               uint8_t *plane, const Launch &launch)
{
    const size_t C = first.size() - 1;
    const int bufs = C > 1 ? 2 : 1;
    const uint64_t max_in = std::max<uint64_t>(4, *std::max_element(in_floats.begin(), in_floats.end()));
    const uint64_t max_out = std::max<uint64_t>(16, *std::max_element(out_bytes.begin(), out_bytes.end()));
    void *stage[2] = { nullptr, nullptr };
    std::shared_ptr<void> stage_owner[2];
    DevBuf d_in[2], d_out[2];
    for (int b = 0; b < bufs; b++) {
        if (!(stage_owner[b] = afg_front::staging_lease((size_t)max_in * sizeof(float), &stage[b]))) return AFG_ERR_OOM;
        if (int rc = d_in[b].alloc((size_t)max_in * sizeof(float))) return rc;
        if (int rc = d_out[b].alloc((size_t)align16(max_out))) return rc;
    }
    return afg_front::run_chunks(
        C, /* before */ nullptr,
        [&](size_t c, int b, hipStream_t up) -> int {
            const size_t p0 = first[c];
            float *hin = (float *)stage[b];
            afg_front::parallel_run(first[c + 1] - p0, n_threads, [&](size_t j) {
                const Piece &pc = pieces[p0 + j];
                if (pc.count) std::memcpy(hin + pc.in_off, in[pc.file].pcm + pc.src, (size_t)pc.count * sizeof(float));
            });
            if (in_floats[c]) AFG_HIP_CHECK(hipMemcpyAsync(d_in[b].p, hin, (size_t)in_floats[c] * sizeof(float), hipMemcpyHostToDevice, up));
            return AFG_OK;
        },
        [&](size_t c, int b, hipStream_t up) -> int { return launch(c, (const float *)d_in[b].p, (uint8_t *)d_out[b].p, up); },
        [&](size_t c, int b, hipStream_t down) -> int {
            if (out_bytes[c]) AFG_HIP_CHECK(hipMemcpyAsync(plane + plane_at[c], d_out[b].p, (size_t)out_bytes[c], hipMemcpyDeviceToHost, down));
            return AFG_OK;
        });
}

void wav_header(uint8_t *p, uint64_t frames, uint32_t channels, uint32_t rate, int format)
{
    // afg_wav.cpp's header, through the host writer itself: a file of no frames is the header alone, the two lengths follow
    (void)afg_wav_encode(nullptr, 0, channels, rate, format, p, kWavHeader);
    const uint64_t data_bytes = (uint64_t)((uint32_t)sample_size(format) * channels) * frames;
    const uint32_t riff = (uint32_t)(4 + (4 + 4 + 16) + (4 + 4 + data_bytes)), data = (uint32_t)data_bytes;
    std::memcpy(p + 4, &riff, 4);                       // (little-endian hosts only, like the rest of the library)
    std::memcpy(p + 40, &data, 4);
}

int encode_wav(const afg_encode_input *in, int n_threads, std::vector<File> &files, int sample_format, bool dither, uint32_t seed,
               EncodeOwner &owner)
{
    const uint64_t B = (uint64_t)sample_size(sample_format);
    std::vector<Piece> pieces;
    std::vector<afg_wav_pack_span> spans;                // chunk-relative offsets
    std::vector<size_t> first{ 0 };
    std::vector<uint64_t> in_floats, out_bytes, plane_at, tiles;
    uint64_t plane_bytes = 0, in_at = 0, chunk_samples = 0, chunk_at = 0, chunk_end = 0;
    auto close_chunk = [&] {
        if (first.back() == pieces.size()) return;
        first.push_back(pieces.size());
        in_floats.push_back(in_at);
        out_bytes.push_back(chunk_end - chunk_at);
        plane_at.push_back(chunk_at);
        in_at = 0; chunk_samples = 0;
    };
    for (size_t k = 0; k < files.size(); k++) {
        File &f = files[k];
        if (!f.ok) continue;
        const uint64_t data_at = align16(plane_bytes + kWavHeader);        // the samples start on a 16-byte boundary
        f.at = data_at - kWavHeader;
        f.size = kWavHeader + f.count * B;
        plane_bytes = data_at + f.count * B;
        for (uint64_t done = 0; done < f.count;) {
            if (kChunkSamples - chunk_samples < AFG_WAV_TILE_SAMPLES) close_chunk();
            const uint64_t room = (kChunkSamples - chunk_samples) & ~(uint64_t)(AFG_WAV_TILE_SAMPLES - 1);
            const uint64_t take = std::min(f.count - done, room);
            if (first.back() == pieces.size()) chunk_at = data_at + done * B;     // (done is a multiple of the tile: aligned)
            afg_wav_pack_span sp;
            std::memset(&sp, 0, sizeof(sp));
            sp.in_off = in_at;
            sp.out_off = data_at + done * B - chunk_at;
            sp.count = take;
            sp.draw0 = 2 * done;
            sp.seed = seed;
            sp.format = (uint8_t)sample_format;
            sp.dither = dither ? 1 : 0;
            spans.push_back(sp);
            pieces.push_back({ k, done, in_at, take });
            in_at += (take + 3) & ~(uint64_t)3;
            chunk_samples += take;
            chunk_end = data_at + (done + take) * B;
            done += take;
        }
    }
    close_chunk();
    void *plane = nullptr;
    owner.plane = afg_front::staging_lease((size_t)std::max<uint64_t>(plane_bytes, 16), &plane);
    if (!owner.plane) return AFG_ERR_OOM;
    if (!pieces.empty()) {
        const size_t C = first.size() - 1;
        tiles.resize(C);
        for (size_t c = 0; c < C; c++) tiles[c] = afg_wav_pack_layout(spans.data() + first[c], first[c + 1] - first[c]);
        DevBuf d_spans;
        if (int rc = d_spans.alloc(spans.size() * sizeof(afg_wav_pack_span))) return rc;
        // (synchronous: the table is in place before the pipeline's streams start)
        AFG_HIP_CHECK(hipMemcpy(d_spans.p, spans.data(), spans.size() * sizeof(afg_wav_pack_span), hipMemcpyHostToDevice));
        const int rc = run_pieces(in, n_threads, pieces, first, in_floats, out_bytes, plane_at, (uint8_t *)plane,
                                  [&](size_t c, const float *d_in, uint8_t *d_out, hipStream_t st) {
                                      return afg_wav_pack_hip(first[c + 1] - first[c], (const afg_wav_pack_span *)d_spans.p + first[c], tiles[c],
                                                              d_in, in_floats[c], d_out, align16(out_bytes[c]), st);
                                  });
        if (rc) return rc;
    }
    afg_front::parallel_run(files.size(), n_threads, [&](size_t k) {
        const File &f = files[k];
        if (!f.ok) return;
        wav_header((uint8_t *)plane + f.at, in[k].frames, in[k].channels, f.rate, sample_format);
        owner.items[k].bytes = (uint8_t *)plane + f.at;
        owner.items[k].size = f.size;
    });
    return AFG_OK;
}

int encode_qoa(const afg_encode_input *in, int n_threads, std::vector<File> &files, EncodeOwner &owner)
{
    std::vector<Piece> pieces;
    std::vector<afg_qoa_enc_stream> recs;                // chunk-relative offsets
    std::vector<size_t> first{ 0 };
    std::vector<uint64_t> in_floats, out_bytes, plane_at;
    uint64_t plane_bytes = 0, in_at = 0, chunk_at = 0;
    auto close_chunk = [&] {
        if (first.back() == pieces.size()) return;
        first.push_back(pieces.size());
        in_floats.push_back(in_at);
        out_bytes.push_back(plane_bytes - chunk_at);
        plane_at.push_back(chunk_at);
        in_at = 0;
    };
    for (size_t k = 0; k < files.size(); k++) {
        File &f = files[k];
        if (!f.ok) continue;
        if (in_at && in_at + f.count > kChunkSamples) close_chunk();
        plane_bytes = (plane_bytes + 7) & ~(uint64_t)7;
        if (first.back() == pieces.size()) chunk_at = plane_bytes;
        f.at = plane_bytes;
        f.size = afg_qoa_encoded_size((uint32_t)in[k].frames, in[k].channels);
        afg_qoa_enc_stream r;
        std::memset(&r, 0, sizeof(r));
        r.pcm_off = in_at;
        r.out_off = f.at - chunk_at;
        r.samples = (uint32_t)in[k].frames;
        r.samplerate = f.rate;
        r.channels = (uint8_t)in[k].channels;
        recs.push_back(r);
        pieces.push_back({ k, 0, in_at, f.count });
        in_at += (f.count + 3) & ~(uint64_t)3;
        plane_bytes += f.size;
    }
    close_chunk();
    void *plane = nullptr;
    owner.plane = afg_front::staging_lease((size_t)std::max<uint64_t>(plane_bytes, 16), &plane);
    if (!owner.plane) return AFG_ERR_OOM;
    if (!pieces.empty()) {
        DevBuf d_recs;
        if (int rc = d_recs.alloc(recs.size() * sizeof(afg_qoa_enc_stream))) return rc;
        AFG_HIP_CHECK(hipMemcpy(d_recs.p, recs.data(), recs.size() * sizeof(afg_qoa_enc_stream), hipMemcpyHostToDevice));
        const int rc = run_pieces(in, n_threads, pieces, first, in_floats, out_bytes, plane_at, (uint8_t *)plane,
                                  [&](size_t c, const float *d_in, uint8_t *d_out, hipStream_t st) {
                                      return afg_qoa_encode_hip((uint32_t)(first[c + 1] - first[c]), (const afg_qoa_enc_stream *)d_recs.p + first[c],
                                                                nullptr, d_in, d_out, st);
                                  });
        if (rc) return rc;
    }
    for (size_t k = 0; k < files.size(); k++) {
        if (!files[k].ok) continue;
        owner.items[k].bytes = (uint8_t *)plane + files[k].at;
        owner.items[k].size = files[k].size;
    }
    return AFG_OK;
}

}  // namespace

extern "C" {

int afg_batch_encode(const afg_encode_input *in, int n_files, int format, const afg_encoding_options *opts, int n_threads,
                     afg_encode_result *out)
{
    if (out) { out->n_files = 0; out->items = nullptr; out->owner = nullptr; }
    if (!out || n_files < 0 || (n_files > 0 && !in) || n_threads < 0) {
        afg::set_error("afg_batch_encode: bad arguments");
        return AFG_ERR_INVALID;
    }
    if (opts && opts->struct_size != sizeof(afg_encoding_options)) {
        afg::set_error("afg_batch_encode: afg_encoding_options.struct_size does not match this library");
        return AFG_ERR_INVALID;
    }
    if (format != AFG_FORMAT_WAV && format != AFG_FORMAT_QOA) {
        afg::set_error("afg_batch_encode: only WAV and QOA are written");
        return AFG_ERR_UNSUPPORTED;
    }
    const int sample_format = opts ? opts->sample_format : AFG_WAV_FP32LE;
    const int dither = opts ? opts->dither : AFG_DITHER_LIBC;
    const bool wav = format == AFG_FORMAT_WAV, integer = sample_format <= AFG_WAV_S24LE;
    if (wav && (sample_format < AFG_WAV_S8 || sample_format > AFG_WAV_FP64LE || dither < AFG_DITHER_OFF || dither > AFG_DITHER_LCG31)) {
        afg::set_error("afg_batch_encode: unknown sample format or dither");
        return AFG_ERR_INVALID;
    }
    if (wav && integer && dither == AFG_DITHER_LIBC) {
        afg::set_error("afg_batch_encode: libc rand() dither has no defined draw order across files; use AFG_DITHER_LCG31 or AFG_DITHER_OFF");
        return AFG_ERR_UNSUPPORTED;
    }
    if (int rc = afg::require_device()) return rc;
    try {
        std::unique_ptr<EncodeOwner> owner(new EncodeOwner);
        owner->items.resize((size_t)n_files);
        std::vector<File> files((size_t)n_files);
        for (int i = 0; i < n_files; i++) {
            afg_encoded_item &it = owner->items[(size_t)i];
            File &f = files[(size_t)i];
            it.status = AFG_ERR_INVALID;
            it.bytes = nullptr;
            it.size = 0;
            const float biased = in[i].samplerate + 0.5f;                      // stream.d:1852
            const bool rate_ok = wav ? (biased >= 0.0f && biased < 2147483648.0f) : (biased >= 1.0f && biased < 16777216.0f);
            const uint64_t max_frames = ~(uint64_t)0 / 8 / std::max<uint32_t>(1, in[i].channels);
            if (in[i].channels == 0 || in[i].channels > (wav ? 1024u : 8u)) it.message = kMessageChannels;
            else if (!rate_ok) it.message = kMessageRate;
            else if (!in[i].pcm && in[i].frames) it.message = kMessageNoPcm;
            else if (in[i].frames > (wav ? max_frames : (uint64_t)0xffffffffu)) it.message = kMessageTooLong;
            else {
                it.status = AFG_OK;
                it.message = nullptr;
                f.ok = true;
                f.rate = (uint32_t)(int)biased;
                f.count = in[i].frames * in[i].channels;
            }
        }
        const int rc = wav ? encode_wav(in, n_threads, files, sample_format, integer && dither == AFG_DITHER_LCG31, opts ? opts->dither_seed : 0, *owner)
                           : encode_qoa(in, n_threads, files, *owner);
        if (rc) return rc;
        out->n_files = n_files;
        out->items = owner->items.data();
        out->owner = owner.release();
        return AFG_OK;
    } catch (const std::bad_alloc &) {
        afg::set_error("afg_batch_encode: out of memory");
        return AFG_ERR_OOM;
    }
}

// Decode with the sample type the WAV format asks for -- the body of every file is made on the device and comes down at
// its own width -- then one host copy per file on the pooled threads puts header and body side by side in the result's
// plane.  (The other way, reserving 44 bytes in front of every file inside the decode stages' planes, would have every
// stage lay its plane out for this one caller.)
int afg_batch_transcode(const uint8_t *const *data, const size_t *length, int n_files, int out_format, const afg_encoding_options *enc,
                        const afg_batch_opts *opts, afg_encode_result *out)
{
    if (out) { out->n_files = 0; out->items = nullptr; out->owner = nullptr; }
    if (!out || n_files < 0 || (n_files > 0 && (!data || !length))) {
        afg::set_error("afg_batch_transcode: bad arguments");
        return AFG_ERR_INVALID;
    }
    if (enc && enc->struct_size != sizeof(afg_encoding_options)) {
        afg::set_error("afg_batch_transcode: afg_encoding_options.struct_size does not match this library");
        return AFG_ERR_INVALID;
    }
    if (opts && opts->struct_size < offsetof(afg_batch_opts, sample_type)) {
        afg::set_error("afg_batch_transcode: afg_batch_opts.struct_size too small");
        return AFG_ERR_INVALID;
    }
    if (out_format == AFG_FORMAT_QOA) {
        afg::set_error("afg_batch_transcode: QOA output is not provided: the encoder's state runs through a whole file and the decode stages cut files at chunk borders; decode, then afg_batch_encode");
        return AFG_ERR_UNSUPPORTED;
    }
    if (out_format != AFG_FORMAT_WAV) {
        afg::set_error("afg_batch_transcode: only WAV is written");
        return AFG_ERR_UNSUPPORTED;
    }
    const int sample_format = enc ? enc->sample_format : AFG_WAV_FP32LE;
    const int dither = enc ? enc->dither : AFG_DITHER_OFF;
    if (sample_format < AFG_WAV_S8 || sample_format > AFG_WAV_FP64LE) {
        afg::set_error("afg_batch_transcode: unknown sample_format %d", sample_format);
        return AFG_ERR_INVALID;
    }
    if (dither < AFG_DITHER_OFF || dither > AFG_DITHER_LCG31) {
        afg::set_error("afg_batch_transcode: unknown dither %d", dither);
        return AFG_ERR_INVALID;
    }
    const bool integer = sample_format <= AFG_WAV_S24LE;
    if (integer && dither == AFG_DITHER_LIBC) {
        afg::set_error("afg_batch_transcode: dither: libc rand() has no defined draw order across files; use AFG_DITHER_LCG31 or AFG_DITHER_OFF");
        return AFG_ERR_INVALID;
    }
    try {
        afg_batch_opts o;
        std::memset(&o, 0, sizeof(o));
        o.struct_size = sizeof(o);
        if (opts) { o.n_threads = opts->n_threads; o.n_devices = opts->n_devices; o.devices = opts->devices; }
        o.sample_type = integer ? (uint32_t)(AFG_SAMPLE_PCM_S8 + (sample_format - AFG_WAV_S8)) : sample_format == AFG_WAV_FP64LE ? AFG_SAMPLE_F64 : AFG_SAMPLE_F32;
        o.dither = integer ? dither : AFG_DITHER_OFF;           // (the float formats never dither)
        o.dither_seed = enc ? enc->dither_seed : 0;
        afg_batch_result dec;
        if (int rc = afg_batch_decode_ex(data, length, n_files, &o, &dec)) return rc;
        struct FreeDecoded { afg_batch_result *r; ~FreeDecoded() { afg_batch_free(r); } } free_decoded{ &dec };
        std::unique_ptr<EncodeOwner> owner(new EncodeOwner);
        owner->items.resize((size_t)n_files);
        const uint64_t B = (uint64_t)sample_size(sample_format);
        std::vector<File> files((size_t)n_files);
        uint64_t plane_bytes = 0;
        for (int i = 0; i < n_files; i++) {
            const afg_batch_item &d = dec.items[i];
            afg_encoded_item &it = owner->items[(size_t)i];
            File &f = files[(size_t)i];
            it.status = d.status;
            it.message = d.message;
            it.bytes = nullptr;
            it.size = 0;
            if (d.status != AFG_OK) continue;
            const float biased = d.samplerate + 0.5f;                          // stream.d:1852
            if (d.channels < 1 || d.channels > 1024) { it.status = AFG_ERR_INVALID; it.message = kMessageChannels; continue; }
            if (!(biased >= 0.0f && biased < 2147483648.0f)) { it.status = AFG_ERR_INVALID; it.message = kMessageRate; continue; }
            f.ok = true;
            f.rate = (uint32_t)(int)biased;
            f.count = (uint64_t)std::max<int64_t>(d.frames, 0) * (uint64_t)d.channels;
            f.at = plane_bytes;
            f.size = kWavHeader + f.count * B;
            plane_bytes = align16(plane_bytes + f.size);
        }
        // (pageable: nothing is copied from the device into this plane, and pinning costs about as much as a copy)
        uint8_t *plane = (uint8_t *)std::malloc((size_t)std::max<uint64_t>(plane_bytes, 16));
        if (!plane) throw std::bad_alloc();
        owner->plane = std::shared_ptr<void>(plane, [](void *q) { std::free(q); });
        afg_front::parallel_run((size_t)n_files, o.n_threads, [&](size_t k) {
            const File &f = files[k];
            if (!f.ok) return;
            const afg_batch_item &d = dec.items[k];
            uint8_t *p = plane + f.at;
            wav_header(p, (uint64_t)std::max<int64_t>(d.frames, 0), (uint32_t)d.channels, f.rate, sample_format);
            if (f.count) std::memcpy(p + kWavHeader, d.pcm, (size_t)(f.count * B));
            owner->items[k].bytes = p;
            owner->items[k].size = f.size;
        });
        out->n_files = n_files;
        out->items = owner->items.data();
        out->owner = owner.release();
        return AFG_OK;
    } catch (const std::bad_alloc &) {
        afg::set_error("afg_batch_transcode: out of memory");
        return AFG_ERR_OOM;
    }
}

void afg_encode_free(afg_encode_result *r)
{
    if (!r) return;
    delete (EncodeOwner *)r->owner;
    r->n_files = 0;
    r->items = nullptr;
    r->owner = nullptr;
}

}  // extern "C"
