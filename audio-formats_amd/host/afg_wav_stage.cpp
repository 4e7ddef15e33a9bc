// afg_wav_stage.cpp -- the device side of WAV decoding: a stream's reads and the batch path's WAV stage.
//
// Both hand csrc/wav_pcm.hip the sample bytes as they are in the file -- 1 to 8 bytes per sample, nothing converted on the
// host -- and bring float32 back.  End to end this is bound by the bus (1-8 bytes up, 4 down per sample), not by the
// kernel; it runs on the device because the library has no CPU path, and so that a WAV in a batch rides the same upload /
// kernel / download pipeline as its neighbours.
#include "afg_wav_front.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <atomic>
#include <cstring>

namespace afg_wav {

using afg_front::align16;

const char *const kMessageDecodingError = "Decoder encountered an error";

namespace {
constexpr uint64_t kStreamChunkSamples = (uint64_t)1 << 18;               // a stream's FIFO refill: 1 MB of floats
constexpr uint64_t kBatchChunkSamples = (uint64_t)8 << 20;                // a batch chunk: 32 MB of floats, 8-64 MB of input
static_assert(kBatchChunkSamples % AFG_WAV_TILE_SAMPLES == 0, "files are cut at tile boundaries");
}  // namespace

bool StreamConv::seek(int frame)
{
    if (frame < 0 || (uint32_t)frame > info.frames) return false;
    position_ = (uint32_t)frame;
    return true;
}

// frames [frame0, frame0 + frames) of the file into the FIFO; all of their samples are in the file
int StreamConv::decode(const uint8_t *file, uint64_t frame0, uint64_t frames)
{
    const uint64_t C = (uint64_t)info.channels, B = (uint64_t)bytes_per_sample(info);
    const uint64_t count = frames * C, bytes = count * B;
    hipStream_t st = nullptr;                                             // (after a change of device the buffers follow by themselves)
    if (int rc = stream_.current(&st)) return rc;
    afg_wav_span span;
    std::memset(&span, 0, sizeof(span));
    span.count = count;
    span.kind = (uint32_t)kind_of(info);
    const uint64_t tiles = afg_wav_layout(&span, 1);
    const size_t in_bytes = align16(bytes), out_samples = (size_t)((count + 3) & ~(uint64_t)3);
    if (in_.alloc(in_bytes) || out_.alloc(out_samples * es_) || spans_.alloc(sizeof(span))) return AFG_ERR_OOM;
    fifo_.resize((size_t)count * es_);
    fifo_frame_ = frame0;
    AFG_HIP_CHECK(hipMemcpyAsync(spans_.p, &span, sizeof(span), hipMemcpyHostToDevice, st));
    AFG_HIP_CHECK(hipMemcpyAsync(in_.p, file + info.samples_off + frame0 * C * B, bytes, hipMemcpyHostToDevice, st));
    const int rc = es_ == sizeof(double)
                       ? afg_pcm_to_f64_hip(1, (const afg_wav_span *)spans_.p, tiles, (const uint8_t *)in_.p, in_bytes, (double *)out_.p, out_samples, st)
                       : afg_wav_convert_hip(1, (const afg_wav_span *)spans_.p, tiles, (const uint8_t *)in_.p, in_bytes, (float *)out_.p, out_samples, st);
    if (rc) {
        fifo_.clear();
        return rc;
    }
    hipError_t e = hipMemcpyAsync(fifo_.data(), out_.p, count * es_, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        fifo_.clear();
        afg::set_error("WAV stream: %s", hipGetErrorString(e));
        return AFG_ERR_HIP;
    }
    return AFG_OK;
}

int StreamConv::read(const uint8_t *file, size_t size, void *out, int frames, bool *failed, bool f64)
{
    (void)size;
    *failed = false;
    if (es_ != (f64 ? sizeof(double) : sizeof(float))) {                  // a change of type: what is held is of the other one
        fifo_.clear();
        es_ = f64 ? sizeof(double) : sizeof(float);
    }
    if (frames <= 0) return 0;
    // wav.d:247-255: the request is clamped to what the header declares and the position moves before anything is read
    const uint32_t n = std::min<uint32_t>((uint32_t)frames, info.frames - position_);
    const uint64_t first = position_, C = (uint64_t)info.channels;
    position_ += n;
    if (kind_of(info) < 0) { *failed = true; return 0; }                  // wav.d:282-286, :332-337
    if (n == 0) return 0;
    // the reference reads sample by sample and gives the whole read up at the first one that is not there
    if ((first + n) * C > info.present) { *failed = true; return 0; }
    const uint64_t chunk = std::max<uint64_t>(1, kStreamChunkSamples / C), valid_end = std::min<uint64_t>(info.frames, info.present / C);
    uint64_t f = first, done = 0;
    while (done < n) {
        uint64_t held = fifo_.size() / (es_ * C);
        if (f < fifo_frame_ || f >= fifo_frame_ + held) {
            if (decode(file, f, std::min(valid_end - f, chunk)) != AFG_OK) return -1;
            held = fifo_.size() / (es_ * C);
        }
        const uint64_t take = std::min<uint64_t>(n - done, fifo_frame_ + held - f);
        if (out) std::memcpy((uint8_t *)out + done * C * es_, fifo_.data() + (f - fifo_frame_) * C * es_, (size_t)(take * C) * es_);
        f += take;
        done += take;
    }
    return (int)n;
}

int batch_stage(const uint8_t *const *data, const size_t *length, const std::vector<int> &which,
                int n_threads, afg_batch_item *items, std::shared_ptr<void> &keep, afg_front::SampleOut so)
{
    if (which.empty()) return AFG_OK;
    const bool f64 = so.f64();
    const size_t es = so.es();                                    // bytes per sample of the PCM plane (span offsets count samples)
    // (tests make small files span several chunks: afg_dev_option("stage_chunk_samples"))
    const uint64_t chunk_cap = (afg_front::stage_chunk_samples(kBatchChunkSamples) + AFG_WAV_TILE_SAMPLES - 1) & ~(uint64_t)(AFG_WAV_TILE_SAMPLES - 1);
    std::vector<afg_front::PackRun> runs;                         // AFG_SAMPLE_PCM_* with dither, collate: a file is one run of its own samples
    // ---- the scan, one file per helper-thread job ----
    struct File { bool ok = false; Info info; int kind = -1; uint64_t out_off = 0; };
    std::vector<File> files(which.size());
    afg_front::parallel_run(which.size(), n_threads, [&](size_t k) {
        const int i = which[k];
        File &f = files[k];
        if (!data[i] || scan(data[i], length[i], &f.info) != nullptr) return;
        f.ok = true;
        f.kind = kind_of(f.info);
    });
    // ---- layout: a file's floats start on a 16-byte boundary of the PCM plane; files are cut into pieces at tile
    //      boundaries where a chunk is full, so that a file of any length goes through buffers of one chunk ----
    struct Piece { size_t file; uint64_t src_byte; };
    std::vector<Piece> pieces;
    std::vector<afg_wav_span> spans;                     // chunk-relative offsets
    std::vector<size_t> first{ 0 };                      // chunk c owns pieces [first[c], first[c + 1])
    std::vector<uint64_t> chunk_out0{ 0 };               // its first float in the PCM plane
    uint64_t plane_floats = 0, in_at = 0, chunk_samples = 0, max_in = 16, max_out = 4;
    bool any = false;
    auto close_chunk = [&] {
        if (first.back() == pieces.size()) return;
        first.push_back(pieces.size());
        chunk_out0.push_back(0);
        in_at = 0; chunk_samples = 0;
    };
    for (size_t k = 0; k < files.size(); k++) {
        File &f = files[k];
        if (!f.ok) continue;
        afg_batch_item &it = items[which[k]];
        it.format = AFG_FORMAT_WAV;
        it.channels = f.info.channels;
        it.samplerate = (float)f.info.sample_rate;
        it.frames = 0;
        it.pcm = nullptr;
        const uint64_t count = (uint64_t)f.info.frames * (uint64_t)f.info.channels, B = (uint64_t)bytes_per_sample(f.info);
        if (f.kind < 0 || f.info.present != count) {     // one read of the whole declared length fails (stream.d:563-567)
            it.status = AFG_ERR_INVALID;
            it.message = kMessageDecodingError;
            f.ok = false;
            continue;
        }
        it.status = AFG_OK;
        it.message = nullptr;
        any = true;
        plane_floats = (plane_floats + 3) & ~(uint64_t)3;
        f.out_off = plane_floats;
        if (so.runs()) runs.push_back(afg_front::PackRun{ f.out_off, count, 0, (uint32_t)which[k], (uint32_t)f.info.channels });
        for (uint64_t done = 0; done < count;) {
            if (chunk_cap - chunk_samples < AFG_WAV_TILE_SAMPLES) close_chunk();
            const uint64_t room = (chunk_cap - chunk_samples) & ~(uint64_t)(AFG_WAV_TILE_SAMPLES - 1);
            const uint64_t take = std::min(count - done, room);
            if (first.back() == pieces.size()) chunk_out0.back() = f.out_off + done;
            afg_wav_span sp;
            std::memset(&sp, 0, sizeof(sp));
            sp.in_off = in_at;
            sp.out_off = f.out_off + done - chunk_out0.back();
            sp.count = take;
            sp.kind = (uint32_t)f.kind;
            spans.push_back(sp);
            pieces.push_back({ k, f.info.samples_off + done * B });
            in_at += align16(take * B);
            chunk_samples += take;
            done += take;
            max_in = std::max(max_in, in_at);
            max_out = std::max(max_out, (sp.out_off + take + 3) & ~(uint64_t)3);
        }
        plane_floats += count;
    }
    if (!any) return AFG_OK;
    close_chunk();
    const size_t C = first.size() - 1;
    std::vector<uint64_t> tiles(C, 0);
    for (size_t c = 0; c < C; c++) tiles[c] = afg_wav_layout(spans.data() + first[c], first[c + 1] - first[c]);

    // page-locked: the PCM plane the items point into (owned by `keep`) and two input stagings that take turns
    void *pcm = nullptr, *stage[2] = { nullptr, nullptr };
    std::shared_ptr<void> pcm_owner;                     // (collate: the floats go on to the tensor, nothing comes back)
    if (so.fetch() && !(pcm_owner = afg_front::staging_lease(std::max<uint64_t>(plane_floats, 4) * es, &pcm))) return AFG_ERR_OOM;
    std::shared_ptr<void> stage_owner[2];
    for (int b = 0; b < (C > 1 ? 2 : 1); b++)
        if (!(stage_owner[b] = afg_front::staging_lease((size_t)max_in, &stage[b]))) return AFG_ERR_OOM;
    afg_front::DevBuf d_spans, d_in[2], d_out[2];
    if (int rc = d_spans.alloc(std::max<size_t>(spans.size(), 1) * sizeof(afg_wav_span))) return rc;
    for (int b = 0; b < (C > 1 ? 2 : 1); b++) {
        if (int rc = d_in[b].alloc((size_t)max_in)) return rc;
        if (int rc = d_out[b].alloc((size_t)max_out * (so.pcm() ? sizeof(float) : es))) return rc;
    }
    afg_front::WideSlots packed;                         // AFG_SAMPLE_PCM_*, collate: the converted floats stay on the device and are packed or scattered there
    if (so.pcm()) if (int rc = packed.alloc((size_t)max_out, es)) return rc;
    // what chunk c takes up and brings back: both end with its last piece
    auto in_bytes = [&](size_t c) {
        const size_t p = first[c + 1] - 1;
        return spans[p].in_off + align16(spans[p].count * (uint64_t)bytes_per_sample(files[pieces[p].file].info));
    };
    auto out_floats = [&](size_t c) { return spans[first[c + 1] - 1].out_off + spans[first[c + 1] - 1].count; };
    const int rc = afg_front::run_chunks(
        C,
        [&](hipStream_t up) -> int {
            AFG_HIP_CHECK(hipMemcpyAsync(d_spans.p, spans.data(), spans.size() * sizeof(afg_wav_span), hipMemcpyHostToDevice, up));
            return AFG_OK;
        },
        [&](size_t c, int b, hipStream_t up) -> int {
            const size_t p0 = first[c];
            uint8_t *hin = (uint8_t *)stage[b];
            afg_front::parallel_run(first[c + 1] - p0, n_threads, [&](size_t j) {
                const Piece &pc = pieces[p0 + j];
                const afg_wav_span &sp = spans[p0 + j];
                std::memcpy(hin + sp.in_off, data[which[pc.file]] + pc.src_byte,
                            (size_t)(sp.count * (uint64_t)bytes_per_sample(files[pc.file].info)));
            });
            AFG_HIP_CHECK(hipMemcpyAsync(d_in[b].p, hin, (size_t)in_bytes(c), hipMemcpyHostToDevice, up));
            return AFG_OK;
        },
        [&](size_t c, int b, hipStream_t up) -> int {
            if (f64)
                return afg_pcm_to_f64_hip(first[c + 1] - first[c], (const afg_wav_span *)d_spans.p + first[c], tiles[c], (const uint8_t *)d_in[b].p,
                                          in_bytes(c), (double *)d_out[b].p, (out_floats(c) + 3) & ~(uint64_t)3, up);
            if (int rc = afg_wav_convert_hip(first[c + 1] - first[c], (const afg_wav_span *)d_spans.p + first[c], tiles[c], (const uint8_t *)d_in[b].p,
                                             in_bytes(c), (float *)d_out[b].p, (out_floats(c) + 3) & ~(uint64_t)3, up))
                return rc;
            // (without dither the alignment gaps between files are packed too: their floats are whatever the buffer held)
            // (f64 was converted from the file's own sample type above: no launch follows)
            return packed.launch(b, so, AFG_WAV_KIND_F32, d_out[b].p, chunk_out0[c], out_floats(c), runs, up);
        },
        [&](size_t c, int b, hipStream_t down) -> int {
            if (!so.fetch()) return AFG_OK;
            AFG_HIP_CHECK(hipMemcpyAsync((uint8_t *)pcm + chunk_out0[c] * es, so.pcm() ? packed.buf[b].p : d_out[b].p, (size_t)out_floats(c) * es, hipMemcpyDeviceToHost, down));
            return AFG_OK;
        });
    if (rc) return rc;
    for (size_t k = 0; k < files.size(); k++) {
        const File &f = files[k];
        if (!f.ok) continue;
        afg_batch_item &it = items[which[k]];
        it.frames = (int64_t)f.info.frames;
        it.pcm = f.info.frames && pcm ? (float *)((uint8_t *)pcm + f.out_off * es) : nullptr;
    }
    keep = pcm_owner;
    return AFG_OK;
}

}  // namespace afg_wav
