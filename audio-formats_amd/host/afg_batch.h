// afg_batch.h -- the batch path's inside: what afg_batch.cpp (the passes over a batch), afg_stream.cpp (a stream's refill),
// afg_pools.cpp (staging buffers, helper threads) and the stages of the five codecs they drive (afg_flac_stage.cpp,
// afg_mp3_stage.cpp, afg_vorbis_stage.cpp, afg_opus_stage.cpp) share: each codec's staging pass over a batch and its device
// stage.  decode_parsed lays the five stages out in the order FLAC, QOA, MP3, Vorbis, Opus, runs them and fills the metadata.
#pragma once
#include "../csrc/afg_common.h"
#include "afg_flac_front.h"
#include "afg_mp3_front.h"
#include "afg_opus_front.h"
#include "afg_stage.h"
#include "afg_vorbis_front.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>

namespace afg_front {

// error strings of the reference (internals.d:16-23; stream.d:1379)
constexpr const char *kErrorUnknownFormat = "Cannot decode stream: unrecognized encoding.";
constexpr const char *kErrorDecodingError = "Decoder encountered an error";
constexpr const char *kErrorDecoderInitializationFailed = "Decoder initialization failed";
constexpr const char *kErrorNotInitialized = "Stream not initialized";
// this library's own: the reference decodes such files, the device path does not (out of scope)
constexpr const char *kErrorOpusMode = "Cannot decode stream: Opus SILK / hybrid packets are not supported (CELT-only).";

extern const bool g_trace;                       // AFG_TRACE was set when the library was loaded

// AFG_TRACE=1: wall-clock of the host stages on stderr (development aid)
struct StageTimer {
    bool on = g_trace;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[afg] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// A page-locked buffer on lease from the staging pool of afg_pools.cpp; it goes back when the lease ends.
struct StagingLease {
    void *p = nullptr;
    size_t cap = 0;
    StagingLease() = default;
    StagingLease(const StagingLease &) = delete;
    StagingLease &operator=(const StagingLease &) = delete;
    ~StagingLease();
};
int staging_take(size_t bytes, StagingLease &out);

// work() on the caller and on up to `helpers` pooled threads of the calling thread's helper pool (afg_pools.cpp)
void helpers_run(unsigned helpers, const std::function<void()> &work);
template <typename F>
void parallel_for(size_t n, unsigned threads, F fn)
{
    if (n == 0) return;
    threads = (unsigned)std::min<size_t>(std::max(1u, threads), n);
    std::atomic<size_t> next{ 0 };
    const std::function<void()> work = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) return;
            fn(i);
        }
    };
    helpers_run(threads - 1, work);
}
// host threads of a batch whose caller leaves the choice to the library, and of a stage that keeps every CPU busy by itself
unsigned default_threads();
unsigned sustained_threads();

// The helper pool and the stage chunk count of the calling host thread, for as long as the scope lives; the destructor puts
// back what it found.  kGroupLead / kGroup: the calling and the second host thread of a grouped batch, whose stages cut their
// files into 2 chunks, the second with the group pool of device `index`; kDevice: the thread of part `index` of a
// multi-device batch, with that part's pool.
struct HelperScope {
    enum Kind { kGroupLead, kGroup, kDevice };
    HelperScope(Kind kind, int index);
    HelperScope(const HelperScope &) = delete;
    HelperScope &operator=(const HelperScope &) = delete;
    ~HelperScope();
private:
    void *prev_pool;
    unsigned prev_chunks;
};
unsigned stage_chunks();                         // chunks a device stage of the calling thread cuts its files into

// ---------------------------------------------------------------------------------------------
// decoded files: one result plane for a whole batch
// ---------------------------------------------------------------------------------------------
struct Decoded {
    int status = AFG_OK;
    const char *message = nullptr;
    int format = AFG_FORMAT_UNKNOWN;
    int channels = 0;
    float samplerate = 0;
    int64_t frames = 0;                 // frames actually decoded
    int64_t declared_frames = AFG_UNKNOWN_LENGTH;
    size_t pcm_off = 0;                 // float offset of this file's interleaved PCM in the result plane
    bool in_mp3_plane = false;          // ... or in the batch's MP3 plane (staging layout, afg_batch_decode)
    bool in_opus_plane = false;         // ... or in the batch's Opus plane (decoded by the pipelined stage of afg_batch_decode)
};

struct Parsed {
    int format = AFG_FORMAT_UNKNOWN;
    FlacInfo fi;
    FlacRecords flac;
    QoaInfo qi;
    std::vector<afg_qoa_frame> qoa;
    afg_mp3::File mp3;
    afg_vorbis::File ogg;
    afg_opus::File opus;
    bool opus_mode = false;               // an Ogg Opus file with SILK / hybrid packets: reported, not decoded
    const float *mp3_coef() const { return mp3.ext_coef ? mp3.ext_coef : mp3.coef.data(); }
    const uint32_t *mp3_flags() const { return mp3.ext_flags ? mp3.ext_flags : mp3.flags.data(); }
};

struct BatchOut {
    std::vector<Decoded> files;
    StagingLease plane;                 // all PCM of the batch: FLAC files, then QOA files, then MP3 files; page-locked,
    size_t plane_floats = 0;            // returned to the pool by afg_batch_free / afg_close
    StagingLease mp3_plane;             // batch path: the MP3 PCM in staging layout, served in place
    StagingLease opus_plane;            // batch path: the Opus PCM, files back to back
    std::unique_ptr<BatchOut> early;    // batch path: the FLAC / QOA files, decoded on a second host thread meanwhile
    std::shared_ptr<void> mod_plane;    // batch path: the MOD files' PCM (afg_mod_stage.cpp)
    std::shared_ptr<void> wav_plane;    // batch path: the WAV files' PCM (afg_wav_stage.cpp)
    std::shared_ptr<void> xm_plane;     // batch path: the XM files' PCM (afg_xm_stage.cpp)
    bool f64 = false;                   // a stream's double reads: `plane` holds plane_floats doubles
};

// What every stage of one decode_parsed call works from.
// `own` (optional, one byte per file): the files this call is responsible for.  The batch path decodes its FLAC / QOA
// files on a second host thread while the first still parses MP3 / Ogg files: a call never looks at (not even the format
// of) a file it does not own.
struct StageCtx {
    std::vector<Parsed> &parsed;
    const uint8_t *const *data;
    const size_t *len;
    const uint8_t *own;
    unsigned threads;                   // host threads of a gather
    SampleOut so;
    unsigned chunks;                    // a stage cuts its files into about this many chunks
    BatchOut &out;
    StageTimer tm;
    size_t nf() const { return parsed.size(); }
    int fmt_of(size_t i) const { return (!own || own[i]) ? parsed[i].format : -1; }
    uint8_t *plane_at(size_t float_off) const { return (uint8_t *)out.plane.p + float_off * so.es(); }
};

// The device memory decode_parsed holds for its stages: FLAC and QOA restore into their ranges of d_out (the result plane's
// layout) and are converted in place of it into d_out64; the other stages keep planes of their own.  Every stage's
// conversions go through `conv`, which outlives the stages (SampleConv: until the streams have drained).
struct StageDev {
    DevBuf d_out, d_out64;
    SampleConv conv;
};

// ---- the staging passes of the batch path (afg_batch_decode): FLAC, MP3 and Ogg Vorbis files are parsed straight into one
// page-locked buffer per codec.  Pass 1 asks every file's bound (0: not this codec's file); prefix() gives file i its place
// base[i]; the codec's parse pass fills the lease and says whether every file is in it (otherwise the codec's files are
// gathered from their own buffers, wherever they sit). ----
struct StagingPlan {
    std::vector<size_t> bounds, base;
    size_t total = 0;
    StagingLease lease;
    explicit StagingPlan(size_t n_files) : bounds(n_files, 0), base(n_files, 0) {}
    void prefix(size_t align)                    // every file's share a multiple of `align` (a power of two)
    {
        for (size_t i = 0; i < bounds.size(); i++) { base[i] = total; total += (bounds[i] + align - 1) & ~(align - 1); }
    }
};

// FLAC files of declared length: file i's residual plane at word base[i] (16-byte aligned planes)
struct FlacStaging : StagingPlan {              // afg_flac_stage.cpp
    const int32_t *res = nullptr;               // set, with `words`, when every FLAC file of the batch is in the staging
    size_t words = 0;
    using StagingPlan::StagingPlan;
    size_t bound(size_t i, const uint8_t *d, size_t n) { return bounds[i] = flac_res_bound(d, n); }
    int parse(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm);
};

struct Mp3Staging;
// H2D -> kernel on stream `up`, D2H on stream `down` behind an event: chunk k+1 uploads and transforms while chunk
// k's PCM goes back (PCIe is full duplex) -- and while the host threads parse chunk k+2.
struct Mp3Pipe {                        // afg_mp3_stage.cpp
    const Mp3Staging *st = nullptr;
    DevBuf d_in, d_pcm, d_pcm64;
    SampleConv conv;
    uint32_t *d_flags = nullptr;
    std::vector<afg_mp3_plan *> plans;
    DevBuf d_tables;                    // plan tables: at most one 16-byte segment and stream record per block
    StagingLease h_tables;
    afg::PlanArena arena;
    int rc = AFG_OK;

    DevBuf d_qin;                       // quantised upload: int16 plane, record slots, stereo descriptors
    int16_t *d_q = nullptr;
    afg_mp3_qgranule *d_recs = nullptr;
    afg_mp3_sdesc *d_sdesc = nullptr;
    StagingLease h_sdesc;
    size_t sdesc_cap = 0, sdesc_used = 0;
    uint64_t h2d_bytes = 0;
    StageStreams s;                     // (behind the buffers and records: it drains first)

    int open(const Mp3Staging &stage);
    void submit(const std::vector<Parsed> &parsed, size_t f0, size_t f1);   // files [f0, f1) have been parsed into the stage: plan, upload, transform, download
    int close();
    ~Mp3Pipe() { (void)close(); }
};

// MP3 files: file i at block base[i] (gaps between files).
// The device planes and the MP3 result plane mirror that layout, so a chunk of files moves in ONE copy each way and
// a file's PCM is served where it lands (a per-file copy costs ~20 us of submission: 2 x 2048 of them were the whole
// end-to-end time of a 2048-file batch).  The files are parsed chunk by chunk, and a parsed chunk's device work is queued
// on `pipe` while the host threads go on with the next.
struct Mp3Staging : StagingPlan {               // afg_mp3_stage.cpp
    float *coef = nullptr;                      // float upload: dequantised spectra, blocks * 576 ...
    int16_t *q = nullptr;                       // ... or quantised upload: Huffman values, blocks * 576, and one record slot
    afg_mp3_qgranule *recs = nullptr;           // per block (the slot of a granule's first block is used, nch = 0 elsewhere)
    uint32_t *flags = nullptr;
    size_t blocks = 0;                          // `total` while the pipeline serves the files; 0: none, or the batch fell back
    float *plane = nullptr;                     // host PCM plane, blocks * 576 floats (page-locked) ...
    SampleOut so;                               // ... or as many doubles / packed integer samples (afg_batch_opts.sample_type): made of the transform's floats on the device
    bool fallback = false;                      // a file did not fit the staging: decode_parsed gathers the MP3 files
    Mp3Pipe pipe;                               // (behind the lease: it drains first)
    using StagingPlan::StagingPlan;
    size_t es() const { return so.es(); }
    size_t bound(size_t i, const uint8_t *d, size_t n) { return bounds[i] = afg_mp3::looks_like_mp3(d, n) ? afg_mp3::max_blocks(d, n) : 0; }
    int open(StagingLease &owner_plane, const SampleOut &out, StageTimer &tm);
    void parse_and_submit(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm);
    int close(StageTimer &tm);
};

// Ogg Vorbis files: file i's spectra at float base[i]
struct OggStaging : StagingPlan {               // afg_vorbis_stage.cpp
    const float *spec = nullptr;                // set, with `floats`, when every Vorbis file of the batch is in the staging
    size_t floats = 0;
    using StagingPlan::StagingPlan;
    size_t bound(size_t i, const uint8_t *d, size_t n) { return bounds[i] = afg_vorbis::max_spec_floats(d, n); }
    int parse(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm);
};

// FLAC: residual rows that fit 16 bits are packed as int16 (default) or left as int32 (AFG_FLAC_HOST_RES32=1)
bool flac_rows_int16();                         // afg_flac_stage.cpp
// Vorbis: inverse coupling and floor curves on the device (default) or in the host parser (AFG_VORBIS_HOST_FLOOR=1)
bool vorbis_floor_on_device();                  // afg_vorbis_stage.cpp

// ---- the five stages.  layout(ctx, plane_off): the stage's files get their pcm_off (the stage's PCM starts at float
// plane_off of the result plane), the stage its run list (with dither and in collate mode: afg_stage.h, PackRun) and its
// totals; returns the floats it needs in the result plane.  run(ctx, dev): the device work, into the stage's range of
// ctx.out.plane; it returns with its streams drained. ----
struct FlacDecode {                     // afg_flac_stage.cpp
    const FlacStaging *staged = nullptr;
    std::vector<size_t> res_base, fr_base, sf_base;
    size_t res_total = 0, fr_total = 0, sf_total = 0, out_floats = 0;
    std::vector<PackRun> runs;
    bool is_staged() const { return staged && staged->words; }
    size_t layout(StageCtx &ctx, size_t plane_off);
    int run(StageCtx &ctx, StageDev &dev);
};

struct QoaDecode {                      // afg_flac_stage.cpp
    std::vector<size_t> byte_base, fr_base;
    size_t bytes = 0, frames = 0, out_floats = 0, plane_off = 0;
    std::vector<PackRun> runs;
    size_t layout(StageCtx &ctx, size_t plane_off);
    int run(StageCtx &ctx, StageDev &dev);
};

// Decoder state an MP3 stream carries from one chunk of frames to the next (chunked AudioStream reads): the overlap and
// polyphase history of the run that was open when the previous chunk ended, as the transform kernel left it.  A stream
// that has moved to another device left it behind: `state` is of the old device then, and is dropped unread.
struct Mp3Carry {
    DevBuf state;                       // AFG_MP3_STATE_FLOATS floats
    bool valid = false;                 // `state` holds the end of the previous chunk
    bool continues = false;             // this chunk's first run goes on from it
};

// the runs of MP3 file `file` (its PCM plane starts at block `base` of the stage's): the pieces of its copy plan, in order
void mp3_runs(std::vector<PackRun> &runs, const afg_mp3::File &f, uint64_t base, size_t file);

struct Mp3Decode {                      // afg_mp3_stage.cpp
    const Mp3Staging *staged = nullptr;   // the files are already decoded, in staging layout, in staged->plane (Mp3Pipe)
    Mp3Carry *carry = nullptr;          // a stream's chunk
    std::vector<size_t> blk_base;
    size_t blocks = 0, plane_off = 0;
    std::vector<PackRun> runs;
    DevBuf d_pcm64;
    bool is_staged() const { return staged && staged->blocks && blocks; }
    size_t layout(StageCtx &ctx, size_t plane_off);
    void deliver_in_place(StageCtx &ctx);         // staged: the pieces of damaged files closed up, where they landed
    int run(StageCtx &ctx, StageDev &dev);        // not staged: the gathered stage
};

struct VorbisDecode {                   // afg_vorbis_stage.cpp
    const OggStaging *staged = nullptr;
    // chunks of files, one plan each; the Vorbis part of the result plane is the plans' output planes back to back, so a
    // chunk's PCM comes back in one copy and a file is served where it lands (first piece onwards)
    struct Chunk {
        size_t f0 = 0, f1 = 0, spec0 = 0, spec_n = 0, out0 = 0, out_n = 0;
        afg_vorbis_plan *plan = nullptr;
        std::vector<size_t> spec_at;                         // per file of the chunk: float offset of its spectra in the chunk
    };
    struct Piece { size_t file; uint64_t from, count; };     // pieces of files that are not served as one run
    std::vector<Chunk> chunks;
    std::vector<Piece> pieces;
    std::vector<size_t> broken;
    size_t out_floats = 0, packets = 0, spec = 0, plane_off = 0;
    std::vector<PackRun> runs;
    DevBuf d_pcm64;
    ~VorbisDecode();
    bool is_staged() const { return staged && staged->floats; }
    int layout(StageCtx &ctx, size_t plane_off, size_t *floats);   // (makes the plans: it can fail)
    int run(StageCtx &ctx, StageDev &dev);
private:
    int plan_chunk(StageCtx &ctx, Chunk &c, size_t plane_off);
};

// What an Opus stream carries from one chunk of packets to the next on the device: the transform stage's per-channel
// memory (overlap, post-filter history, de-emphasis), as afg_celt_transform_hip reads and rewrites it.  As with Mp3Carry,
// states of another device are dropped unread.
struct OpusCarry {
    DevBuf states;                      // channels * AFG_CELT_STATE_FLOATS floats
    bool valid = false;
};

struct OpusDecode {                     // afg_opus_stage.cpp: the gathered stage
    // batch path: the Opus files are already decoded (opus_pipeline), file i's PCM at float done_at[i] of the batch's Opus
    // plane; only their metadata is filled in
    const size_t *done_at = nullptr;
    OpusCarry *carry = nullptr;         // a stream's chunk
    std::vector<size_t> rec_base, coef_base, pcm_base;
    std::vector<uint64_t> seq_table;    // the first record of every channel sequence
    size_t out_floats = 0, recs = 0, coefs = 0, seqs = 0, plane_off = 0;
    std::vector<PackRun> runs;
    DevBuf d_pcm64;
    size_t layout(StageCtx &ctx, size_t plane_off);
    int run(StageCtx &ctx, StageDev &dev);
};

// Pass 1c of the batch path: every file with opened[i] -- its open scan left exact sizes in parsed[i].opus -- is decoded
// (range decoder + CELT frame decoder, by all helper threads) straight into one page-locked buffer, a chunk of files at a
// time; the chunk's upload, transform, output conversion and download are queued on two streams and run while the helpers
// decode the next chunk.  File i's PCM lands at float pcm_at[i] of `plane` (or, collate mode, in the tensor).
// *staged: the stage ran (there were Opus files).
int opus_pipeline(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *length, const std::vector<uint8_t> &opened,
                  unsigned threads, const SampleOut &so, StagingLease &plane, std::vector<size_t> &pcm_at, bool *staged, StageTimer &tm);


// ---- afg_batch.cpp ----
// a decode_parsed call's context, with the calling thread's chunk count
StageCtx stage_ctx(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, const uint8_t *own, unsigned threads,
                   SampleOut so, BatchOut &out);
// The device stages for a set of parsed files, each handed in with its optional inputs set; the results come back as one
// plane in ctx.out, laid out FLAC, QOA, MP3, Vorbis, Opus, and ctx.out.files tells where each file's PCM is.
int decode_parsed(StageCtx &ctx, FlacDecode &flac, Mp3Decode &mp3, VorbisDecode &ogg, OpusDecode &opus);

}  // namespace afg_front
