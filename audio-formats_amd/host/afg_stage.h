// afg_stage.h -- the toolkit every host stage shares (the FLAC / QOA, MP3, Vorbis and Opus stages of afg_*_stage.cpp behind
// afg_batch.h; MOD, XM and WAV decoding, the batch encoder, the write stream): the library's pools, the one pooled device
// buffer, a handle's own stream, the conversion that follows a stage's kernels (SampleConv), the stream holder and chunk
// cutter of the pipelined stages, the two-slot chunk pipeline (run_chunks), and what the tensor entries behind
// afg_batch_decode_resampled open and close with (tensor_entry .. resample_opts_of).
#pragma once
#include "../csrc/afg_records.h"

#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

namespace afg_front {

// ---- the pools and helper threads of afg_pools.cpp ----
int devpool_take(size_t bytes, void **out, size_t *cap_out);   // device memory, kept between calls
void devpool_give(void *p, size_t cap, int dev);               // dev: the device it was taken on
bool poison_alloc();                                           // AFG_POISON_ALLOC was set when the library was loaded (tests)
// a page-locked staging lease (pinning memory costs about as much as moving it); the buffer goes back to the pool when
// the last owner lets go.  NULL: out of memory.
std::shared_ptr<void> staging_lease(size_t bytes, void **p);
// the kept upload / download pair of the current device; mid (optional): a third stream for the kernels of a stage whose
// uploads should never wait behind them
hipError_t streams_take(hipStream_t *up, hipStream_t *down, hipStream_t *mid = nullptr);
void streams_give(hipStream_t up, hipStream_t down, hipStream_t mid = nullptr);   // ... given back drained
// fn(0) .. fn(n - 1) on the library's pooled host threads; n_threads 0 = the library's choice (afg_batch_decode)
void parallel_run(size_t n, int n_threads, const std::function<void(size_t)> &fn);

constexpr uint64_t align16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// Device memory from the pool, returned to the device it was taken on: the library's one device-buffer type.
// AFG_POISON_ALLOC (tests): a buffer freshly taken from the pool starts out holding NaN patterns, so that a stage that
// reads what nobody wrote shows.  (hipMemset runs on the null stream and returns early; the stages copy on non-blocking
// streams, which do not wait for it: alloc synchronises, or the fill could land on top of an upload.)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int dev = -1;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t bytes);                                    // keeps the buffer when it is large enough and on the current device
    void release();
    bool here() const;                                          // holds a buffer, and of the current device: what it carries can be read
};

// The stream of one handle (a stream being read or written): non-blocking, on the device that was current at the last
// call, destroyed on that device.
struct HandleStream {
    hipStream_t stream = nullptr;
    int dev = -1;
    HandleStream() = default;
    HandleStream(const HandleStream &) = delete;
    HandleStream &operator=(const HandleStream &) = delete;
    ~HandleStream();
    // *st: the stream on the caller's current device (`dev` from then on).  When the caller changed devices since the last
    // call the stream is made again there and *moved (optional) is set: what the handle keeps in device memory is stale.
    int current(hipStream_t *st, bool *moved = nullptr);
};

// ---- float64 output (afg_read_samples_double) ----
// One plane of `count` samples of one kind (AFG_WAV_KIND_*, AFG_F64_KIND_FLAC_S32) to doubles on the device
// (csrc/pcm_f64.hip): makes the plane's span, keeps it in a pooled buffer of its own and queues one afg_pcm_to_f64_hip
// launch on `st` behind whatever wrote the plane there.  d_in and d_out are 16-byte aligned for the fast path.  The
// object -- it holds the record the upload reads -- lives until the launch has run.
inline uint64_t f64_kind_bytes(uint32_t kind)
{
    return kind == AFG_WAV_KIND_U8 ? 1 : kind == AFG_WAV_KIND_S16 ? 2 : kind == AFG_WAV_KIND_S24 ? 3 : kind == AFG_WAV_KIND_F64 ? 8 : 4;
}
struct F64Plane {
    afg_wav_span rec;
    DevBuf span;
    int launch(uint32_t kind, const void *d_in, uint64_t count, double *d_out, hipStream_t st);
};

// The end of a stream's read: the plane its kernels left on the device (`count` samples of `kind`, queued on st) comes to
// `out` as it is, or -- f64 -- as doubles through one conversion launch; out NULL: the samples are skipped.  Waits for st.
struct PlaneFetch {
    F64Plane conv;
    DevBuf wide;
    std::vector<uint8_t> bounce;
    int run(const void *d_plane, uint32_t kind, uint64_t count, void *out, bool f64, hipStream_t st);
};

// ---- packed integer PCM output (afg_batch_opts.sample_type AFG_SAMPLE_PCM_*, afg_batch_transcode) ----
// What a batch stage delivers per sample.  A bool converts to it (true: doubles), which is all a stream's reads ask for.
// Collate mode (afg_batch_decode_to_device) is a sample type of its own, known to the stages only: the stage's floats
// stay on the device, afg_collate_hip scatters each chunk into the caller's tensor, and the download -- with the host
// plane it would fill -- is left out.  Batch file i has its slab at d_out + i * C * T and starts at first_frame[i].
constexpr uint32_t kSampleCollate = 0x100;
struct SampleOut {
    uint32_t type = AFG_SAMPLE_F32;
    bool dither = false;                                         // AFG_DITHER_LCG31, the integer types only
    uint32_t seed = 0;
    float *d_out = nullptr;                                      // collate: the tensor, n_files * C * T floats ...
    uint32_t C = 0, T = 0;
    uint64_t n_files = 0;
    const int64_t *first_frame = nullptr;                        // ... and the file frame at t = 0, per batch file (NULL: 0)
    bool no_pad = false;                                         // collate: the zero runs at the end are left out -- whoever reads
                                                                 // the tensor reads only what the files delivered (ResamplePlane)
    SampleOut() = default;
    SampleOut(bool f64) : type(f64 ? AFG_SAMPLE_F64 : AFG_SAMPLE_F32) {}
    bool f64() const { return type == AFG_SAMPLE_F64; }
    bool pcm() const { return type >= AFG_SAMPLE_PCM_S8 && type <= AFG_SAMPLE_PCM_S24; }
    bool collate() const { return type == kSampleCollate; }
    bool wide() const { return type != AFG_SAMPLE_F32; }         // a conversion launch follows the stage's kernels
    bool runs() const { return dither || collate(); }            // the stage lists where each file's samples lie (PackRun)
    bool fetch() const { return !collate(); }                    // the result comes back to host memory
    size_t es() const { return type == AFG_SAMPLE_F64 ? 8 : (type == AFG_SAMPLE_F32 || collate()) ? 4 : type - AFG_SAMPLE_PCM_S8 + 1; }   // bytes per sample
    uint8_t wav_format() const { return (uint8_t)(type - AFG_SAMPLE_PCM_S8 + AFG_WAV_S8); }
    bool operator!=(const SampleOut &o) const { return type != o.type || dither != o.dither || seed != o.seed; }
};
// A run of one file's samples inside a stage's float plane: floats [at, at + count) are samples sample0 ... of the file.
// A stage lists its runs (sorted by `at`) from the offsets it knows; they matter with dither only, where a sample's
// draws follow from its index in the file, and in collate mode, where a sample's place follows from it.  Floats outside
// every run are never delivered.  file, channels (collate mode): the file's index in the batch and its channel count.
struct PackRun { uint64_t at, count, sample0; uint32_t file = 0, channels = 0; };
void sort_runs(std::vector<PackRun> &runs);
// One launch of afg_pcm_pack_hip (csrc/pcm_pack.hip): floats [c0, c0 + n) of a stage's plane to the bytes at the same
// sample index of a byte plane that mirrors it (the sample at float i lives at byte i * es).  d_in[0] is float `origin` of
// the plane and d_out[0] its byte.  Without dither that is one span; with it one span per run-and-chunk intersection,
// draw0 taken from the run, and nothing for floats outside the runs.  The object holds the records its upload reads and lives until the
// launch has run: the rule F64Plane follows.
struct PackPlane {
    std::vector<afg_pcm_pack_span> recs;
    DevBuf spans;
    int launch(const SampleOut &out, const float *d_in, uint8_t *d_out, uint64_t origin, uint64_t c0, uint64_t n,
               const std::vector<PackRun> &runs, hipStream_t st);
};
// One launch of afg_collate_hip (csrc/collate.hip) beside PackPlane: the runs' intersections with floats [c0, c0 + n) of
// a stage's plane -- d_in[0] is float `origin` of it -- become copy spans into the tensor of `out`; floats outside the
// runs go nowhere.  The same lifetime rule: the object holds the records its upload reads and lives until the launch has run.
struct CollatePlane {
    std::vector<afg_collate_span> recs;
    DevBuf spans;
    int launch(const SampleOut &out, const float *d_in, uint64_t origin, uint64_t c0, uint64_t n, const std::vector<PackRun> &runs, hipStream_t st);
    // what the files did not fill, as zero runs: file i delivered frames[i] frames of channels[i] channels (0, 0: it failed)
    int pad(const SampleOut &out, const std::vector<int64_t> &frames, const std::vector<int> &channels, hipStream_t st);
private:
    int submit(const SampleOut &out, const float *d_in, uint64_t in_floats, hipStream_t st);
};
// ---- the tensor at one sample rate (afg_batch_decode_resampled, host/afg_resample.cpp) ----
// What the call asks for, with the defaults filled in, and the scratch tensor [files, R_s, T_s] its collate pass fills at
// the files' own rates: scratch frame 0 of a file is file frame max(0, first_frame - H).
struct ResampleJob {
    uint32_t C = 0, T = 0, samplerate = 0, Z = 6, in_channels = 2, max_in_rate = 48000;
    bool mono = false;
    uint32_t R_s = 0, H = 0;
    uint64_t T_s = 0;
    void plan();                                                 // R_s, H and T_s from the fields above
};
// The filter table of one rate pair (afg_resample_taps), made once per (in, out, Z) and kept for the process.
struct ResampleTable {
    uint32_t M = 0, L = 0, W = 0;
    std::shared_ptr<const std::vector<float>> taps;              // L * 2 W floats (none for equal rates)
};
int resample_table(uint32_t in_rate, uint32_t out_rate, uint32_t Z, ResampleTable &t);   // AFG_ERR_INVALID: afg_last_error says why
// One launch of afg_resample_hip (csrc/resample.hip) behind a collate pass: files [0, n) of a sublist, whose scratch slabs
// lie at d_scratch in list order, to their slabs in d_out (the sublist's first).  One record per output row; a failed
// or refused file's rows, and rows the file has no channel for, are records without input.  Refused files (rate, channel
// count) get their status and message in `items`; the message strings live in `messages`.  The object holds the records
// and tables its uploads read: it lives until `st` has drained.
struct ResamplePlane {
    std::vector<afg_resample_row> recs;
    std::vector<float> taps;
    DevBuf d_recs, d_taps;
    int launch(const ResampleJob &job, const float *d_scratch, afg_batch_item *items, size_t n, const int64_t *first_frame,
               const int64_t *scratch_frame0, float *d_out, std::deque<std::string> &messages, hipStream_t st);
};
// afg_batch_decode_resampled in two steps (afg_batch.cpp), for an entry that runs it into a tensor of its own
// (afg_batch_decode_mel): the checks of the options behind struct_size, which fill in the job and touch no device; then the
// tensor of a checked call into d_out, with `items` (n_files of them, zeroed) and the strings of `messages` as the entry
// returns them.
int resampled_check(const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files, ResampleJob &job);
int resampled_run(const ResampleJob &job, const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files,
                  float *d_out, afg_batch_item *items, std::deque<std::string> &messages);
// ---- what the tensor entries share (afg_batch_decode_resampled and the stages that run behind it) ----
// body() under the entries' one catch: what throws there is out of host memory.
template <typename Body> int tensor_entry(Body body)
{
    try {
        return body();
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}
// An entry's required pointers in the order it names them: the first NULL one is refused by name; with all of them there,
// `out` -- one of them -- is zeroed.
struct EntryArg { const char *name; const void *p; };
inline int entry_args(const char *who, std::initializer_list<EntryArg> args, afg_batch_result *out)
{
    for (const EntryArg &a : args)
        if (!a.p) { afg::set_error("%s: NULL %s", who, a.name); return AFG_ERR_INVALID; }
    out->n_files = 0; out->items = nullptr; out->owner = nullptr;
    return AFG_OK;
}
// How an entry that takes afg_resample_opts goes on behind entry_args: the struct_size test, then resampled_check, which
// fills in the job.
inline int resampled_opts_check(const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files, ResampleJob &job)
{
    if (opts->struct_size < offsetof(afg_resample_opts, lowpass_width) + sizeof(uint32_t)) {
        afg::set_error("afg_resample_opts.struct_size too small");
        return AFG_ERR_INVALID;
    }
    return resampled_check(opts, data, length, n_files, job);
}
// The afg_resample_opts of an entry whose own options (afg_mel_opts, afg_stft_opts, afg_resample_opts itself) carry its fields.
template <typename Opts> afg_resample_opts resample_opts_of(const Opts &o)
{
    afg_resample_opts ro;
    std::memset(&ro, 0, sizeof(ro));
    ro.struct_size = (uint32_t)sizeof(ro);
    ro.n_threads = o.n_threads; ro.channels = o.channels; ro.frames = o.frames; ro.first_frame = o.first_frame;
    ro.samplerate = o.samplerate; ro.mono = o.mono; ro.in_channels = o.in_channels; ro.max_in_rate = o.max_in_rate;
    ro.lowpass_width = o.lowpass_width;
    return ro;
}
// The files of one sublist: as many as the scratch budget (2 GiB, or what afg_dev_option says for `budget_option`) holds
// slabs of slab_bytes, one at the least.
inline size_t sublist_size(int n_files, uint64_t slab_bytes, afg::DevOption budget_option)
{
    const long opt = afg::dev_option(budget_option);
    const uint64_t budget = opt > 0 ? (uint64_t)opt : (uint64_t)2 << 30;
    return (size_t)std::min<uint64_t>((uint64_t)n_files, std::max<uint64_t>(budget / slab_bytes, 1));
}
// Waits for the null stream on the way out of an entry that queues on it.  Whatever the queued uploads read -- record
// vectors, planes, pooled buffers -- is declared in front of it, so that it is still there when the wait ends.
struct NullStreamDrain {
    ~NullStreamDrain() { (void)hipStreamSynchronize(nullptr); }
};
// The records of a launch into a pooled buffer, queued on st.  recs is read until st has passed the copy.
template <typename Rec> int upload_records(DevBuf &d, const std::vector<Rec> &recs, hipStream_t st)
{
    if (int rc = d.alloc(recs.size() * sizeof(Rec))) return rc;
    AFG_HIP_CHECK(hipMemcpyAsync(d.p, recs.data(), recs.size() * sizeof(Rec), hipMemcpyHostToDevice, st));
    return AFG_OK;
}
// A batch result in the making, for every batch entry: alloc makes the zeroed items and their owner -- what afg_batch_free
// lets go: the planes the items' PCM points into (afg_batch.cpp) and the message strings that are not static -- and finish
// hands both to `out`; until then they go with the object.
struct BatchOwner;
struct BatchResult {
    afg_batch_item *items = nullptr;
    int n_files = 0;
    BatchOwner *owner = nullptr;
    BatchResult() = default;
    BatchResult(const BatchResult &) = delete;
    BatchResult &operator=(const BatchResult &) = delete;
    ~BatchResult();
    int alloc(int n);                                            // AFG_ERR_OOM: no memory for the items
    std::deque<std::string> &messages();
    int finish(afg_batch_result *out);                           // AFG_OK
};

// ---- mel spectrogram features (afg_batch_decode_mel, host/afg_melspec.cpp) ----
// The tables of one parameter set, made once and kept for the process: afg_mel_basis's and afg_mel_filters'.
// With AFG_MEL_ALGO_FFT `basis` holds afg_mel_fft_tables' table instead.
struct MelTables {
    std::shared_ptr<const std::vector<float>> basis, filters;
};
int mel_tables(const afg_mel_opts &o, MelTables &t);            // AFG_ERR_INVALID: afg_last_error says why
// One launch of afg_melspec_hip (csrc/melspec.hip), or by o.algorithm of afg_melspec_fft_hip (csrc/melspec_fft.hip), over rows [0, n_rows) of T samples each, contiguous in d_in, to slabs of
// n_mels * n_out floats, contiguous in d_out.  The object holds the records its upload reads, and the tables on the device
// (uploaded on the first launch): it lives until `st` has drained.
struct MelPlane {
    std::vector<afg_mel_row> recs;
    DevBuf d_recs, d_basis, d_filters;
    bool tables_up = false;
    int launch(const afg_mel_opts &o, const MelTables &t, const float *d_in, uint64_t n_rows, float *d_out, hipStream_t st);
};

// ---- normalisation (afg_batch_decode_resampled_norm, afg_batch_decode_mel_norm; host/afg_normalize.cpp) ----
// The valid length of a file's rows in the tensor at one rate: min(T, ceil((frames - first_frame) * L / M)) with
// M / L = in_rate / out_rate in lowest terms; 0 when that is not positive or a rate is 0.
uint32_t norm_valid(int64_t frames, int64_t first_frame, uint32_t in_rate, uint32_t out_rate, uint32_t T);
// The groups of files [0, n) of a tensor [n, C, T] made by resampled_run (items: what it returned for them).
void norm_file_groups(const ResampleJob &job, const afg_batch_item *items, size_t n, const int64_t *first_frame, std::vector<afg_norm_group> &groups);
// One afg_normalize_hip over `groups`, in place on d_plane (plane_floats of it), with the groups, the partials and -- when
// the caller has none, d_stats NULL -- the records in pooled buffers.  The object holds what its upload reads: it lives until
// `st` has drained.
struct NormPlane {
    std::vector<afg_norm_group> recs;
    DevBuf d_recs, d_partials, d_own_stats;
    int launch(const afg_norm_params &prm, std::vector<afg_norm_group> &groups, float *d_plane, uint64_t plane_floats, afg_norm_stats *d_stats,
               hipStream_t st);
};
// afg_batch_decode_mel with its two optional normalisations (afg_melspec.cpp): both entries run through it
int mel_batch(const uint8_t *const *data, const size_t *length, int n_files, const afg_mel_opts *opts, const afg_norm_params *wave_norm,
              const afg_norm_params *feat_norm, float *d_out, afg_batch_result *out);

// The conversion that follows a stage's kernels, by what `out` asks for: floats [c0, c0 + n) of the stage's 4-byte plane
// (elements of `kind`; d_in[0] is element `origin` of it) go to the same samples of its converted mirror (d_out[0] is the
// mirror of element `origin`) as doubles (afg_pcm_to_f64_hip) or packed integers (afg_pcm_pack_hip), or -- collate mode,
// d_out unused -- into the caller's tensor (afg_collate_hip); AFG_SAMPLE_F32: nothing.  One launch on `st`, behind whatever
// wrote the plane there.
// Lifetime: every launch uploads records asynchronously from host memory this object owns.  It therefore lives, and is not
// cleared, until the streams it queued on have drained: declare it in front of whatever drains them on the way out
// (StageStreams, run_chunks), and call clear() only behind a drain.
struct SampleConv {
    int launch(const SampleOut &out, uint32_t kind, const void *d_in, uint64_t origin, uint64_t c0, uint64_t n, void *d_out,
               const std::vector<PackRun> &runs, hipStream_t st);
    void clear() { widen.clear(); packs.clear(); collated.clear(); }
private:
    std::vector<std::unique_ptr<F64Plane>> widen;
    std::vector<std::unique_ptr<PackPlane>> packs;
    std::vector<std::unique_ptr<CollatePlane>> collated;
};
// The converted side of a batch stage's two output slots: the chunk in `slot` (its first float is float `origin` of the
// stage's plane) is converted into buf[slot] on the kernel stream, between the stage's kernels and the download.
struct WideSlots {
    DevBuf buf[2];                                               // out.es() bytes per sample (not needed in collate mode)
    SampleConv conv;
    int alloc(size_t samples, size_t es);
    int launch(int slot, const SampleOut &out, uint32_t kind, const void *d_in, uint64_t origin, uint64_t n, const std::vector<PackRun> &runs, hipStream_t st)
    {
        return conv.launch(out, kind, d_in, origin, origin, n, buf[slot].p, runs, st);
    }
};

// ---- what the pipelined stages share ----
// The streams of one stage -- the kept pair, or with `three` the pair and a kernel stream between them -- and the events
// that chain them.  `e` keeps the first HIP error of take, chain and drain; a stage reports it once it has drained.  The
// destructor drains the streams and gives them back, so the stage's buffers -- declared in front of it -- are idle when
// they are let go, on every way out.
struct StageStreams {
    hipStream_t up = nullptr, down = nullptr, mid = nullptr;
    hipError_t e = hipSuccess;
    StageStreams() = default;
    StageStreams(const StageStreams &) = delete;
    StageStreams &operator=(const StageStreams &) = delete;
    ~StageStreams() { release(); }
    void take(bool three = false);                              // (e tells whether it worked)
    void chain(hipStream_t from, hipStream_t to);               // what is queued on `to` from here on waits for what is on `from` now
    // The end of the stage's device work: waits for up, mid and down in that order (the first error wins); nothing is queued
    // behind it.  uploads_done (optional, a trace's clock) runs between the waits for the kernels and for the downloads.
    void drain(const std::function<void()> &uploads_done = nullptr);
    void release();                                             // drained, the events destroyed, the streams back in the pool
private:
    void sync(hipStream_t st);
    std::vector<hipEvent_t> events;
    bool drained = false;
};

// Files [f0, f1) of n: from f0 on until the members' weights reach `target`.  member(i, &w): file i belongs to the stage,
// with weight w.  first / last: the first and last member of the chunk (both n: it has none).
struct FileChunk { size_t f1, first, last, weight; };
template <typename M> FileChunk cut_chunk(size_t f0, size_t n, size_t target, M member)
{
    FileChunk c{ f0, n, n, 0 };
    for (; c.f1 < n && c.weight < target; c.f1++) {
        size_t w = 0;
        if (!member(c.f1, w)) continue;
        c.weight += w;
        if (c.first == n) c.first = c.f1;
        c.last = c.f1;
    }
    return c;
}

// ---- the chunk pipeline of a batch stage ----
// How much a stage puts into a chunk at least, or at most: `dflt`, unless afg_dev_option("stage_chunk_samples", n) says n.
// The stages' own figures are millions of samples; tests set a few thousand, so that small files span several chunks.
uint64_t stage_chunk_samples(uint64_t dflt);

// Chunks 0 .. n_chunks - 1 go through two slots in turn (chunk c uses slot c & 1) on the kept stream pair: uploads and
// kernels on `up`, downloads on `down`, so that chunk c + 1 is worked on while chunk c comes back.  The caller keeps the
// slots' device buffers and stagings; run_chunks owns the pair, the events and the order:
//   before(up)             (optional) what every chunk needs, queued once ahead of chunk 0
//   upload(c, slot, up)    (optional) fills the slot's host staging and queues its upload; the host first waits until the
//                          upload of chunk c - 2 has left that staging.  Without it nothing ever waits on the host.
//   launch(c, slot, up)    the kernels, writing the slot's output buffer; they wait until chunk c - 2 has come back from it
//   download(c, slot, down) queued behind the chunk's kernels
// A step returns AFG_OK or the status run_chunks returns at once; on every way out both streams are drained before the
// pair goes back, so no buffer of the caller is still in use when run_chunks has returned.
using ChunkStep = std::function<int(size_t c, int slot, hipStream_t st)>;
int run_chunks(size_t n_chunks, const std::function<int(hipStream_t up)> &before, const ChunkStep &upload, const ChunkStep &launch,
               const ChunkStep &download);

// The chunks of the MOD and XM stages: song j fills output frames [start[j], end[j]) of the batch's PCM plane, and a chunk
// is closed behind the song that brings it to kSongChunkFrames.  Chunk c is songs [first[c], first[c + 1]).
constexpr uint64_t kSongChunkFrames = (uint64_t)16 << 20;          // 128 MB of PCM (afg_dev_option("stage_chunk_samples") / 2 in tests)
struct SongChunks {
    std::vector<size_t> first;
    std::vector<uint64_t> frames;                                   // per chunk: from its first song's start to its last song's end
    uint64_t max_frames = 1;                                        // of the longest chunk
    SongChunks(const std::vector<uint64_t> &start, const std::vector<uint64_t> &end);
    size_t count() const { return first.size() - 1; }
    // the song records as the mixer takes them: output frame and tick base count from the chunk's first song
    template <typename Song> std::vector<Song> relative(const std::vector<Song> &songs) const
    {
        std::vector<Song> rel(songs);
        for (size_t c = 0; c < count(); c++)
            for (size_t j = first[c]; j < first[c + 1]; j++) {
                rel[j].out_frame -= songs[first[c]].out_frame;
                rel[j].tick_base -= songs[first[c]].tick_base;
            }
        return rel;
    }
};

}  // namespace afg_front
