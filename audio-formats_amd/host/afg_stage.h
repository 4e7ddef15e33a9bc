// afg_stage.h -- what the host stages beside afg_host.cpp share (MOD, XM and WAV decoding, the batch encoder, the write
// stream): the library's pools, a pooled device buffer, a handle's own stream, and the chunk pipeline of the batch stages.
#pragma once
#include "../../include/afg.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

namespace afg_front {

// ---- the pools and helper threads of afg_host.cpp ----
int devpool_take(size_t bytes, void **out, size_t *cap_out);   // device memory, kept between calls
void devpool_give(void *p, size_t cap, int dev);               // dev: the device it was taken on
// a page-locked staging lease (pinning memory costs about as much as moving it); the buffer goes back to the pool when
// the last owner lets go.  NULL: out of memory.
std::shared_ptr<void> staging_lease(size_t bytes, void **p);
hipError_t streams_take(hipStream_t *up, hipStream_t *down);   // the kept upload / download pair of the current device
void streams_give(hipStream_t up, hipStream_t down);           // ... given back drained
// fn(0) .. fn(n - 1) on the library's pooled host threads; n_threads 0 = the library's choice (afg_batch_decode)
void parallel_run(size_t n, int n_threads, const std::function<void(size_t)> &fn);

constexpr uint64_t align16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// Device memory from the pool, returned to the device it was taken on.
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

// The float64 side of a batch stage's two output slots (afg_batch_opts.sample_type): the chunk in `slot` is widened from the
// stage's float plane into wide[slot] on the kernel stream, between the stage's kernels and the download.  One F64Plane per
// launch, kept until the stage has drained (run_chunks drains on every way out).
struct F64Slots {
    DevBuf wide[2];
    std::vector<std::unique_ptr<F64Plane>> conv;
    int alloc(size_t samples);
    int launch(int slot, uint32_t kind, const void *d_in, uint64_t count, hipStream_t st);
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
// The packed side of a batch stage's two output slots, beside F64Slots.
struct PackSlots {
    DevBuf bytes[2];
    std::vector<std::unique_ptr<PackPlane>> conv;
    int alloc(size_t samples, size_t es);
    int launch(int slot, const SampleOut &out, const void *d_in, uint64_t origin, uint64_t n, const std::vector<PackRun> &runs, hipStream_t st);
};

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
