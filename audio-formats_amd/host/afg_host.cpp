// afg_host.cpp -- host front-ends and the AudioStream-shaped surface of the C ABI.
//
// What stays on the host (bitstream / entropy parsing) for the formats whose
// front-ends exist so far:
//   FLAC  container + frame/subframe headers + Rice residuals   (reference drflac.d:680-1695,
//         :1887-2153; the prediction half of drflac.d:1235 is NOT done here: residuals and
//         subframe parameters become afg_flac_subframe / afg_flac_frame records)
//   QOA   file/frame headers only (reference qoa.d:413-486): the device reads the raw bytes
// and the outer surface mirroring AudioStream (stream.d:150-170 openFromMemory, :295-412
// getters, :429-637 readSamplesFloat): parse the file into transform-stage records, restore the
// samples on the device, serve interleaved floats.
#include "../csrc/afg_common.h"
#include "afg_flac_front.h"
#include "afg_mod_front.h"
#include "afg_wav_front.h"
#include "afg_xm_front.h"
#include "afg_mp3_front.h"
#include "afg_opus_front.h"
#include "afg_batch.h"
#include "afg_stage.h"
#include "afg_vorbis_front.h"
#include "afg_write_stream.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

using namespace afg_front;

// debugging aids, read ONCE when the library is loaded (set them before that): a trace of the host stages and the staging
// pool, and poisoned allocations (the test-suite runs with it: an output byte the library forgets to write shows up as NaN)
namespace afg_front {
const bool g_trace = std::getenv("AFG_TRACE") != nullptr;
}  // namespace afg_front

namespace {

static const bool g_poison_alloc = std::getenv("AFG_POISON_ALLOC") != nullptr;
// Vorbis: inverse coupling and floor curves on the device (default) or in the host parser (AFG_VORBIS_HOST_FLOOR=1)
static bool vorbis_floor_on_device() { return afg::dev_option(afg::kDevVorbisHostFloor) <= 0; }

// FLAC: residual rows that fit 16 bits are packed as int16 (default) or left as int32 (AFG_FLAC_HOST_RES32=1)
static bool flac_rows_int16() { return afg::dev_option(afg::kDevFlacHostRes32) <= 0; }

// Device buffers of the batch path are kept between calls (round 6).  A batch call used to hipMalloc its planes and hipFree them
// on the way out; the driver wipes freed video memory with the copy engines, and that wipe ran into the NEXT call's transfers:
// of back-to-back calls over the 2048-file FLAC batch every one but the first after a pause moved its 0.8 GB in 21.8 ms, the
// first in 15.4 (AFG_TRACE; the pipeline alone, tools/ubench_pipe.hip: 10.9 ms).  The pool keeps what it has seen, per device,
// bounded in count and bytes; afg_host_pool_trim() frees it.
class DevicePool {
public:
    int take(size_t bytes, void **out, size_t *cap_out)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        const size_t want = bytes ? bytes : 1;
        {
            std::lock_guard<std::mutex> lk(mu_);
            size_t best = free_.size();
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].dev == dev && free_[i].cap >= want && free_[i].cap <= 2 * want + ((size_t)1 << 20) &&
                    (best == free_.size() || free_[i].cap < free_[best].cap)) best = i;
            if (best != free_.size()) {
                *out = free_[best].p; *cap_out = free_[best].cap;
                held_ -= free_[best].cap;
                free_.erase(free_.begin() + (long)best);
                return AFG_OK;
            }
        }
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipErrorOutOfMemory && trim()) e = hipMalloc(&p, want);          // what the pool holds may be what is missing
        if (e != hipSuccess) { afg::set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return AFG_ERR_OOM; }
        *out = p; *cap_out = want;
        return AFG_OK;
    }
    void give_back_on(int dev, void *p, size_t cap)      // dev: the device the buffer was taken on (-1: unknown)
    {
        const bool known = dev >= 0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (known && free_.size() < 128 && held_ + cap <= ((size_t)64 << 30)) {
                free_.push_back({ dev, p, cap });
                held_ += cap;
                return;
            }
        }
        (void)hipFree(p);
    }
    size_t trim()
    {
        std::vector<Buf> drop;
        {
            std::lock_guard<std::mutex> lk(mu_);
            drop.swap(free_);
            held_ = 0;
        }
        size_t bytes = 0;
        for (auto &b : drop) { (void)hipFree(b.p); bytes += b.cap; }
        return bytes;
    }
private:
    struct Buf { int dev; void *p; size_t cap; };
    std::mutex mu_;
    std::vector<Buf> free_;
    size_t held_ = 0;
};
DevicePool g_devpool;
}  // namespace

namespace {

// page-locked host memory: H2D / D2H run at PCIe rate without a staging copy
struct PinnedBuf {
    void *p = nullptr;
    ~PinnedBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    int alloc(size_t bytes)
    {
        hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
        if (e != hipSuccess) { p = nullptr; afg::set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return AFG_ERR_OOM; }
        return AFG_OK;
    }
};

// Staging buffers (gathered inputs, the raw MP3 PCM plane) are reused across calls: pinning memory costs about as
// much as moving it.  The pool keeps the few largest buffers it has seen, bounded in count and bytes.
class StagingPool {
public:
    int take(size_t bytes, StagingLease &out)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            size_t best = free_.size();
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].second >= bytes && (best == free_.size() || free_[i].second < free_[best].second)) best = i;
            if (best != free_.size()) {
                out.p = free_[best].first; out.cap = free_[best].second;
                held_ -= out.cap;
                free_.erase(free_.begin() + (long)best);
                if (g_poison_alloc) std::memset(out.p, 0xff, out.cap);     // (tests: see DevBuf)
                return AFG_OK;
            }
        }
        void *p = nullptr;
        const size_t cap = bytes ? bytes : 1;
        if (g_trace) fprintf(stderr, "[afg] staging pool miss: pinning %.1f MB\n", cap / 1e6);
        hipError_t e = hipHostMalloc(&p, cap, hipHostMallocPortable);
        if (e != hipSuccess) { afg::set_error("hipHostMalloc(%zu) failed: %s", cap, hipGetErrorString(e)); return AFG_ERR_OOM; }
        out.p = p; out.cap = cap;
        if (g_poison_alloc) std::memset(out.p, 0xff, out.cap);
        return AFG_OK;
    }
    // Frees every buffer that is not on lease (afg_host_pool_trim): a long-lived process gives the pinned memory back.
    size_t trim()
    {
        std::vector<std::pair<void *, size_t>> drop;
        {
            std::lock_guard<std::mutex> lk(mu_);
            drop.swap(free_);
            held_ = 0;
        }
        size_t bytes = 0;
        for (auto &b : drop) { (void)hipHostFree(b.first); bytes += b.second; }
        return bytes;
    }
    void give_back(void *p, size_t cap)                  // (the end of a StagingLease)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (free_.size() < 128 && held_ + cap <= ((size_t)24 << 30)) {      // (a grouped batch leases a set of buffers per group)
            free_.emplace_back(p, cap);
            held_ += cap;
        } else {
            (void)hipHostFree(p);
        }
    }
private:
    std::mutex mu_;
    std::vector<std::pair<void *, size_t>> free_;
    size_t held_ = 0;
};
StagingPool g_staging;

// The upload / download stream pair of a device stage, kept between calls.  Creating and destroying two streams cost 2.8 ms of
// every batch call (hipStreamCreateWithFlags 0.8 ms, hipStreamDestroy 0.6 ms each), and a freshly created pair moves its first
// several hundred megabytes at half the rate of a pair that has been used before (round 6, AFG_TRACE on the 2048-file FLAC
// batch: 67 MB downloads 2.8 ms each on new streams, 1.4 ms on streams a probe had just run 1 GB through; `tools/ubench_pipe.hip`
// is the pipeline alone).  A stage leases a pair (stages of one call may run on two host threads) and gives it back drained.
class StreamPool {
public:
    // `mid` (optional): a third stream for the kernels of a stage whose uploads should never wait behind them
    hipError_t take(hipStream_t *up, hipStream_t *down, hipStream_t *mid = nullptr)
    {
        *up = *down = nullptr;
        if (mid) *mid = nullptr;
        int dev = 0;
        if (hipError_t e = hipGetDevice(&dev)) return e;
        Pair got{ -1, nullptr, nullptr, nullptr };
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].dev == dev) {
                    got = free_[i];
                    free_.erase(free_.begin() + (long)i);
                    break;
                }
        }
        hipError_t e = hipSuccess;
        if (!got.up) e = hipStreamCreateWithFlags(&got.up, hipStreamNonBlocking);
        if (e == hipSuccess && !got.down) e = hipStreamCreateWithFlags(&got.down, hipStreamNonBlocking);
        if (e == hipSuccess && mid && !got.mid) e = hipStreamCreateWithFlags(&got.mid, hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (hipStream_t st : { got.up, got.down, got.mid }) if (st) (void)hipStreamDestroy(st);
            return e;
        }
        *up = got.up; *down = got.down;
        if (mid) *mid = got.mid;
        else if (got.mid) {                              // not wanted this time: keep it for a later lease
            std::lock_guard<std::mutex> lk(mu_);
            spare_mid_.push_back({ dev, got.mid });
        }
        return e;
    }
    void give(hipStream_t up, hipStream_t down, hipStream_t mid = nullptr)
    {
        int dev = 0;
        const bool known = up && down && hipGetDevice(&dev) == hipSuccess;
        std::unique_lock<std::mutex> lk(mu_);
        if (known && !mid)
            for (size_t i = 0; i < spare_mid_.size(); i++)
                if (spare_mid_[i].first == dev) { mid = spare_mid_[i].second; spare_mid_.erase(spare_mid_.begin() + (long)i); break; }
        if (known && free_.size() < 16) { free_.push_back({ dev, up, down, mid }); return; }
        lk.unlock();
        for (hipStream_t st : { up, down, mid }) if (st) (void)hipStreamDestroy(st);
    }
private:
    struct Pair { int dev; hipStream_t up, down, mid; };
    std::vector<std::pair<int, hipStream_t>> spare_mid_;
    std::mutex mu_;
    std::vector<Pair> free_;
};
StreamPool g_streams;
}  // namespace

// the pools as the stages use them (declared in afg_stage.h and afg_batch.h)
namespace afg_front {
bool poison_alloc() { return g_poison_alloc; }
int devpool_take(size_t bytes, void **out, size_t *cap_out) { return g_devpool.take(bytes, out, cap_out); }
void devpool_give(void *p, size_t cap, int dev) { g_devpool.give_back_on(dev, p, cap); }
StagingLease::~StagingLease() { if (p) g_staging.give_back(p, cap); }
int staging_take(size_t bytes, StagingLease &out) { return g_staging.take(bytes, out); }
// a page-locked staging lease; the buffer goes back to the pool when the last owner lets go
std::shared_ptr<void> staging_lease(size_t bytes, void **p)
{
    auto lease = std::make_shared<StagingLease>();
    if (g_staging.take(bytes, *lease)) return nullptr;
    *p = lease->p;
    return lease;
}
hipError_t streams_take(hipStream_t *up, hipStream_t *down, hipStream_t *mid) { return g_streams.take(up, down, mid); }
void streams_give(hipStream_t up, hipStream_t down, hipStream_t mid) { g_streams.give(up, down, mid); }
}  // namespace afg_front

namespace {


// Helper threads are kept between calls: the batch path runs one parallel_for per chunk of files, and creating a
// few hundred threads each time cost more than the parsing they did.
class HelperPool {
public:
    ~HelperPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    // Runs work() on the caller and on up to `helpers` pooled threads; returns when all of them are done.
    // One job at a time: a second caller (another host thread in the library) just runs its work alone.
    void run(unsigned helpers, const std::function<void()> &work)
    {
        if (helpers == 0) { work(); return; }                // (without touching the pool: the caller wants no helpers)
        std::unique_lock<std::mutex> job_lock(job_mu_, std::try_to_lock);
        if (!job_lock.owns_lock()) { work(); return; }
        {
            std::lock_guard<std::mutex> lk(mu_);
            while (workers_.size() < helpers && workers_.size() < 1024) workers_.emplace_back([this] { loop(); });
            job_ = &work; want_ = helpers; started_ = finished_ = 0; epoch_++;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        want_ = started_;                                    // no helper may still pick the job up
        done_cv_.wait(lk, [&] { return finished_ == started_; });
        job_ = nullptr;
    }
private:
    void loop()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || (epoch_ != seen && started_ < want_); });
            if (stop_) return;
            seen = epoch_;
            started_++;
            const std::function<void()> *job = job_;
            lk.unlock();
            (*job)();
            lk.lock();
            finished_++;
            done_cv_.notify_all();
        }
    }
    std::mutex mu_, job_mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> workers_;
    const std::function<void()> *job_ = nullptr;
    unsigned want_ = 0, started_ = 0, finished_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};
HelperPool g_helpers;
// A multi-device batch runs one host thread per device, each with its own helpers (g_helpers serves one job at a time)
HelperPool g_device_helpers[16];
// ... and the second host thread of a grouped batch (afg_batch_decode_ex) its own: a pool serves one job at a time, and a
// group's parse pass must not find it taken by the other group's small gather jobs (it would run on one thread)
HelperPool g_group_helpers[16];
thread_local HelperPool *tl_helpers = nullptr;
}  // namespace

namespace afg_front {
void helpers_run(unsigned helpers, const std::function<void()> &work) { (tl_helpers ? *tl_helpers : g_helpers).run(helpers, work); }
}  // namespace afg_front

namespace {


// chunks a device stage cuts its files into (8; a group of a grouped batch -- below -- is itself a piece of a pipeline and takes 2).
// Per host thread: the second thread of a batch, which decodes the FLAC / QOA files, has always cut into 8.
thread_local unsigned tl_stage_chunks = 8;

StageCtx stage_ctx(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, const uint8_t *own, unsigned threads,
                   SampleOut so, BatchOut &out)
{
    return StageCtx{ parsed, data, len, own, threads, so, tl_stage_chunks, out, StageTimer() };
}

// what the caller is told of every file (the PCM offsets are the layouts')
void fill_metadata(StageCtx &ctx)
{
    for (size_t i = 0; i < ctx.nf(); i++) {
        Parsed &p = ctx.parsed[i];
        Decoded &dcd = ctx.out.files[i];
        const int fmt = dcd.format = ctx.fmt_of(i);
        if (fmt == AFG_FORMAT_FLAC) {
            dcd.channels = (int)p.fi.channels;
            dcd.samplerate = (float)p.fi.sample_rate;
            dcd.frames = (int64_t)(p.flac.out_samples / p.fi.channels);
            dcd.declared_frames = (int64_t)p.fi.total_samples;      // totalSampleCount / channels, stream.d:1631
        } else if (fmt == AFG_FORMAT_MP3) {
            dcd.channels = p.mp3.channels;
            dcd.samplerate = (float)p.mp3.hz;
            dcd.frames = (int64_t)(p.mp3.pcm_samples / (uint64_t)p.mp3.channels);
            dcd.declared_frames = (int64_t)(p.mp3.declared_samples / (uint64_t)p.mp3.channels);   // stream.d:1737
        } else if (fmt == AFG_FORMAT_OGG) {
            dcd.channels = p.ogg.channels;
            dcd.samplerate = (float)p.ogg.sample_rate;
            dcd.frames = (int64_t)p.ogg.pcm_frames;
            dcd.declared_frames = (int64_t)p.ogg.total_samples;    // stb_vorbis_stream_length_in_samples, stream.d:1696
        } else if (fmt == AFG_FORMAT_OPUS) {
            dcd.channels = p.opus.channels;
            dcd.samplerate = 48000.0f;                              // OpusFileCtx.rate (dopus.d:7973)
            dcd.declared_frames = p.opus.declared_frames;           // smpduration(), stream.d:1609
            // the reference never reads past the declared length (stream.d:439-442); the pre-skip samples are not dropped
            dcd.frames = std::min<int64_t>((int64_t)p.opus.pcm_frames, std::max<int64_t>(p.opus.declared_frames, 0));
            if (p.opus.error) {                                     // a packet failed: the read that reaches it reports an error
                dcd.status = AFG_ERR_INVALID;
                dcd.message = kErrorDecoderInitializationFailed;    // (the string stream.d:454 sets)
            }
        } else if (fmt == AFG_FORMAT_QOA) {
            dcd.channels = (int)p.qi.channels;
            dcd.samplerate = (float)p.qi.samplerate;
            dcd.frames = (int64_t)(p.qoa.back().out_off / p.qi.channels) + p.qoa.back().samples;
            dcd.declared_frames = (int64_t)p.qi.samples;
        } else {
            dcd.status = AFG_ERR_UNSUPPORTED;
            dcd.message = p.opus_mode ? kErrorOpusMode : kErrorUnknownFormat;
        }
    }
}

// The device stages for a set of parsed files (afg_batch.h), each handed in with its optional inputs set: every FLAC record
// of the batch in one stage, every QOA frame in another, and so on; the results come back as one plane, laid out FLAC,
// QOA, MP3, Vorbis, Opus.
// so.f64() (afg_read_samples_double, afg_batch_opts.sample_type): the result plane holds doubles.  Every stage's device plane
// -- int32 for FLAC, float for the others -- is widened by afg_pcm_to_f64_hip behind the stage's kernels, on their
// stream, and the doubles are what comes back.  The batch path's MP3 and Opus planes were widened by their own pipelines.
// AFG_SAMPLE_PCM_* (afg_batch_opts.sample_type): the result plane holds samples of 1, 2 or 3 bytes, packed from every
// stage's float plane by afg_pcm_pack_hip at the same place; FLAC restores to float as for a float read.
// Collate mode (afg_batch_decode_to_device): there is no result plane.  afg_collate_hip scatters every stage's float plane
// into the caller's tensor where the other types convert, and the downloads are left out; parsed[i] is batch file i.
int decode_parsed(StageCtx &ctx, FlacDecode &flac, Mp3Decode &mp3, VorbisDecode &ogg, OpusDecode &opus)
{
    const SampleOut &so = ctx.so;
    if (mp3.staged && mp3.staged->blocks && mp3.staged->so != so) { afg::set_error("decode_parsed: the MP3 stage's sample type differs"); return AFG_ERR_INVALID; }
    BatchOut &out = ctx.out;
    out.f64 = so.f64();
    out.files.assign(ctx.nf(), Decoded());
    QoaDecode qoa;
    size_t at = flac.layout(ctx, 0);
    at += qoa.layout(ctx, at);
    const size_t main_floats = at;                           // FLAC and QOA: converted in place of the plane
    at += mp3.layout(ctx, at);
    size_t ogg_floats = 0;
    if (int rc = ogg.layout(ctx, at, &ogg_floats)) return rc;
    at += ogg_floats;
    mp3.deliver_in_place(ctx);
    at += opus.layout(ctx, at);
    out.plane_floats = at;
    if (out.plane_floats) {
        if (so.fetch()) if (int rc = staging_take(out.plane_floats * so.es(), out.plane)) return rc;
        ctx.tm.lap("layout + plane alloc");
        // (the converted planes and the conversion records live out here and in the stages the caller holds: on an early way
        //  out of a stage they are let go only after the device has drained, below them)
        StageDev dev;
        if (int rc = dev.d_out.alloc(out.plane_floats * sizeof(float))) return rc;
        if (so.wide() && so.fetch()) if (int rc = dev.d_out64.alloc(std::max<size_t>(main_floats * so.es(), 16))) return rc;
        struct Drain { bool on; ~Drain() { if (on) (void)hipDeviceSynchronize(); } } drain{ so.wide() };
        if (int rc = flac.run(ctx, dev)) return rc;
        if (int rc = qoa.run(ctx, dev)) return rc;
        if (int rc = mp3.run(ctx, dev)) return rc;
        if (int rc = ogg.run(ctx, dev)) return rc;
        if (int rc = opus.run(ctx, dev)) return rc;
        drain.on = false;                                    // every stage has drained its own streams
    }
    fill_metadata(ctx);
    return AFG_OK;
}

}  // namespace

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

extern "C" {

namespace {
struct FlacParsedOwner {
    FlacRecords rec;
};
}  // namespace

int afg_flac_parse(const uint8_t *data, size_t length, afg_flac_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<FlacParsedOwner> own_guard(new (std::nothrow) FlacParsedOwner);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        FlacInfo fi;
        if (!flac_parse(data, length, fi, own->rec)) {
            own_guard.reset();
            afg::set_error("afg_flac_parse: not a native FLAC stream");
            return AFG_ERR_UNSUPPORTED;
        }
        out->sample_rate = fi.sample_rate;
        out->channels = fi.channels;
        out->bps = fi.bps;
        out->max_block = fi.max_block;
        out->total_samples = fi.total_samples;
        out->n_frames = own->rec.frames.size();
        out->n_subframes = own->rec.subframes.size();
        out->n_res = own->rec.res.size();
        out->out_samples = own->rec.out_samples;
        out->frames = own->rec.frames.data();
        out->subframes = own->rec.subframes.data();
        out->res = own->rec.res.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_flac_parsed_free(afg_flac_parsed *p)
{
    if (!p) return;
    delete (FlacParsedOwner *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_mp3_parse(const uint8_t *data, size_t length, afg_mp3_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_mp3::File> own_guard(new (std::nothrow) afg_mp3::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        if (!afg_mp3::parse_file(data, length, *own)) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse: no MPEG Layer III stream found");
            return AFG_ERR_UNSUPPORTED;
        }
        static_assert(sizeof(afg_mp3::Copy) == sizeof(afg_mp3_copy), "copy plan layout");
        out->channels = own->channels;
        out->hz = own->hz;
        out->tagged = own->tagged ? 1 : 0;
        out->start_delay = own->start_delay;
        out->detected_samples = own->detected_samples;
        out->declared_samples = own->declared_samples;
        out->pcm_samples = own->pcm_samples;
        out->n_runs = own->run_granules.size();
        out->n_blocks = own->blocks();
        out->n_copies = own->copies.size();
        out->run_granules = own->run_granules.data();
        out->coef = own->coef.data();
        out->flags = own->flags.data();
        out->copies = (afg_mp3_copy *)own->copies.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_mp3_parsed_free(afg_mp3_parsed *p)
{
    if (!p) return;
    delete (afg_mp3::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_mp3_parse_q(const uint8_t *data, size_t length, afg_mp3_parsed_q *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_mp3::File> own_guard(new (std::nothrow) afg_mp3::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        own->quantised = true;
        if (!afg_mp3::parse_file(data, length, *own)) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse_q: no MPEG Layer III stream found");
            return AFG_ERR_UNSUPPORTED;
        }
        if (own->q_unsupported) {
            own_guard.reset();
            afg::set_error("afg_mp3_parse_q: the stream holds granules the device requantiser does not cover (MPEG-2.5 8 kHz mixed blocks, or a mono frame with the intensity bit set)");
            return AFG_ERR_UNSUPPORTED;
        }
        afg_mp3_parsed &b = out->base;
        b.channels = own->channels;
        b.hz = own->hz;
        b.tagged = own->tagged ? 1 : 0;
        b.start_delay = own->start_delay;
        b.detected_samples = own->detected_samples;
        b.declared_samples = own->declared_samples;
        b.pcm_samples = own->pcm_samples;
        b.n_runs = own->run_granules.size();
        b.n_blocks = own->blocks();
        b.n_copies = own->copies.size();
        b.run_granules = own->run_granules.data();
        b.coef = nullptr;
        b.flags = own->flags.data();
        b.copies = (afg_mp3_copy *)own->copies.data();
        b.owner = own;                                  // (released from the guard at the end)
        out->n_granules = own->qgr.size();
        out->n_sdesc = own->sdesc.size();
        out->q = own->q.data();
        out->granules = own->qgr.data();
        out->sdesc = own->sdesc.data();
        own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_mp3_qtables(uint8_t band_of_line[24][576], uint16_t dst_of_src[24][576], float pow43[145])
{
    const afg_mp3::QTables &t = afg_mp3::qtables();
    if (band_of_line) std::memcpy(band_of_line, t.band_of_line, sizeof(t.band_of_line));
    if (dst_of_src) std::memcpy(dst_of_src, t.dst_of_src, sizeof(t.dst_of_src));
    if (pow43) std::memcpy(pow43, t.pow43, sizeof(t.pow43));
}

void afg_mp3_parsed_q_free(afg_mp3_parsed_q *p)
{
    if (!p) return;
    delete (afg_mp3::File *)p->base.owner;
    std::memset(p, 0, sizeof(*p));
}

static int vorbis_parse_any(const uint8_t *data, size_t length, afg_vorbis_parsed *out, bool device_floor)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_vorbis::File> own_guard(new (std::nothrow) afg_vorbis::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        if (!afg_vorbis::parse_file(data, length, *own, device_floor)) {
            own_guard.reset();
            afg::set_error("afg_vorbis_parse: not an Ogg Vorbis I stream");
            return AFG_ERR_UNSUPPORTED;
        }
        out->channels = own->channels;
        out->blocksize0 = own->blocksize0;
        out->blocksize1 = own->blocksize1;
        out->sample_rate = own->sample_rate;
        out->total_samples = own->total_samples;
        out->n_packets = own->pflags.size();
        out->spec_floats = own->spec.size();
        out->pcm_frames = own->pcm_frames;
        out->pflags = own->pflags.data();
        out->spec = own->spec.data();
        out->take_from = own->take_from.data();
        out->take_count = own->take_count.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

int afg_vorbis_parse(const uint8_t *data, size_t length, afg_vorbis_parsed *out) { return vorbis_parse_any(data, length, out, false); }

void afg_vorbis_parsed_free(afg_vorbis_parsed *p)
{
    if (!p) return;
    delete (afg_vorbis::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_vorbis_parse_r(const uint8_t *data, size_t length, afg_vorbis_parsed_r *out)
{
    if (!out) return AFG_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    if (int rc = vorbis_parse_any(data, length, &out->base, true)) return rc;
    afg_vorbis::File *own = (afg_vorbis::File *)out->base.owner;
    out->n_curves = own->fl_curves.size();
    out->n_points = own->fl_points.size() / 2;
    out->n_steps = own->fl_steps.size() / 2;
    out->packets = own->fl_packets.data();
    out->curves = own->fl_curves.data();
    out->points = own->fl_points.data();
    out->steps = own->fl_steps.data();
    return AFG_OK;
}

void afg_vorbis_parsed_r_free(afg_vorbis_parsed_r *p)
{
    if (!p) return;
    afg_vorbis_parsed_free(&p->base);
    std::memset(p, 0, sizeof(*p));
}

int afg_opus_parse(const uint8_t *data, size_t length, afg_opus_parsed *out)
{
    try {
        if (!out) return AFG_ERR_INVALID;
        std::memset(out, 0, sizeof(*out));
        if (!data) return AFG_ERR_INVALID;
        std::unique_ptr<afg_opus::File> own_guard(new (std::nothrow) afg_opus::File);               // (freed if the parser throws)
        auto *own = own_guard.get();
        if (!own) return AFG_ERR_OOM;
        const afg_opus::Status st = afg_opus::parse_file(data, length, *own);
        if (st != afg_opus::kOpened) {
            if (st == afg_opus::kUnsupported) {
                out->channels = own->channels;
                out->preskip = own->preskip;
                afg::set_error("afg_opus_parse: the stream holds SILK or hybrid packets (only CELT-only Opus is decoded)");
            } else {
                afg::set_error("afg_opus_parse: not an Ogg Opus stream");
            }
            own_guard.reset();
            return AFG_ERR_UNSUPPORTED;
        }
        out->channels = own->channels;
        out->preskip = own->preskip;
        out->gain_i = own->gain_i;
        out->error = own->error ? 1 : 0;
        out->gain = own->gain;
        out->declared_frames = own->declared_frames;
        out->pcm_frames = own->pcm_frames;
        out->n_frames = own->frames.size();
        out->n_coeffs = own->coeffs.size();
        out->frames = own->frames.data();
        out->coeffs = own->coeffs.data();
        out->owner = own_guard.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_opus_parsed_free(afg_opus_parsed *p)
{
    if (!p) return;
    delete (afg_opus::File *)p->owner;
    std::memset(p, 0, sizeof(*p));
}

int afg_qoa_parse(const uint8_t *data, size_t length, uint32_t *channels, uint32_t *samplerate, uint32_t *samples,
                  afg_qoa_frame *frames, size_t frame_cap, size_t *n_frames)
{
    if (!data) return AFG_ERR_INVALID;
    QoaInfo qi;
    std::vector<afg_qoa_frame> fr;
    if (!qoa_parse(data, length, qi, fr)) {
        afg::set_error("afg_qoa_parse: not a QOA file");
        return AFG_ERR_UNSUPPORTED;
    }
    if (channels) *channels = qi.channels;
    if (samplerate) *samplerate = qi.samplerate;
    if (samples) *samples = qi.samples;
    if (n_frames) *n_frames = fr.size();
    if (frames) std::memcpy(frames, fr.data(), std::min(frame_cap, fr.size()) * sizeof(afg_qoa_frame));
    return AFG_OK;
}

}  // extern "C"

namespace {

// The CPU time the process may actually use: a container's cgroup quota in CPUs (0: none / unknown).
double cpu_quota()
{
    static const double quota = [] {
        double q = 0;
        if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {                    // cgroup v2: "<quota|max> <period>"
            char w[32] = { 0 };
            double period = 0;
            if (std::fscanf(f, "%31s %lf", w, &period) == 2 && period > 0 && std::strcmp(w, "max") != 0) q = std::atof(w) / period;
            std::fclose(f);
        } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { // cgroup v1
            double us = -1, period = 100000;
            if (std::fscanf(g, "%lf", &us) != 1) us = -1;
            std::fclose(g);
            if (FILE *h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(h, "%lf", &period) != 1) period = 100000;
                std::fclose(h);
            }
            if (us > 0 && period > 0) q = us / period;
        }
        return q;
    }();
    return quota;
}

// Host threads of a batch when the caller leaves the choice to the library: one per physical core of an SMT-2 host (with one
// per logical CPU the parse stages ran up to 10x longer on a shared 256-CPU box: the stragglers wait for a CPU) -- and under a
// cgroup quota ONE AND A HALF times the quota's CPUs.  The GPU boxes of this project show 256 logical CPUs behind a 16-CPU
// quota.  What counts for back-to-back calls -- what a service does and what bench.py times -- is the CPU seconds a call
// costs, and threads the quota cannot run cost more of them (descheduled in the middle of a file, cold caches): round 6, 2048-file
// batches, CPU seconds per call with 16 / 24 / 32 / 64 threads: FLAC 0.27 / 0.28 / 0.31 / 0.37, Vorbis 1.09 / 1.16 / 1.24 / 1.39,
// and MP3 5.8e9 samples/s with 64 threads, 7.0e9 with 24 (tools/gpu_r06_e2e_threads.sh, gpu_r06_groups.sh).  Rounds 3-5 used four
// times the quota, sized on single calls that finish inside the burst the quota allows.
unsigned default_threads()
{
    static const unsigned n = [] {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        unsigned t = hw >= 16 ? hw / 2 : hw;
        const double quota = cpu_quota();
        if (quota > 0) t = std::min(t, std::max(1u, (unsigned)(1.5 * quota + 0.5)));
        return std::max(1u, t);
    }();
    return n;
}

// ... and for a stage that keeps every CPU busy for half a second by itself (the Opus range / PVQ decode of a 2048-file batch):
// twice the quota (1.7e9 samples/s with 128 threads, 2.3e9 with 32).
unsigned sustained_threads()
{
    static const unsigned n = [] {
        unsigned t = default_threads();
        const double quota = cpu_quota();
        if (quota > 0) t = std::min(t, std::max(1u, (unsigned)(2 * quota + 0.5)));
        return std::max(1u, t);
    }();
    return n;
}

// What a batch result owns: one BatchOut per device the batch ran on.
struct BatchOwner {
    std::vector<std::unique_ptr<BatchOut>> parts;
    std::deque<std::string> messages;                            // the item messages that are not static strings (afg_batch_decode_resampled)
};

// The whole batch path for the files handed in, on the calling thread's current device; fills items[0..n_files).
// `parse_done` (optional) is called once, when the host passes that keep every helper thread busy are over and what remains is
// the device stages of decode_parsed: a grouped batch lets its next group start parsing then.
int batch_decode_device(const uint8_t *const *data, const size_t *length, int n_files, int n_threads, afg_batch_item *items,
                        std::unique_ptr<BatchOut> &keep, const std::function<void()> *parse_done = nullptr, SampleOut so = SampleOut())
{
    // so (afg_batch_opts.sample_type, dither, dither_seed): every plane the items point into holds doubles or packed integer
    // samples, made on the device
    // Collate mode: nothing comes back.  Every stage scatters its chunks into so.d_out; what the files did not fill is written
    // as zero runs at the end, when every file's delivered length is known, and the items point at the slabs.  With
    // so.no_pad (afg_batch_decode_resampled: the tensor is a scratch whose reader knows every file's length) they are left out.
        const bool fetch = so.fetch();
        const size_t es = so.es();
    {
        if (int rc = afg::require_device()) return rc;
        int cur_dev = 0;
        AFG_HIP_CHECK(hipGetDevice(&cur_dev));
        StageTimer tm;
        struct ExitLap { StageTimer *t; const char *what; ~ExitLap() { t->lap(what); } } exit_lap{ &tm, "records released (call ends)" };
        std::vector<Parsed> parsed((size_t)n_files);
        tm.lap("call set-up");
        // default: one thread per physical core of an SMT-2 host (half the logical CPUs).  With one thread per logical
        // CPU the parse stages ran up to 10x longer on a shared 256-CPU box: the stragglers wait for a CPU.
        const unsigned nt = n_threads > 0 ? (unsigned)n_threads : default_threads();
        const unsigned nt_long = n_threads > 0 ? (unsigned)n_threads : sustained_threads();
        // pass 1: containers with a signature are parsed at once; MP3 candidates only get an upper bound of their
        // record count, so that pass 2 can parse them straight into one page-locked staging buffer
        std::vector<size_t> bound((size_t)n_files, 0), base((size_t)n_files, 0), ogg_bound((size_t)n_files, 0), ogg_base((size_t)n_files, 0),
            flac_bound((size_t)n_files, 0), flac_base((size_t)n_files, 0);
        std::vector<uint8_t> opus_open((size_t)n_files, 0);
        parallel_for((size_t)n_files, nt, [&](size_t i) {
            if (!data[i] || !length[i]) return;
            Parsed &p = parsed[i];
            try {
            if (length[i] >= 4 && std::memcmp(data[i], "OggS", 4) == 0) {                             // Opus is tried first (stream.d:1596)
                afg_opus::Reader rd;                                                                  // headers + sizes; decoded in pass 1c
                const afg_opus::Status st = rd.open(data[i], length[i], p.opus);
                if (st == afg_opus::kOpened) { opus_open[i] = 1; return; }
                p.opus = afg_opus::File();
                if (st == afg_opus::kUnsupported) { p.opus_mode = true; return; }
            }
            if ((flac_bound[i] = flac_res_bound(data[i], length[i])) != 0) return;                    // parsed in pass 1b
            p.flac.pack16 = flac_rows_int16();
            if (flac_parse(data[i], length[i], p.fi, p.flac)) { p.format = AFG_FORMAT_FLAC; return; }
            p.flac = FlacRecords();
            if (qoa_parse(data[i], length[i], p.qi, p.qoa)) { p.format = AFG_FORMAT_QOA; return; }
            if ((ogg_bound[i] = afg_vorbis::max_spec_floats(data[i], length[i])) != 0) return;       // parsed in pass 1b
            if (afg_mp3::looks_like_mp3(data[i], length[i])) bound[i] = afg_mp3::max_blocks(data[i], length[i]);
            } catch (...) { p = Parsed(); }
        });
        tm.lap("pass 1: flac / qoa parse, ogg + mp3 bounds");
        size_t total_bound = 0, ogg_total = 0, flac_total = 0;
        for (size_t i = 0; i < (size_t)n_files; i++) {
            base[i] = total_bound; total_bound += bound[i];
            ogg_base[i] = ogg_total; ogg_total += ogg_bound[i];
            flac_base[i] = flac_total; flac_total += (flac_bound[i] + 3) & ~(size_t)3;        // 16-byte aligned planes
        }
        // pass 1b: FLAC files of known length straight into one page-locked residual buffer
        StagingLease flac_lease;
        FlacStage flac_stage;
        if (flac_total) {
            if (int rc = staging_take(flac_total * sizeof(int32_t), flac_lease)) return rc;
            int32_t *res0 = (int32_t *)flac_lease.p;
            std::atomic<bool> lost{ false };
            parallel_for((size_t)n_files, nt, [&](size_t i) {
                if (!flac_bound[i]) return;
                Parsed &p = parsed[i];
                bool ok = false;
                try {
                    p.flac.pack16 = flac_rows_int16();
                    ok = flac_parse_into(data[i], length[i], p.fi, p.flac, res0 + flac_base[i], flac_bound[i]);
                    if (ok && p.flac.overflow) {                 // more audio than STREAMINFO declares: the file's own buffer
                        p.flac = FlacRecords();
                        p.flac.pack16 = flac_rows_int16();
                        ok = flac_parse(data[i], length[i], p.fi, p.flac);
                        lost = true;
                    }
                } catch (...) { ok = false; }
                if (ok) p.format = AFG_FORMAT_FLAC;
                else p.flac = FlacRecords();
            });
            // the staged layout is used only when every FLAC file of the batch is in it (a file of undeclared length
            // was parsed into its own buffer in pass 1): otherwise everything is gathered, wherever it sits
            bool all_staged = !lost;
            for (size_t i = 0; i < (size_t)n_files && all_staged; i++)
                if (parsed[i].format == AFG_FORMAT_FLAC && !parsed[i].flac.ext_res && parsed[i].flac.res_size()) all_staged = false;
            if (all_staged) { flac_stage.res = res0; flac_stage.words = flac_total; flac_stage.base = flac_base.data(); }
            tm.lap("pass 1b: flac parse into staging");
        }
        BatchOut *owner = new (std::nothrow) BatchOut;
        if (!owner) return AFG_ERR_OOM;
        std::unique_ptr<BatchOut> guard(owner);
        // ---- pass 1c: Ogg Opus, decoded by all helper threads and queued chunk by chunk (afg_opus_stage.cpp)
        std::vector<size_t> opus_pcm_at;
        bool opus_staged = false;
        if (int rc = opus_pipeline(parsed, data, length, opus_open, nt_long, so, owner->opus_plane, opus_pcm_at, &opus_staged, tm)) return rc;
        // The FLAC and QOA files are complete now: their device stage (mostly PCIe time) runs on a second host thread
        // while this one parses the MP3 and Ogg files.  Each call of decode_parsed only touches the files it owns.
        std::vector<uint8_t> own_early((size_t)n_files, 0), own_late((size_t)n_files, 1);
        size_t n_early = 0;
        for (size_t i = 0; i < (size_t)n_files; i++)
            if (parsed[i].format == AFG_FORMAT_FLAC || parsed[i].format == AFG_FORMAT_QOA) { own_early[i] = 1; own_late[i] = 0; n_early++; }
        struct EarlyJob {
            std::thread th;
            int rc = AFG_OK;
            std::string error;
            ~EarlyJob() { if (th.joinable()) th.join(); }
        } early_job;
        const bool split = n_early && (total_bound || ogg_total);
        if (split) {
            owner->early.reset(new BatchOut);
            BatchOut *eo = owner->early.get();
            const FlacStage *fs = flac_stage.words ? &flac_stage : nullptr;
            early_job.th = std::thread([&, eo, fs, cur_dev] {
                try {
                    // HIP's current device is per host thread and starts at 0: this thread works for the caller's device
                    if (hipSetDevice(cur_dev) != hipSuccess) { afg::set_error("hipSetDevice(%d) failed", cur_dev); early_job.rc = AFG_ERR_HIP; return; }
                    StageCtx early = stage_ctx(parsed, data, length, own_early.data(), 1 /* no helpers: they are parsing */, so, *eo);
                    FlacDecode early_flac;
                    early_flac.staged = fs;
                    Mp3Decode no_mp3;
                    VorbisDecode no_ogg;
                    OpusDecode no_opus;
                    early_job.rc = decode_parsed(early, early_flac, no_mp3, no_ogg, no_opus);
                } catch (...) {
                    afg::set_error("out of host memory");
                    early_job.rc = AFG_ERR_OOM;
                }
                if (early_job.rc) early_job.error = afg_last_error();
            });
        }
        StagingLease mp3_stage;
        Mp3Stage stage;
        Mp3Pipe pipe;
        bool fallback = false;
        if (total_bound) {
            // Quantised upload by default: int16 Huffman values + a record per granule, requantised on the device.
            // afg_dev_option("mp3_float_upload", 1) keeps the float spectra of round 1 (A/B of the bytes that cross the bus).
            const bool qmode = afg::dev_option(afg::kDevMp3FloatUpload) <= 0;
            const size_t per_block = qmode ? 576 * sizeof(int16_t) + sizeof(afg_mp3_qgranule) + sizeof(uint32_t)
                                           : 576 * sizeof(float) + sizeof(uint32_t);
            if (int rc = staging_take(total_bound * per_block + 64, mp3_stage)) return rc;
            if (fetch) if (int rc = staging_take(total_bound * 576 * es, owner->mp3_plane)) return rc;
            float *coef0 = nullptr;
            int16_t *q0 = nullptr;
            afg_mp3_qgranule *recs0 = nullptr;
            uint32_t *flags0 = nullptr;
            if (qmode) {
                recs0 = (afg_mp3_qgranule *)mp3_stage.p;                           // 8-byte aligned records first
                flags0 = (uint32_t *)(recs0 + total_bound);
                q0 = (int16_t *)(flags0 + total_bound);
                stage.q = q0; stage.recs = recs0;
            } else {
                coef0 = (float *)mp3_stage.p;
                flags0 = (uint32_t *)(coef0 + total_bound * 576);
                stage.coef = coef0;
            }
            stage.flags = flags0; stage.blocks = total_bound; stage.base = base.data();
            stage.plane = (float *)owner->mp3_plane.p;
            stage.so = so;
            if (int rc = pipe.open(stage)) return rc;
            tm.lap("mp3 pipeline set-up (device planes, streams, table arena)");
            // pass 2, chunk by chunk: all host threads parse a chunk of files, its device work is queued, and they go on
            // with the next chunk while the copies and the kernel of this one run
            size_t want = 8;
            if (afg::dev_option(afg::kDevMp3Chunks) > 0) want = (size_t)afg::dev_option(afg::kDevMp3Chunks);
            const size_t target = std::max<size_t>((total_bound + want - 1) / want, 8192);
            for (size_t f0 = 0; f0 < (size_t)n_files;) {
                const size_t f1 = cut_chunk(f0, (size_t)n_files, target, [&](size_t i, size_t &w) { w = bound[i]; return true; }).f1;
                std::atomic<bool> lost{ false };
                parallel_for(f1 - f0, nt, [&](size_t k) {
                    const size_t i = f0 + k;
                    if (!bound[i]) return;
                    Parsed &p = parsed[i];
                    bool ok = false;
                    try {
                        if (qmode) {
                            std::memset(recs0 + base[i], 0, bound[i] * sizeof(afg_mp3_qgranule));     // nch = 0: slot unused
                            p.mp3.quantised = true;
                            p.mp3.ext_q = q0 + base[i] * 576;
                            p.mp3.ext_qgr = recs0 + base[i];
                            ok = afg_mp3::parse_file_into(data[i], length[i], p.mp3, nullptr, flags0 + base[i], bound[i]);
                            if (ok && !p.mp3.overflow && !p.mp3.q_unsupported) {
                                const uint64_t shift = (uint64_t)base[i] * 576;                       // file-relative -> plane offsets
                                for (size_t k = 0; k < p.mp3.blocks(); k++)
                                    if (recs0[base[i] + k].nch) { recs0[base[i] + k].q_off += shift; recs0[base[i] + k].coef_off += shift; }
                            }
                        } else {
                            ok = afg_mp3::parse_file_into(data[i], length[i], p.mp3, coef0 + base[i] * 576, flags0 + base[i], bound[i]);
                        }
                        if (ok && (p.mp3.overflow || p.mp3.q_unsupported)) {
                            // overflow cannot happen; a stream the device requantiser does not cover (MPEG-2.5 8 kHz mixed
                            // blocks) can: either way the file is parsed into its own float buffers and the batch takes the
                            // gathered path
                            p.mp3 = afg_mp3::File();
                            ok = afg_mp3::parse_file(data[i], length[i], p.mp3);
                            lost = true;
                        }
                    } catch (...) {
                        // the file may have left records with file-relative offsets in the staged plane: the chunk must not
                        // be submitted as it stands (afg_mp3_requant_hip walks every slot with nch != 0)
                        ok = false;
                        if (qmode) std::memset(recs0 + base[i], 0, bound[i] * sizeof(afg_mp3_qgranule));
                        lost = true;
                    }
                    if (ok) p.format = AFG_FORMAT_MP3;
                    else p.mp3 = afg_mp3::File();
                });
                if (lost) fallback = true;
                if (!fallback) pipe.submit(parsed, f0, f1);
                f0 = f1;
            }
            if (fallback && qmode) {
                // the gathered path works from float records: the files that were parsed into the quantised staging are
                // parsed again into their own buffers (rare: one file of the batch is outside the requantiser's coverage)
                parallel_for((size_t)n_files, nt, [&](size_t i) {
                    if (!bound[i] || parsed[i].format != AFG_FORMAT_MP3 || !parsed[i].mp3.quantised) return;
                    Parsed &p = parsed[i];
                    bool ok = false;
                    try {
                        p.mp3 = afg_mp3::File();
                        ok = afg_mp3::parse_file(data[i], length[i], p.mp3);
                    } catch (...) { ok = false; }
                    if (!ok) { p.mp3 = afg_mp3::File(); p.format = AFG_FORMAT_UNKNOWN; }
                });
            }
            tm.lap("mp3 parse (all threads) | h2d | kernel | d2h");
        }
        // pass 1b: Ogg Vorbis files straight into one page-locked staging buffer (no per-file megabyte vectors to
        // fault in, gather and unmap) -- while the MP3 chunks queued above are still moving
        StagingLease ogg_lease;
        OggStage ogg_stage;
        if (ogg_total) {
            if (int rc = staging_take(ogg_total * sizeof(float), ogg_lease)) return rc;
            float *spec0 = (float *)ogg_lease.p;
            std::atomic<bool> lost{ false };
            parallel_for((size_t)n_files, nt, [&](size_t i) {
                if (!ogg_bound[i]) return;
                Parsed &p = parsed[i];
                bool ok = false;
                try {
                    ok = afg_vorbis::parse_file_into(data[i], length[i], p.ogg, spec0 + ogg_base[i], ogg_bound[i], vorbis_floor_on_device());
                    if (ok && p.ogg.overflow) {                  // cannot happen; be safe: the file's own buffer
                        ok = afg_vorbis::parse_file(data[i], length[i], p.ogg, vorbis_floor_on_device());
                        lost = true;
                    }
                } catch (...) { ok = false; }
                if (ok) p.format = AFG_FORMAT_OGG;
                else p.ogg = afg_vorbis::File();
            });
            if (!lost) { ogg_stage.spec = spec0; ogg_stage.floats = ogg_total; ogg_stage.base = ogg_base.data(); }
            tm.lap("pass 1b: ogg parse into staging");
        }
        if (total_bound) {
            const int prc = pipe.close();
            tm.lap("mp3 pipeline drain");
            if (prc) return prc;
            if (fallback) stage.blocks = 0;                   // decode_parsed does those files from their own buffers
        }
        if (parse_done) (*parse_done)();
        StageCtx late = stage_ctx(parsed, data, length, split ? own_late.data() : nullptr, nt, so, *owner);
        FlacDecode late_flac;
        if (!split && flac_stage.words) late_flac.staged = &flac_stage;
        Mp3Decode late_mp3;
        if (stage.blocks) late_mp3.staged = &stage;
        VorbisDecode late_ogg;
        if (ogg_stage.floats) late_ogg.staged = &ogg_stage;
        OpusDecode late_opus;
        if (opus_staged) late_opus.done_at = opus_pcm_at.data();
        int rc = decode_parsed(late, late_flac, late_mp3, late_ogg, late_opus);
        tm.lap("decode_parsed total");
        if (split) {
            early_job.th.join();
            tm.lap("flac / qoa thread joined");
            if (!rc && early_job.rc) { afg::set_error("%s", early_job.error.c_str()); rc = early_job.rc; }
        }
        if (rc) return rc;
        for (int i = 0; i < n_files; i++) {
            const BatchOut *src = (split && own_early[(size_t)i]) ? owner->early.get() : owner;
            const Decoded &d = src->files[(size_t)i];
            items[i].status = d.status;
            items[i].message = d.message;
            items[i].format = d.format;
            items[i].channels = d.channels;
            items[i].samplerate = d.samplerate;
            items[i].frames = d.frames;
            const uint8_t *plane = d.in_mp3_plane ? (const uint8_t *)owner->mp3_plane.p
                                   : d.in_opus_plane ? (const uint8_t *)owner->opus_plane.p : (const uint8_t *)src->plane.p;
            items[i].pcm = (d.status == AFG_OK && d.frames > 0 && fetch) ? (float *)(plane + d.pcm_off * es) : nullptr;
        }
        // MOD is probed last (stream.d:1796): files no other front-end took go to its stage
        std::vector<int> unknown;
        for (int i = 0; i < n_files; i++)
            if (items[i].status == AFG_ERR_UNSUPPORTED && items[i].message == kErrorUnknownFormat) unknown.push_back(i);
        // WAV comes well before either (stream.d:1638); no probe between it and them takes a file its scan accepts (QOA and
        // Ogg have their own magic, looks_like_mp3 declines RIFF), so its stage can run here, on the files nothing took
        if (int wrc = afg_wav::batch_stage(data, length, unknown, (int)nt, items, owner->wav_plane, so)) return wrc;
        tm.lap("wav stage");
        unknown.erase(std::remove_if(unknown.begin(), unknown.end(), [&](int i) { return items[i].status == AFG_OK || items[i].message != kErrorUnknownFormat; }), unknown.end());
        // ... and XM directly before it (stream.d:1751)
        if (int xrc = afg_xm::batch_stage(data, length, unknown, (int)nt, items, owner->xm_plane, so)) return xrc;
        tm.lap("xm stage");
        unknown.erase(std::remove_if(unknown.begin(), unknown.end(), [&](int i) { return items[i].status == AFG_OK || items[i].message != kErrorUnknownFormat; }), unknown.end());
        if (int mrc = afg_mod::batch_stage(data, length, unknown, (int)nt, items, owner->mod_plane, so)) return mrc;
        tm.lap("mod stage");
        if (so.collate()) {
            // Every stage has drained its streams.  The padding: tails, the rows a file has no channel for, and the whole slab
            // of a file that failed or starts past its end -- whatever a stage may have written there (an Opus file whose
            // last packet failed) is overwritten.
            std::vector<int64_t> frames((size_t)n_files, 0);
            std::vector<int> channels((size_t)n_files, 0);
            for (int i = 0; i < n_files; i++) {
                const bool ok = items[i].status == AFG_OK;
                if (ok) { frames[(size_t)i] = items[i].frames; channels[(size_t)i] = items[i].channels; }
                items[i].pcm = ok ? so.d_out + (size_t)i * so.C * so.T : nullptr;
            }
            if (!so.no_pad) {
                CollatePlane padding;
                if (int rc2 = padding.pad(so, frames, channels, nullptr)) return rc2;
                AFG_HIP_CHECK(hipStreamSynchronize(nullptr));
                tm.lap("collate padding");
            }
        }
        keep = std::move(guard);
        tm.lap("items filled");
        return AFG_OK;
    }
}

}  // namespace

namespace afg_front {
void parallel_run(size_t n, int n_threads, const std::function<void(size_t)> &fn)
{
    parallel_for(n, n_threads > 0 ? (unsigned)n_threads : default_threads(), fn);
}
}  // namespace afg_front

extern "C" {

int afg_set_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        afg::set_error("no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return AFG_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        afg::set_error("afg_set_device(%d): %d device(s) visible", device, n);
        return AFG_ERR_INVALID;
    }
    AFG_HIP_CHECK(hipSetDevice(device));
    return afg::require_device();
}

uint64_t afg_host_pool_trim(void) { return (uint64_t)g_staging.trim() + (uint64_t)g_devpool.trim(); }

int afg_get_device(void)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        afg::set_error("hipGetDevice failed: %s", hipGetErrorString(e));
        return e == hipErrorNoDevice ? AFG_ERR_NO_DEVICE : AFG_ERR_HIP;
    }
    return dev;
}

int afg_batch_decode_ex(const uint8_t *const *data, const size_t *length, int n_files, const afg_batch_opts *opts, afg_batch_result *out)
{
    try {
        if (!out || n_files < 0 || (n_files && (!data || !length))) return AFG_ERR_INVALID;
        out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        // (a caller built before sample_type was appended hands in the struct up to `devices`: it gets float, as it always did)
        if (opts && opts->struct_size < offsetof(afg_batch_opts, sample_type)) { afg::set_error("afg_batch_opts.struct_size too small"); return AFG_ERR_INVALID; }
        uint32_t sample_type = AFG_SAMPLE_F32;
        if (opts && opts->struct_size >= offsetof(afg_batch_opts, sample_type) + sizeof(uint32_t)) sample_type = opts->sample_type;
        if (sample_type > AFG_SAMPLE_PCM_S24) {
            afg::set_error("afg_batch_opts.sample_type %u: AFG_SAMPLE_F32 (0), AFG_SAMPLE_F64 (1) or AFG_SAMPLE_PCM_S8 / _S16 / _S24 (2 - 4)", sample_type);
            return AFG_ERR_INVALID;
        }
        // (dither and dither_seed were appended together: a struct that ends before dither_seed means no dither)
        int dither = AFG_DITHER_OFF;
        uint32_t dither_seed = 0;
        if (opts && opts->struct_size >= offsetof(afg_batch_opts, dither_seed) + sizeof(uint32_t)) { dither = opts->dither; dither_seed = opts->dither_seed; }
        if (dither == AFG_DITHER_LIBC) {
            afg::set_error("afg_batch_opts.dither: libc rand() dither has no defined draw order across files; use AFG_DITHER_LCG31 or AFG_DITHER_OFF");
            return AFG_ERR_INVALID;
        }
        if (dither != AFG_DITHER_OFF && dither != AFG_DITHER_LCG31) {
            afg::set_error("afg_batch_opts.dither %d: AFG_DITHER_OFF (0) or AFG_DITHER_LCG31 (2)", dither);
            return AFG_ERR_INVALID;
        }
        SampleOut so;
        so.type = sample_type;
        so.dither = so.pcm() && dither == AFG_DITHER_LCG31;       // (the float types never dither)
        so.seed = so.dither ? dither_seed : 0;
        if (n_files == 0) return AFG_OK;
        // ---- which devices ----
        std::vector<int> devs;
        const int want = opts ? opts->n_devices : 0;
        if (want != 0) {
            const int visible = afg_device_count();
            if (visible <= 0) { afg::set_error("no HIP device available; this library has no CPU fallback"); return AFG_ERR_NO_DEVICE; }
            if (want < 0) for (int d = 0; d < visible; d++) devs.push_back(d);
            else for (int k = 0; k < want; k++) {
                const int d = opts->devices ? opts->devices[k] : k;
                if (d < 0 || d >= visible) { afg::set_error("afg_batch_decode_ex: device %d of %d visible", d, visible); return AFG_ERR_INVALID; }
                devs.push_back(d);
            }
            if (devs.size() > 16) { afg::set_error("afg_batch_decode_ex: at most 16 devices"); return AFG_ERR_INVALID; }
        }
        const int n_threads = opts ? opts->n_threads : 0;
        auto owner = std::unique_ptr<BatchOwner>(new BatchOwner);
        afg_batch_item *items = (afg_batch_item *)std::calloc((size_t)n_files, sizeof(afg_batch_item));
        if (!items) return AFG_ERR_OOM;
        struct ItemsGuard { afg_batch_item *p; ~ItemsGuard() { std::free(p); } } items_guard{ items };
        if (devs.size() <= 1) {
            // one device: the caller's current one, or the one named
            int restore = -1;
            if (devs.size() == 1) {
                int cur = 0;
                AFG_HIP_CHECK(hipGetDevice(&cur));
                if (cur != devs[0]) { restore = cur; AFG_HIP_CHECK(hipSetDevice(devs[0])); }
            }
            // A large batch runs as a pipeline of GROUPS of files (round 6): while one group's device stages run -- the host mostly
            // waiting -- the next group is parsed.  Two host threads take the groups in turn; a token serialises their parse passes
            // (one set of helper threads at a time), handed on when a group reaches its device stages.  Results do not depend on
            // the grouping (files are independent).  afg_dev_option("batch_groups", n) forces n (1: off).
            size_t total_bytes = 0;
            for (int i = 0; i < n_files; i++) total_bytes += length[i];
            // By default only batches of (almost only) native FLAC and Ogg Vorbis files, from 512 files and 16 MB up, in 4 groups:
            // their calls are a parse pass followed by device stages; the MP3 and Opus paths overlap their parsing with their own
            // transfers already and lose 5-10 % to the split (2048-file batches, 24 helper threads, samples/s ungrouped -> 4 groups:
            // Vorbis 5.3e9 -> 6.2e9, FLAC 5.0e9 -> 5.7e9, MP3 6.5e9 -> 6.0e9, Opus 2.5e9 -> 2.3e9, mixed 4.9e9 -> 4.5e9).
            long groups = afg::dev_option(afg::kDevBatchGroups);
            if (groups <= 0) {
                groups = 1;
                if (n_files >= 512 && total_bytes >= ((size_t)16 << 20)) {
                    int staged = 0;
                    for (int i = 0; i < n_files; i++) {
                        const uint8_t *b = data[i];
                        const size_t n = length[i];
                        if (n >= 4 && !std::memcmp(b, "fLaC", 4)) staged++;
                        else if (n >= 28 && !std::memcmp(b, "OggS", 4) && n >= (size_t)27 + b[26] + 7 &&
                                 !std::memcmp(b + 27 + b[26], "\x01vorbis", 7)) staged++;      // (the first page's payload: the identification header)
                    }
                    if ((size_t)staged * 10 >= (size_t)n_files * 9) groups = 4;
                }
            }
            if (groups > n_files) groups = n_files;
            int rc = AFG_OK;
            if (groups <= 1) {
                owner->parts.emplace_back();
                rc = batch_decode_device(data, length, n_files, n_threads, items, owner->parts.back(), nullptr, so);
            } else {
                const size_t G = (size_t)groups;
                owner->parts.resize(G);
                std::vector<int> first(G + 1, n_files);          // contiguous ranges of about equal compressed size
                {
                    size_t acc = 0, g = 0;
                    first[0] = 0;
                    for (int i = 0; i < n_files && g + 1 < G; i++) {
                        acc += length[i];
                        if (acc * G >= total_bytes * (g + 1)) first[++g] = i + 1;
                    }
                }
                int dev = 0;
                AFG_HIP_CHECK(hipGetDevice(&dev));
                HelperPool *const helpers = tl_helpers;
                std::mutex token;
                std::atomic<bool> failed{ false };
                struct Job { int rc = AFG_OK; std::string error; } jobs[2];
                auto work = [&](int w) {
                    try {
                        if (w && hipSetDevice(dev) != hipSuccess) { jobs[w].rc = AFG_ERR_HIP; jobs[w].error = "hipSetDevice failed"; failed = true; return; }
                        tl_helpers = w ? &g_group_helpers[dev & 15] : helpers;
                        tl_stage_chunks = 2;
                        for (size_t g = (size_t)w; g < G && !failed; g += 2) {
                            const int f0 = first[g], f1 = first[g + 1];
                            if (f1 <= f0) continue;
                            std::unique_lock<std::mutex> lk(token);
                            bool released = false;
                            const std::function<void()> done = [&] { if (!released) { released = true; lk.unlock(); } };
                            const int r = batch_decode_device(data + f0, length + f0, f1 - f0, n_threads, items + f0, owner->parts[g], &done, so);
                            done();
                            if (r) { jobs[w].rc = r; jobs[w].error = afg_last_error(); failed = true; }
                        }
                    } catch (...) {
                        jobs[w].rc = AFG_ERR_OOM; jobs[w].error = "out of host memory"; failed = true;
                    }
                    tl_stage_chunks = 8;
                    tl_helpers = helpers;
                };
                {
                    struct Joiner { std::thread th; ~Joiner() { if (th.joinable()) th.join(); } } j;
                    j.th = std::thread(work, 1);
                    work(0);
                }
                for (const Job &jb : jobs)
                    if (jb.rc && !rc) { afg::set_error("%s", jb.error.c_str()); rc = jb.rc; }
            }
            if (restore >= 0) (void)hipSetDevice(restore);
            if (rc) return rc;
        } else {
            // Files are independent (stream.d:1363-1434 is all per-instance): the batch shards by file, longest file first
            // onto the least loaded device (compressed bytes stand for decode work), no exchange between devices.
            const size_t nd = devs.size();
            std::vector<size_t> order((size_t)n_files);
            for (size_t i = 0; i < order.size(); i++) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return length[a] > length[b]; });
            std::vector<std::vector<size_t>> mine(nd);
            std::vector<uint64_t> load(nd, 0);
            for (size_t f : order) {
                size_t best = 0;
                for (size_t k = 1; k < nd; k++) if (load[k] < load[best]) best = k;
                mine[best].push_back(f);
                load[best] += length[f] + 1;
            }
            for (auto &v : mine) std::sort(v.begin(), v.end());
            const unsigned total_threads = n_threads > 0 ? (unsigned)n_threads : default_threads();
            const int per_dev_threads = (int)std::max<unsigned>(1u, total_threads / (unsigned)nd);
            owner->parts.resize(nd);
            struct Part {
                std::vector<const uint8_t *> data;
                std::vector<size_t> len;
                std::vector<afg_batch_item> items;
                int rc = AFG_OK;
                std::string error;
            };
            std::vector<Part> parts(nd);
            int caller_dev = 0;
            AFG_HIP_CHECK(hipGetDevice(&caller_dev));
            auto run_part = [&](size_t k) {
                Part &p = parts[k];
                try {
                    for (size_t f : mine[k]) { p.data.push_back(data[f]); p.len.push_back(length[f]); }
                    p.items.assign(mine[k].size(), afg_batch_item{});
                    if (mine[k].empty()) return;
                    if (hipSetDevice(devs[k]) != hipSuccess) { p.rc = AFG_ERR_HIP; p.error = "hipSetDevice failed"; return; }
                    tl_helpers = &g_device_helpers[k];
                    p.rc = batch_decode_device(p.data.data(), p.len.data(), (int)mine[k].size(), per_dev_threads, p.items.data(), owner->parts[k], nullptr, so);
                    tl_helpers = nullptr;
                    if (p.rc) p.error = afg_last_error();
                } catch (...) {
                    tl_helpers = nullptr;
                    p.rc = AFG_ERR_OOM; p.error = "out of host memory";
                }
            };
            {
                // joins on every way out: a thread that cannot be created after others have started must not take the
                // process down (std::terminate on a joinable std::thread) instead of returning AFG_ERR_OOM
                struct Joiner {
                    std::vector<std::thread> th;
                    ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
                } j;
                j.th.reserve(nd);
                for (size_t k = 1; k < nd; k++) j.th.emplace_back(run_part, k);
                run_part(0);
            }
            (void)hipSetDevice(caller_dev);
            for (size_t k = 0; k < nd; k++)
                if (parts[k].rc) { afg::set_error("device %d: %s", devs[k], parts[k].error.c_str()); return parts[k].rc; }
            for (size_t k = 0; k < nd; k++)
                for (size_t j = 0; j < mine[k].size(); j++) items[mine[k][j]] = parts[k].items[j];
        }
        items_guard.p = nullptr;
        out->n_files = n_files;
        out->items = items;
        out->owner = owner.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

int afg_batch_decode(const uint8_t *const *data, const size_t *length, int n_files, int n_threads, afg_batch_result *out)
{
    afg_batch_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (uint32_t)sizeof(o);
    o.n_threads = n_threads;
    return afg_batch_decode_ex(data, length, n_files, &o, out);
}

int afg_batch_decode_to_device(const uint8_t *const *data, const size_t *length, int n_files, const afg_collate_opts *opts,
                               float *d_out, afg_batch_result *out)
{
    try {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (!opts || !d_out || !out) { afg::set_error("afg_batch_decode_to_device: NULL %s", !opts ? "opts" : !d_out ? "d_out" : "out"); return AFG_ERR_INVALID; }
        out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        if (opts->struct_size < offsetof(afg_collate_opts, first_frame) + sizeof(const int64_t *)) {
            afg::set_error("afg_collate_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        if (opts->channels == 0 || opts->frames == 0) {
            afg::set_error("afg_collate_opts: channels and frames must be at least 1 (%u, %u)", opts->channels, opts->frames);
            return AFG_ERR_INVALID;
        }
        if (n_files < 0 || (n_files && (!data || !length))) { afg::set_error("afg_batch_decode_to_device: n_files %d, or no file list", n_files); return AFG_ERR_INVALID; }
        for (int i = 0; i < n_files && opts->first_frame; i++)
            if (opts->first_frame[i] < 0) { afg::set_error("afg_collate_opts.first_frame[%d] is negative", i); return AFG_ERR_INVALID; }
        if (n_files == 0) return AFG_OK;
        if ((uint64_t)opts->channels * opts->frames > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
            afg::set_error("afg_batch_decode_to_device: a tensor of %d x %u x %u floats", n_files, opts->channels, opts->frames);
            return AFG_ERR_INVALID;
        }
        SampleOut so;
        so.type = afg_front::kSampleCollate;
        so.d_out = d_out;
        so.C = opts->channels;
        so.T = opts->frames;
        so.n_files = (uint64_t)n_files;
        so.first_frame = opts->first_frame;
        auto owner = std::unique_ptr<BatchOwner>(new BatchOwner);
        afg_batch_item *items = (afg_batch_item *)std::calloc((size_t)n_files, sizeof(afg_batch_item));
        if (!items) return AFG_ERR_OOM;
        struct ItemsGuard { afg_batch_item *p; ~ItemsGuard() { std::free(p); } } items_guard{ items };
        // one pass over the whole list on the current device: a slab's place follows from the file's index in it
        owner->parts.emplace_back();
        if (int rc = batch_decode_device(data, length, n_files, opts->n_threads, items, owner->parts.back(), nullptr, so)) return rc;
        items_guard.p = nullptr;
        out->n_files = n_files;
        out->items = items;
        out->owner = owner.release();
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

}  // extern "C"

namespace afg_front {

// What afg_batch_decode_resampled checks of its options behind struct_size, before any device call; fills in the job.
int resampled_check(const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files, ResampleJob &job)
{
    if (opts->channels == 0 || opts->frames == 0) {
        afg::set_error("afg_resample_opts: channels and frames must be at least 1 (%u, %u)", opts->channels, opts->frames);
        return AFG_ERR_INVALID;
    }
    constexpr uint32_t kMaxRate = 1u << 20;
    if (opts->samplerate == 0 || opts->samplerate > kMaxRate) {
        afg::set_error("afg_resample_opts.samplerate %u: 1 .. %u Hz", opts->samplerate, kMaxRate);
        return AFG_ERR_INVALID;
    }
    if (opts->mono > 1 || (opts->mono && opts->channels != 1)) {
        afg::set_error("afg_resample_opts.mono %u with %u channels: mono is 0 or 1, and a mono tensor has one channel", opts->mono, opts->channels);
        return AFG_ERR_INVALID;
    }
    if (opts->in_channels > 0xffff) { afg::set_error("afg_resample_opts.in_channels %u: at most 65535 (0 means 2)", opts->in_channels); return AFG_ERR_INVALID; }
    if (opts->max_in_rate > kMaxRate) { afg::set_error("afg_resample_opts.max_in_rate %u: at most %u Hz (0 means 48000)", opts->max_in_rate, kMaxRate); return AFG_ERR_INVALID; }
    if (opts->lowpass_width > 64) { afg::set_error("afg_resample_opts.lowpass_width %u: at most 64 (0 means 6)", opts->lowpass_width); return AFG_ERR_INVALID; }
    if (n_files < 0 || (n_files && (!data || !length))) { afg::set_error("afg_batch_decode_resampled: n_files %d, or no file list", n_files); return AFG_ERR_INVALID; }
    for (int i = 0; i < n_files && opts->first_frame; i++)
        if (opts->first_frame[i] < 0) { afg::set_error("afg_resample_opts.first_frame[%d] is negative", i); return AFG_ERR_INVALID; }
    job.C = opts->channels;
    job.T = opts->frames;
    job.samplerate = opts->samplerate;
    job.mono = opts->mono != 0;
    job.Z = opts->lowpass_width ? opts->lowpass_width : 6;
    job.in_channels = opts->in_channels ? opts->in_channels : 2;
    job.max_in_rate = opts->max_in_rate ? opts->max_in_rate : 48000;
    job.plan();
    if (job.T_s > 0xffffffffull) {
        afg::set_error("afg_batch_decode_resampled: %u frames at %u Hz from files of up to %u Hz: a scratch row of 2^32 floats or more", job.T,
                       job.samplerate, job.max_in_rate);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

// The resampled tensor of a checked call into d_out; items (n_files of them, zeroed) and messages as the entry returns them.
int resampled_run(const ResampleJob &job, const afg_resample_opts *opts, const uint8_t *const *data, const size_t *length, int n_files,
              float *d_out, afg_batch_item *items, std::deque<std::string> &messages)
{
    if ((uint64_t)opts->channels * opts->frames > (((uint64_t)1 << 62) / (uint64_t)n_files)) {
        afg::set_error("afg_batch_decode_resampled: a tensor of %d x %u x %u floats", n_files, opts->channels, opts->frames);
        return AFG_ERR_INVALID;
    }
    // the sublists: as many files as the scratch budget holds, one at the least
    const long budget_opt = afg::dev_option(afg::kDevResampleScratchBytes);
    const uint64_t budget = budget_opt > 0 ? (uint64_t)budget_opt : (uint64_t)2 << 30;
    const uint64_t slab_bytes = (uint64_t)job.R_s * job.T_s * sizeof(float);
    const size_t per_list = (size_t)std::min<uint64_t>((uint64_t)n_files, std::max<uint64_t>(budget / slab_bytes, 1));
    // scratch frame 0 of a file: H frames ahead of its first frame, as far as the file reaches
    std::vector<int64_t> frame0((size_t)n_files, 0);
    for (int i = 0; i < n_files && opts->first_frame; i++) frame0[(size_t)i] = std::max<int64_t>(opts->first_frame[i] - (int64_t)job.H, 0);
    if (int rc = afg::require_device()) return rc;
    afg_front::ResamplePlane plane;                           // (declared in front of the drain: it holds what the uploads read)
    afg_front::DevBuf scratch;
    struct Drain { ~Drain() { (void)hipStreamSynchronize(nullptr); } } drain;
    if (int rc = scratch.alloc((size_t)(per_list * slab_bytes))) return rc;
    SampleOut so;
    so.type = afg_front::kSampleCollate;
    so.d_out = (float *)scratch.p;
    so.C = job.R_s;
    so.T = (uint32_t)job.T_s;
    so.no_pad = true;
    for (size_t f0 = 0; f0 < (size_t)n_files; f0 += per_list) {
        const size_t n = std::min(per_list, (size_t)n_files - f0);
        so.n_files = n;
        so.first_frame = frame0.data() + f0;
        // the collate pass at the files' own rates: a slab's place follows from the file's index in the sublist.  It returns
        // with its streams drained; the items point at nothing it owns (messages are static), so its part is let go.
        std::unique_ptr<BatchOut> part;
        if (int rc = batch_decode_device(data + f0, length + f0, (int)n, opts->n_threads, items + f0, part, nullptr, so)) return rc;
        if (int rc = plane.launch(job, (const float *)scratch.p, items + f0, n, opts->first_frame ? opts->first_frame + f0 : nullptr,
                                  frame0.data() + f0, d_out + f0 * (size_t)job.C * job.T, messages, nullptr)) return rc;
        AFG_HIP_CHECK(hipStreamSynchronize(nullptr));         // the scratch and the records are free for the next sublist
    }
    return AFG_OK;
}

// items (malloc'ed, n_files of them) and the strings their messages point into become what afg_batch_free lets go
int batch_result_adopt(afg_batch_item *items, int n_files, std::deque<std::string> &messages, afg_batch_result *out)
{
    auto owner = std::unique_ptr<BatchOwner>(new BatchOwner);
    owner->messages.swap(messages);                              // (a deque's elements stay where they are)
    out->n_files = n_files;
    out->items = items;
    out->owner = owner.release();
    return AFG_OK;
}

}  // namespace afg_front

extern "C" {

int afg_batch_decode_resampled(const uint8_t *const *data, const size_t *length, int n_files, const afg_resample_opts *opts,
                               float *d_out, afg_batch_result *out)
{
    try {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (!opts || !d_out || !out) { afg::set_error("afg_batch_decode_resampled: NULL %s", !opts ? "opts" : !d_out ? "d_out" : "out"); return AFG_ERR_INVALID; }
        out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        if (opts->struct_size < offsetof(afg_resample_opts, lowpass_width) + sizeof(uint32_t)) {
            afg::set_error("afg_resample_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        afg_front::ResampleJob job;
        if (int rc = afg_front::resampled_check(opts, data, length, n_files, job)) return rc;
        if (n_files == 0) return AFG_OK;
        afg_batch_item *items = (afg_batch_item *)std::calloc((size_t)n_files, sizeof(afg_batch_item));
        if (!items) return AFG_ERR_OOM;
        struct ItemsGuard { afg_batch_item *p; ~ItemsGuard() { std::free(p); } } items_guard{ items };
        std::deque<std::string> messages;
        if (int rc = afg_front::resampled_run(job, opts, data, length, n_files, d_out, items, messages)) return rc;
        items_guard.p = nullptr;
        return afg_front::batch_result_adopt(items, n_files, messages, out);
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

void afg_batch_free(afg_batch_result *r)
{
    if (!r) return;
    StageTimer tm;
    std::free(r->items);
    delete (BatchOwner *)r->owner;
    r->items = nullptr; r->owner = nullptr; r->n_files = 0;
    tm.lap("afg_batch_free");
}

}  // extern "C"
