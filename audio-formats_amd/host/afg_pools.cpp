// afg_pools.cpp -- what the library keeps between calls: pooled device memory, page-locked staging buffers, stream pairs and
// helper threads (declared in afg_stage.h and afg_batch.h), and the thread-count policy of a batch.
#include "afg_batch.h"

#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <thread>

using namespace afg_front;

// debugging aids, read ONCE when the library is loaded (set them before that): a trace of the host stages and the staging
// pool, and poisoned allocations (the test-suite runs with it: an output byte the library forgets to write shows up as NaN)
namespace afg_front {
const bool g_trace = std::getenv("AFG_TRACE") != nullptr;
}  // namespace afg_front

namespace {

static const bool g_poison_alloc = std::getenv("AFG_POISON_ALLOC") != nullptr;

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

// chunks a device stage cuts its files into (8; a group of a grouped batch -- afg_batch.cpp -- is itself a piece of a pipeline and takes 2).
// Per host thread: the second thread of a batch, which decodes the FLAC / QOA files, has always cut into 8.
thread_local unsigned tl_stage_chunks = 8;
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
void helpers_run(unsigned helpers, const std::function<void()> &work) { (tl_helpers ? *tl_helpers : g_helpers).run(helpers, work); }
unsigned stage_chunks() { return tl_stage_chunks; }

HelperScope::HelperScope(Kind kind, int index) : prev_pool(tl_helpers), prev_chunks(tl_stage_chunks)
{
    if (kind == kDevice) { tl_helpers = &g_device_helpers[index]; return; }
    if (kind == kGroup) tl_helpers = &g_group_helpers[index & 15];
    tl_stage_chunks = 2;
}
HelperScope::~HelperScope() { tl_helpers = (HelperPool *)prev_pool; tl_stage_chunks = prev_chunks; }

// The CPU time the process may actually use: a container's cgroup quota in CPUs (0: none / unknown).
static double cpu_quota()
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

void parallel_run(size_t n, int n_threads, const std::function<void(size_t)> &fn)
{
    parallel_for(n, n_threads > 0 ? (unsigned)n_threads : default_threads(), fn);
}

}  // namespace afg_front

extern "C" uint64_t afg_host_pool_trim(void) { return (uint64_t)g_staging.trim() + (uint64_t)g_devpool.trim(); }
