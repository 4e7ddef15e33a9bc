// afg_mp3_stage.cpp -- the MP3 stages (afg_batch.h): the batch path's staging pass (Mp3Staging), which parses chunks of
// files into one page-locked buffer and feeds the pipeline (Mp3Pipe) while it parses; the gathered stage of decode_parsed
// for files parsed into their own buffers (a stream's chunk with its carry, a batch that fell back), and the in-place
// delivery of what the pipeline decoded.
#include "afg_batch.h"

namespace afg_front {

// (with dither a sample's draws follow its index in the file, in collate mode its place does)
void mp3_runs(std::vector<PackRun> &runs, const afg_mp3::File &f, uint64_t base, size_t file)
{
    uint64_t at = 0;
    for (const afg_mp3::Copy &c : f.copies) { runs.push_back(PackRun{ base * 576 + c.src, c.count, at, (uint32_t)file, (uint32_t)f.channels }); at += c.count; }
}

int Mp3Pipe::open(const Mp3Staging &stage)
{
    st = &stage;
    const size_t coef_bytes = stage.blocks * 576 * sizeof(float), flag_bytes = (stage.blocks * 4 + 15) & ~(size_t)15;
    if (int r = d_in.alloc(coef_bytes + flag_bytes)) return r;
    if (int r = d_pcm.alloc(coef_bytes)) return r;
    if (stage.so.wide() && stage.so.fetch()) if (int r = d_pcm64.alloc(std::max<size_t>(stage.blocks * 576 * stage.es(), 16))) return r;
    if (stage.q) {
        const size_t q_bytes = (stage.blocks * 576 * sizeof(int16_t) + 15) & ~(size_t)15;
        const size_t rec_bytes = stage.blocks * sizeof(afg_mp3_qgranule);
        sdesc_cap = 4096;                            // intensity-stereo granules of the whole batch (grown on demand: rare)
        if (int r = d_qin.alloc(q_bytes + rec_bytes + sdesc_cap * sizeof(afg_mp3_sdesc))) return r;
        d_q = (int16_t *)d_qin.p;
        d_recs = (afg_mp3_qgranule *)((uint8_t *)d_qin.p + q_bytes);
        d_sdesc = (afg_mp3_sdesc *)((uint8_t *)d_recs + rec_bytes);
        if (int r = staging_take(sdesc_cap * sizeof(afg_mp3_sdesc), h_sdesc)) return r;
    }
    d_flags = (uint32_t *)((uint8_t *)d_in.p + coef_bytes);
    s.take();
    if (s.e != hipSuccess) { afg::set_error("hipStreamCreate failed: %s", hipGetErrorString(s.e)); return AFG_ERR_HIP; }
    const size_t tab_bytes = stage.blocks * 32 + 4096;
    if (int r = d_tables.alloc(tab_bytes)) return r;
    if (int r = staging_take(tab_bytes, h_tables)) return r;
    arena.host = (uint8_t *)h_tables.p; arena.dev = (uint8_t *)d_tables.p; arena.cap = tab_bytes; arena.stream = s.up;
    return AFG_OK;
}

void Mp3Pipe::submit(const std::vector<Parsed> &parsed, size_t f0, size_t f1)
{
    hipError_t &e = s.e;
    const hipStream_t up = s.up, down = s.down;
    if (rc || e != hipSuccess) return;
    std::vector<uint32_t> granules;
    std::vector<uint8_t> channels;
    std::vector<uint64_t> bases;
    size_t b0 = 0, b1 = 0;
    for (size_t i = f0; i < f1; i++) {
        const Parsed &p = parsed[i];
        if (p.format != AFG_FORMAT_MP3 || !p.mp3.blocks()) continue;
        if (granules.empty()) b0 = st->base[i];
        uint64_t at = st->base[i];
        for (uint32_t g : p.mp3.run_granules) {
            granules.push_back(g);
            channels.push_back((uint8_t)p.mp3.channels);
            bases.push_back(at);
            at += (uint64_t)g * (uint64_t)p.mp3.channels;
        }
        b1 = st->base[i] + p.mp3.blocks();
    }
    if (granules.empty()) return;
    afg_mp3_plan *plan = nullptr;
    rc = afg::mp3_plan_create_at(&plan, (uint32_t)granules.size(), granules.data(), channels.data(), bases.data(), 0, &arena);
    if (rc) return;
    plans.push_back(plan);
    const size_t nb = b1 - b0;
    if (st->q) {
        // quantised upload: 2 bytes per line + a record per granule, requantised on the device into the plane the
        // transform reads (afg_mp3_requant_hip); the stereo descriptors of intensity frames are gathered per chunk
        afg_mp3_qgranule *hrecs = st->recs;
        const size_t sd0 = sdesc_used;
        for (size_t i = f0; i < f1; i++) {
            const Parsed &p = parsed[i];
            if (p.format != AFG_FORMAT_MP3 || p.mp3.sdesc.empty()) continue;
            if (sdesc_used + p.mp3.sdesc.size() > sdesc_cap) { afg::set_error("MP3 stage: more than %zu intensity-stereo granules in one batch", sdesc_cap); rc = AFG_ERR_UNSUPPORTED; return; }
            std::memcpy((afg_mp3_sdesc *)h_sdesc.p + sdesc_used, p.mp3.sdesc.data(), p.mp3.sdesc.size() * sizeof(afg_mp3_sdesc));
            for (size_t k = st->base[i]; k < st->base[i] + p.mp3.blocks(); k++)
                if (hrecs[k].nch && hrecs[k].sdesc != AFG_MP3_NO_SDESC) hrecs[k].sdesc += (uint32_t)sdesc_used;
            sdesc_used += p.mp3.sdesc.size();
        }
        e = hipMemcpyAsync(d_q + b0 * 576, st->q + b0 * 576, nb * 576 * sizeof(int16_t), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync(d_recs + b0, st->recs + b0, nb * sizeof(afg_mp3_qgranule), hipMemcpyHostToDevice, up);
        if (e == hipSuccess && sdesc_used > sd0)
            e = hipMemcpyAsync(d_sdesc + sd0, (afg_mp3_sdesc *)h_sdesc.p + sd0, (sdesc_used - sd0) * sizeof(afg_mp3_sdesc), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync(d_flags + b0, st->flags + b0, nb * sizeof(uint32_t), hipMemcpyHostToDevice, up);
        if (e != hipSuccess) return;
        h2d_bytes += nb * (576 * sizeof(int16_t) + sizeof(afg_mp3_qgranule) + sizeof(uint32_t));
        rc = afg_mp3_requant_hip(nb, d_recs + b0, d_q, d_sdesc, (float *)d_in.p, up);
        if (rc) return;
    } else {
        e = hipMemcpyAsync((float *)d_in.p + b0 * 576, st->coef + b0 * 576, nb * 576 * sizeof(float), hipMemcpyHostToDevice, up);
        if (e == hipSuccess) e = hipMemcpyAsync(d_flags + b0, st->flags + b0, nb * sizeof(uint32_t), hipMemcpyHostToDevice, up);
        if (e != hipSuccess) return;
        h2d_bytes += nb * (576 * sizeof(float) + sizeof(uint32_t));
    }
    rc = afg_mp3_transform_hip(plan, (const float *)d_in.p, d_flags, (float *)d_pcm.p, nullptr, up);
    if (rc) return;
    if (st->so.wide()) {
        std::vector<PackRun> runs;
        for (size_t i = f0; i < f1 && st->so.runs(); i++)
            if (parsed[i].format == AFG_FORMAT_MP3 && parsed[i].mp3.blocks()) mp3_runs(runs, parsed[i].mp3, st->base[i], i);
        sort_runs(runs);
        rc = conv.launch(st->so, AFG_WAV_KIND_F32, d_pcm.p, 0, b0 * 576, nb * 576, d_pcm64.p, runs, up);
        if (rc) return;
    }
    const size_t es = st->es();
    s.chain(up, down);
    if (e == hipSuccess && st->so.fetch())
        e = hipMemcpyAsync((uint8_t *)st->plane + b0 * 576 * es, (const uint8_t *)(st->so.wide() ? d_pcm64.p : d_pcm.p) + b0 * 576 * es, nb * 576 * es, hipMemcpyDeviceToHost, down);
}

int Mp3Pipe::close()
{
    s.drain();
    for (afg_mp3_plan *p : plans) afg_mp3_plan_destroy(p);
    plans.clear();
    conv.clear();
    s.release();
    if (rc) return rc;
    if (s.e != hipSuccess) { afg::set_error("MP3 stage failed: %s", hipGetErrorString(s.e)); return AFG_ERR_HIP; }
    return AFG_OK;
}

// The staging buffer carved for the quantised or the float upload, the batch's MP3 result plane, and the pipeline opened.
int Mp3Staging::open(StagingLease &owner_plane, const SampleOut &out, StageTimer &tm)
{
    if (!total) return AFG_OK;
    // Quantised upload by default: int16 Huffman values + a record per granule, requantised on the device.
    // afg_dev_option("mp3_float_upload", 1) keeps the float spectra of round 1 (A/B of the bytes that cross the bus).
    const bool qmode = afg::dev_option(afg::kDevMp3FloatUpload) <= 0;
    const size_t per_block = qmode ? 576 * sizeof(int16_t) + sizeof(afg_mp3_qgranule) + sizeof(uint32_t)
                                   : 576 * sizeof(float) + sizeof(uint32_t);
    if (int rc = staging_take(total * per_block + 64, lease)) return rc;
    if (out.fetch()) if (int rc = staging_take(total * 576 * out.es(), owner_plane)) return rc;
    if (qmode) {
        recs = (afg_mp3_qgranule *)lease.p;                                    // 8-byte aligned records first
        flags = (uint32_t *)(recs + total);
        q = (int16_t *)(flags + total);
    } else {
        coef = (float *)lease.p;
        flags = (uint32_t *)(coef + total * 576);
    }
    blocks = total;
    plane = (float *)owner_plane.p;
    so = out;
    if (int rc = pipe.open(*this)) return rc;
    tm.lap("mp3 pipeline set-up (device planes, streams, table arena)");
    return AFG_OK;
}

// pass 2, chunk by chunk: all host threads parse a chunk of files, its device work is queued, and they go on
// with the next chunk while the copies and the kernel of this one run
void Mp3Staging::parse_and_submit(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm)
{
    if (!total) return;
    const size_t nf = parsed.size();
    const bool qmode = q != nullptr;
    size_t want = 8;
    if (afg::dev_option(afg::kDevMp3Chunks) > 0) want = (size_t)afg::dev_option(afg::kDevMp3Chunks);
    const size_t target = std::max<size_t>((total + want - 1) / want, 8192);
    for (size_t f0 = 0; f0 < nf;) {
        const size_t f1 = cut_chunk(f0, nf, target, [&](size_t i, size_t &w) { w = bounds[i]; return true; }).f1;
        std::atomic<bool> lost{ false };
        parallel_for(f1 - f0, nt, [&](size_t k) {
            const size_t i = f0 + k;
            if (!bounds[i]) return;
            Parsed &p = parsed[i];
            bool ok = false;
            try {
                if (qmode) {
                    std::memset(recs + base[i], 0, bounds[i] * sizeof(afg_mp3_qgranule));     // nch = 0: slot unused
                    p.mp3.quantised = true;
                    p.mp3.ext_q = q + base[i] * 576;
                    p.mp3.ext_qgr = recs + base[i];
                    ok = afg_mp3::parse_file_into(data[i], len[i], p.mp3, nullptr, flags + base[i], bounds[i]);
                    if (ok && !p.mp3.overflow && !p.mp3.q_unsupported) {
                        const uint64_t shift = (uint64_t)base[i] * 576;                       // file-relative -> plane offsets
                        for (size_t k = 0; k < p.mp3.blocks(); k++)
                            if (recs[base[i] + k].nch) { recs[base[i] + k].q_off += shift; recs[base[i] + k].coef_off += shift; }
                    }
                } else {
                    ok = afg_mp3::parse_file_into(data[i], len[i], p.mp3, coef + base[i] * 576, flags + base[i], bounds[i]);
                }
                if (ok && (p.mp3.overflow || p.mp3.q_unsupported)) {
                    // overflow cannot happen; a stream the device requantiser does not cover (MPEG-2.5 8 kHz mixed
                    // blocks) can: either way the file is parsed into its own float buffers and the batch takes the
                    // gathered path
                    p.mp3 = afg_mp3::File();
                    ok = afg_mp3::parse_file(data[i], len[i], p.mp3);
                    lost = true;
                }
            } catch (...) {
                // the file may have left records with file-relative offsets in the staged plane: the chunk must not
                // be submitted as it stands (afg_mp3_requant_hip walks every slot with nch != 0)
                ok = false;
                if (qmode) std::memset(recs + base[i], 0, bounds[i] * sizeof(afg_mp3_qgranule));
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
        parallel_for(nf, nt, [&](size_t i) {
            if (!bounds[i] || parsed[i].format != AFG_FORMAT_MP3 || !parsed[i].mp3.quantised) return;
            Parsed &p = parsed[i];
            bool ok = false;
            try {
                p.mp3 = afg_mp3::File();
                ok = afg_mp3::parse_file(data[i], len[i], p.mp3);
            } catch (...) { ok = false; }
            if (!ok) { p.mp3 = afg_mp3::File(); p.format = AFG_FORMAT_UNKNOWN; }
        });
    }
    tm.lap("mp3 parse (all threads) | h2d | kernel | d2h");
}

int Mp3Staging::close(StageTimer &tm)
{
    if (!total) return AFG_OK;
    const int rc = pipe.close();
    tm.lap("mp3 pipeline drain");
    if (rc) return rc;
    if (fallback) blocks = 0;                         // decode_parsed does those files from their own buffers
    return AFG_OK;
}

size_t Mp3Decode::layout(StageCtx &ctx, size_t off)
{
    const size_t nf = ctx.nf();
    plane_off = off;
    blk_base.assign(nf, 0);
    size_t out_floats = 0;
    for (size_t i = 0; i < nf; i++) {
        Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
        blk_base[i] = blocks;
        if (ctx.so.runs()) mp3_runs(runs, p.mp3, blocks, i);
        ctx.out.files[i].pcm_off = plane_off + out_floats;
        blocks += p.mp3.blocks();
        out_floats += (size_t)p.mp3.pcm_samples;
    }
    sort_runs(runs);
    if (!is_staged()) return out_floats;
    for (size_t i = 0; i < nf; i++) {
        Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
        const uint64_t first = p.mp3.copies.empty() ? 0 : p.mp3.copies[0].src;
        ctx.out.files[i].pcm_off = staged->base[i] * 576 + (size_t)first;
        ctx.out.files[i].in_mp3_plane = true;
    }
    return 0;
}

// a file whose copy plan is one piece (every undamaged file) is served where it landed; the pieces of a damaged file are
// closed up towards its first piece (ascending, so memmove order is safe)
void Mp3Decode::deliver_in_place(StageCtx &ctx)
{
    if (!is_staged() || !ctx.so.fetch()) return;
    const size_t es = ctx.so.es();
    std::vector<size_t> broken;                          // files whose pieces are not already back to back
    for (size_t i = 0; i < ctx.nf(); i++) {
        const Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
        for (size_t k = 1; k < p.mp3.copies.size(); k++)
            if (p.mp3.copies[k].src != p.mp3.copies[k - 1].src + p.mp3.copies[k - 1].count) { broken.push_back(i); break; }
    }
    parallel_for(broken.size(), ctx.threads, [&](size_t bi) {
        const size_t i = broken[bi];
        const Parsed &p = ctx.parsed[i];
        uint8_t *file_plane = (uint8_t *)staged->plane + staged->base[i] * 576 * es;
        uint8_t *dst = file_plane + p.mp3.copies[0].src * es;
        for (const afg_mp3::Copy &c : p.mp3.copies) {
            if (dst != file_plane + c.src * es) std::memmove(dst, file_plane + c.src * es, (size_t)c.count * es);
            dst += c.count * es;
        }
    });
    ctx.tm.lap("mp3 delivery (in place)");
}

// spectra of every decoded granule -> PCM plane -> the samples mp3dec_ex_read would deliver
int Mp3Decode::run(StageCtx &ctx, StageDev &dev)
{
    if (!blocks || is_staged()) return AFG_OK;
    std::vector<Parsed> &parsed = ctx.parsed;
    const SampleOut &so = ctx.so;
    const bool wide = so.wide(), fetch = so.fetch();
    const size_t nf = ctx.nf(), es = so.es();
    const size_t coef_bytes = blocks * 576 * sizeof(float), flag_bytes = (blocks * 4 + 15) & ~(size_t)15;
    DevBuf d_in, d_pcm;
    if (int rc = d_in.alloc(coef_bytes + flag_bytes)) return rc;
    if (int rc = d_pcm.alloc(coef_bytes)) return rc;
    if (wide && fetch) if (int rc = d_pcm64.alloc(std::max<size_t>(blocks * 576 * es, 16))) return rc;
    // The files are cut into a few chunks of similar size, each with its own plan: the upload and kernel of
    // chunk k+1 (stream `up`) run while chunk k's PCM goes back (stream `down`) -- PCIe is full duplex.
    struct Chunk { size_t f0, f1, blk0, blocks; afg_mp3_plan *plan; size_t runs; };
    struct Chunks {
        std::vector<Chunk> v;
        ~Chunks() { for (Chunk &c : v) if (c.plan) afg_mp3_plan_destroy(c.plan); }
    } chunks;
    {
        size_t want = 8;
        if (afg::dev_option(afg::kDevMp3Chunks) > 0) want = (size_t)afg::dev_option(afg::kDevMp3Chunks);
        const size_t target = std::max<size_t>((blocks + want - 1) / want, 8192);
        Chunk c{ 0, 0, 0, 0, nullptr, 0 };
        for (size_t i = 0; i < nf; i++) {
            if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
            if (c.blocks == 0) { c.f0 = i; c.blk0 = blk_base[i]; }
            c.blocks += parsed[i].mp3.blocks();
            c.f1 = i + 1;
            if (c.blocks >= target) { chunks.v.push_back(c); c = Chunk{ 0, 0, 0, 0, nullptr, 0 }; }
        }
        if (c.blocks) chunks.v.push_back(c);
    }
    StagingLease hfl_lease;                              // page-locked: the flag words travel asynchronously too
    if (int rc = staging_take(blocks * sizeof(uint32_t), hfl_lease)) return rc;
    uint32_t *hfl = (uint32_t *)hfl_lease.p;
    StageStreams s;
    hipError_t &e = s.e;
    s.take();
    const hipStream_t up = s.up, down = s.down;
    int rc = AFG_OK;
    for (Chunk &c : chunks.v) {                          // plans first: their tables are uploaded synchronously
        if (rc || e != hipSuccess) break;
        std::vector<uint32_t> granules;
        std::vector<uint8_t> channels;
        for (size_t i = c.f0; i < c.f1; i++) {
            const Parsed &p = parsed[i];
            if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
            for (uint32_t g : p.mp3.run_granules) {
                granules.push_back(g);
                channels.push_back((uint8_t)p.mp3.channels);
            }
            if (p.mp3.blocks()) std::memcpy(hfl + blk_base[i], p.mp3_flags(), p.mp3.blocks() * sizeof(uint32_t));
        }
        rc = afg_mp3_plan_create(&c.plan, (uint32_t)granules.size(), granules.data(), channels.data(), 0);
        c.runs = granules.size();
    }
    ctx.tm.lap("mp3 plans");
    uint32_t *d_flags = (uint32_t *)((uint8_t *)d_in.p + coef_bytes);
    for (Chunk &c : chunks.v) {
        if (rc || e != hipSuccess) break;
        for (size_t i = c.f0; i < c.f1 && e == hipSuccess; i++) {
            const Parsed &p = parsed[i];
            if (ctx.fmt_of(i) != AFG_FORMAT_MP3 || !p.mp3.blocks()) continue;
            // the batch path parsed this file straight into page-locked staging: one asynchronous copy per file
            // into the packed device plane (a file parsed on its own comes from ordinary memory)
            e = hipMemcpyAsync((float *)d_in.p + blk_base[i] * 576, p.mp3_coef(), p.mp3.blocks() * 576 * sizeof(float),
                               hipMemcpyHostToDevice, up);
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_flags + c.blk0, hfl + c.blk0, c.blocks * sizeof(uint32_t), hipMemcpyHostToDevice, up);
        if (e != hipSuccess) break;
        // chunked stream: one state blob per run of the chunk, zero (a fresh decoder) except the first when the chunk
        // goes on from the previous one; the last run's blob is what the next chunk goes on from
        DevBuf d_states;
        float *states = nullptr;
        if (carry && chunks.v.size() == 1 && c.runs) {
            const size_t sb = AFG_MP3_STATE_FLOATS * sizeof(float);
            if ((rc = d_states.alloc(c.runs * sb)) != AFG_OK) break;
            states = (float *)d_states.p;
            e = hipMemsetAsync(states, 0, c.runs * sb, up);
            // (a state left on another device -- the stream has moved -- is stale: the run starts fresh)
            if (e == hipSuccess && carry->continues && carry->valid && carry->state.here())
                e = hipMemcpyAsync(states, carry->state.p, sb, hipMemcpyDeviceToDevice, up);
            if (e != hipSuccess) break;
        }
        rc = afg_mp3_transform_hip(c.plan, (const float *)d_in.p + c.blk0 * 576, d_flags + c.blk0,
                                   (float *)d_pcm.p + c.blk0 * 576, states, up);
        if (rc) break;
        if (states) {
            const size_t sb = AFG_MP3_STATE_FLOATS * sizeof(float);
            carry->valid = false;
            if ((rc = carry->state.alloc(sb)) != AFG_OK) break;      // (kept from chunk to chunk; made again on a new device)
            e = hipMemcpyAsync(carry->state.p, states + (c.runs - 1) * AFG_MP3_STATE_FLOATS, sb, hipMemcpyDeviceToDevice, up);
            if (e == hipSuccess) e = hipStreamSynchronize(up);          // d_states goes out of scope below
            if (e != hipSuccess) break;
            carry->valid = true;
        }
        if (wide && (rc = dev.conv.launch(so, AFG_WAV_KIND_F32, d_pcm.p, 0, c.blk0 * 576, c.blocks * 576, d_pcm64.p, runs, up)) != AFG_OK) break;
        s.chain(up, down);
        // delivery: the copy plan of each file, merged into maximal contiguous pieces (one per undamaged file),
        // straight from the device PCM plane into the page-locked result plane
        for (size_t i = c.f0; i < c.f1 && e == hipSuccess && fetch; i++) {
            const Parsed &p = parsed[i];
            if (ctx.fmt_of(i) != AFG_FORMAT_MP3) continue;
            const uint8_t *src = (const uint8_t *)(wide ? d_pcm64.p : d_pcm.p) + blk_base[i] * 576 * es;
            uint8_t *dst = ctx.plane_at(ctx.out.files[i].pcm_off);
            const std::vector<afg_mp3::Copy> &cp = p.mp3.copies;
            for (size_t k = 0; k < cp.size() && e == hipSuccess;) {
                uint64_t from = cp[k].src, cnt = cp[k].count;
                size_t j = k + 1;
                while (j < cp.size() && cp[j].src == from + cnt) cnt += cp[j++].count;
                e = hipMemcpyAsync(dst, src + from * es, (size_t)cnt * es, hipMemcpyDeviceToHost, down);
                dst += cnt * es;
                k = j;
            }
        }
    }
    s.drain();
    s.release();
    ctx.tm.lap("mp3 h2d | kernel | d2h (chunks overlapped)");
    if (rc) return rc;
    if (e != hipSuccess) { afg::set_error("MP3 stage failed: %s", hipGetErrorString(e)); return AFG_ERR_HIP; }
    ctx.tm.lap("mp3 delivery copies");
    return AFG_OK;
}

}  // namespace afg_front
