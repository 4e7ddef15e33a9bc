// afg_vorbis_stage.cpp -- the batch path's Ogg Vorbis staging pass and the Ogg Vorbis device stage of decode_parsed
// (afg_batch.h): chunk planning, the floor records of files parsed with the floor left to the device, the chunk pipeline,
// and the close-up of files delivered in pieces.
#include "afg_batch.h"

namespace afg_front {

bool vorbis_floor_on_device() { return afg::dev_option(afg::kDevVorbisHostFloor) <= 0; }

// pass 1b: Ogg Vorbis files straight into one page-locked staging buffer (no per-file megabyte vectors to fault in,
// gather and unmap)
int OggStaging::parse(std::vector<Parsed> &parsed, const uint8_t *const *data, const size_t *len, unsigned nt, StageTimer &tm)
{
    if (!total) return AFG_OK;
    if (int rc = staging_take(total * sizeof(float), lease)) return rc;
    float *spec0 = (float *)lease.p;
    std::atomic<bool> lost{ false };
    parallel_for(parsed.size(), nt, [&](size_t i) {
        if (!bounds[i]) return;
        Parsed &p = parsed[i];
        bool ok = false;
        try {
            ok = afg_vorbis::parse_file_into(data[i], len[i], p.ogg, spec0 + base[i], bounds[i], vorbis_floor_on_device());
            if (ok && p.ogg.overflow) {                  // cannot happen; be safe: the file's own buffer
                ok = afg_vorbis::parse_file(data[i], len[i], p.ogg, vorbis_floor_on_device());
                lost = true;
            }
        } catch (...) { ok = false; }
        if (ok) p.format = AFG_FORMAT_OGG;
        else p.ogg = afg_vorbis::File();
    });
    if (!lost) { spec = spec0; floats = total; }
    tm.lap("pass 1b: ogg parse into staging");
    return AFG_OK;
}

VorbisDecode::~VorbisDecode()
{
    for (Chunk &c : chunks) if (c.plan) afg_vorbis_plan_destroy(c.plan);
}

int VorbisDecode::layout(StageCtx &ctx, size_t off, size_t *floats)
{
    const size_t nf = ctx.nf();
    plane_off = off;
    *floats = 0;
    size_t total = 0;
    for (size_t i = 0; i < nf; i++)
        if (ctx.fmt_of(i) == AFG_FORMAT_OGG) { total += ctx.parsed[i].ogg.n_spec; packets += ctx.parsed[i].ogg.pflags.size(); }
    const size_t target = std::max<size_t>((total + ctx.chunks - 1) / ctx.chunks, (size_t)stage_chunk_samples((size_t)4 << 20));
    for (size_t f0 = 0; f0 < nf && packets;) {
        Chunk c;
        c.f0 = f0;
        c.f1 = f0 = cut_chunk(f0, nf, target, [&](size_t i, size_t &w) { return ctx.fmt_of(i) == AFG_FORMAT_OGG && ((w = ctx.parsed[i].ogg.n_spec), true); }).f1;
        if (int rc = plan_chunk(ctx, c, off)) return rc;
    }
    sort_runs(runs);
    *floats = out_floats;
    return AFG_OK;
}

// one plan for the chunk's files, and their delivery: the pull API's share of every packet's output
int VorbisDecode::plan_chunk(StageCtx &ctx, Chunk &c, size_t off)
{
    const bool ogg_staged = is_staged();
    c.spec0 = spec; c.out0 = out_floats;
    std::vector<uint32_t> npk;
    std::vector<uint8_t> chans, pflags;
    std::vector<uint16_t> b0, b1;
    std::vector<uint64_t> sbase;                     // staged: where each stream's spectra sit in the staging buffer
    c.spec_at.assign(c.f1 - c.f0, 0);
    size_t at = 0, span0 = 0, span1 = 0;
    for (size_t i = c.f0; i < c.f1; i++) {
        const Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_OGG) continue;
        c.spec_at[i - c.f0] = at;
        at += p.ogg.n_spec;
        if (p.ogg.pflags.empty()) continue;
        if (ogg_staged) {
            if (sbase.empty()) span0 = staged->base[i];
            span1 = staged->base[i] + p.ogg.n_spec;
            sbase.push_back(staged->base[i]);
        }
        npk.push_back((uint32_t)p.ogg.pflags.size());
        chans.push_back((uint8_t)p.ogg.channels);
        b0.push_back((uint16_t)p.ogg.blocksize0);
        b1.push_back((uint16_t)p.ogg.blocksize1);
        pflags.insert(pflags.end(), p.ogg.pflags.begin(), p.ogg.pflags.end());
    }
    if (npk.empty()) return AFG_OK;
    if (int rc = afg::vorbis_plan_create_at(&c.plan, (uint32_t)npk.size(), npk.data(), chans.data(), b0.data(), b1.data(),
                                            pflags.data(), ogg_staged ? sbase.data() : nullptr, 0))
        return rc;
    chunks.push_back(std::move(c));
    Chunk &k = chunks.back();
    k.spec_n = (size_t)afg_vorbis_plan_spec_floats(k.plan);
    k.out_n = (size_t)afg_vorbis_plan_out_floats(k.plan);
    if (ogg_staged) {                                // the plan addresses the staging layout: the chunk is a span of it
        if (k.spec_n != span1) {
            afg::set_error("Vorbis stage: spectrum layout mismatch (%zu vs %zu floats)", k.spec_n, span1);
            return AFG_ERR_INVALID;
        }
        k.spec0 = span0;
        k.spec_n = span1 - span0;
    } else if (k.spec_n != at) {
        afg::set_error("Vorbis stage: spectrum layout mismatch (%zu vs %zu floats)", k.spec_n, at);
        return AFG_ERR_INVALID;
    }
    std::vector<uint64_t> out_off(pflags.size());
    if (int rc = afg_vorbis_plan_offsets(k.plan, nullptr, out_off.data())) return rc;
    // delivery: normally one run from the first packet on
    size_t pk = 0;
    for (size_t i = k.f0; i < k.f1; i++) {
        const Parsed &p = ctx.parsed[i];
        if (ctx.fmt_of(i) != AFG_FORMAT_OGG) continue;
        const size_t n = p.ogg.pflags.size(), C = (size_t)p.ogg.channels;
        const size_t first_piece = pieces.size();
        for (size_t q = 0; q < n;) {
            if (p.ogg.take_count[q] <= 0) { q++; continue; }
            uint64_t from = out_off[pk + q] + (uint64_t)p.ogg.take_from[q] * C, cnt = (uint64_t)p.ogg.take_count[q] * C;
            size_t j = q + 1;
            while (j < n && p.ogg.take_count[j] > 0 && out_off[pk + j] + (uint64_t)p.ogg.take_from[j] * C == from + cnt)
                cnt += (uint64_t)p.ogg.take_count[j++] * C;
            pieces.push_back(Piece{ i, out_floats + from, cnt });
            q = j;
        }
        if (ctx.so.runs()) {
            uint64_t s0 = 0;
            for (size_t q = first_piece; q < pieces.size(); q++) { runs.push_back(PackRun{ pieces[q].from, pieces[q].count, s0, (uint32_t)i, (uint32_t)p.ogg.channels }); s0 += pieces[q].count; }
        }
        ctx.out.files[i].pcm_off = off + (pieces.size() > first_piece ? (size_t)pieces[first_piece].from : out_floats);
        if (pieces.size() - first_piece > 1) broken.push_back(i);
        else if (pieces.size() > first_piece) pieces.pop_back();          // one run: nothing to move
        pk += n;
    }
    if (!ogg_staged) spec += k.spec_n;
    out_floats += k.out_n;
    return AFG_OK;
}

namespace {
// Files parsed with the floor left to the device: their packets' coupling / floor records go up with the
// chunk (one page-locked block: packets, curves, points, steps of chunk after chunk) and afg_vorbis_floor_hip turns the
// residue vectors into spectra in place, in front of the transform.
struct FloorRecords {
    std::vector<size_t> pk, cv, pt, st;              // per file: the index of its first packet, curve, point and step
    size_t pk_bytes = 0, cv_bytes = 0, pt_bytes = 0, st_bytes = 0;
    StagingLease host;
    DevBuf dev;
    int alloc(const StageCtx &ctx)
    {
        const size_t nf = ctx.nf();
        pk.assign(nf + 1, 0); cv.assign(nf + 1, 0); pt.assign(nf + 1, 0); st.assign(nf + 1, 0);
        for (size_t i = 0; i < nf; i++) {
            const bool on = ctx.fmt_of(i) == AFG_FORMAT_OGG && ctx.parsed[i].ogg.device_floor;
            const afg_vorbis::File &f = ctx.parsed[i].ogg;
            pk[i + 1] = pk[i] + (on ? f.fl_packets.size() : 0);
            cv[i + 1] = cv[i] + (on ? f.fl_curves.size() : 0);
            pt[i + 1] = pt[i] + (on ? f.fl_points.size() / 2 : 0);
            st[i + 1] = st[i] + (on ? f.fl_steps.size() / 2 : 0);
        }
        pk_bytes = pk[nf] * sizeof(afg_vorbis_floor_packet); cv_bytes = cv[nf] * sizeof(afg_vorbis_floor_curve);
        pt_bytes = pt[nf] * 8; st_bytes = st[nf] * 2;
        if (!pk[nf]) return AFG_OK;
        if (int rc = staging_take(pk_bytes + cv_bytes + pt_bytes + st_bytes, host)) return rc;
        return dev.alloc(pk_bytes + cv_bytes + pt_bytes + st_bytes);
    }
    uint8_t *at(void *base0, int which, size_t index) const   // 0 packets, 1 curves, 2 points, 3 steps
    {
        uint8_t *b = (uint8_t *)base0;
        if (which == 0) return b + index * sizeof(afg_vorbis_floor_packet);
        if (which == 1) return b + pk_bytes + index * sizeof(afg_vorbis_floor_curve);
        if (which == 2) return b + pk_bytes + cv_bytes + index * 8;
        return b + pk_bytes + cv_bytes + pt_bytes + index * 2;
    }
    // file i of chunk [f0, ...): chunk-local indices (the kernel gets the chunk's slices), absolute spectrum offsets
    void gather(const afg_vorbis::File &f, size_t i, size_t f0, size_t spec_base) const
    {
        if (pk[i + 1] == pk[i]) return;
        afg_vorbis_floor_packet *hp = (afg_vorbis_floor_packet *)at(host.p, 0, pk[i]);
        for (size_t q = 0; q < f.fl_packets.size(); q++) {
            afg_vorbis_floor_packet r = f.fl_packets[q];
            r.spec_off += spec_base;
            r.curve_index += (uint32_t)(cv[i] - cv[f0]);
            r.step_off += (uint32_t)(st[i] - st[f0]);
            hp[q] = r;
        }
        afg_vorbis_floor_curve *hc = (afg_vorbis_floor_curve *)at(host.p, 1, cv[i]);
        for (size_t q = 0; q < f.fl_curves.size(); q++) {
            afg_vorbis_floor_curve r = f.fl_curves[q];
            r.point_off += (uint32_t)(pt[i] - pt[f0]);
            hc[q] = r;
        }
        if (!f.fl_points.empty()) std::memcpy(at(host.p, 2, pt[i]), f.fl_points.data(), f.fl_points.size() * sizeof(int32_t));
        if (!f.fl_steps.empty()) std::memcpy(at(host.p, 3, st[i]), f.fl_steps.data(), f.fl_steps.size());
    }
    // the records of files [f0, f1) go up on `up`, and the floor kernel runs over them
    int launch(size_t f0, size_t f1, float *d_spec, hipStream_t up, hipError_t &e) const
    {
        const struct { int which; size_t i0, i1, unit; } part[4] = {
            { 0, pk[f0], pk[f1], sizeof(afg_vorbis_floor_packet) }, { 1, cv[f0], cv[f1], sizeof(afg_vorbis_floor_curve) },
            { 2, pt[f0], pt[f1], 8 }, { 3, st[f0], st[f1], 2 } };
        for (const auto &p : part) {
            if (p.i1 == p.i0 || e != hipSuccess) continue;
            e = hipMemcpyAsync(at(dev.p, p.which, p.i0), at(host.p, p.which, p.i0), (p.i1 - p.i0) * p.unit, hipMemcpyHostToDevice, up);
        }
        if (e != hipSuccess) return AFG_OK;
        return afg_vorbis_floor_hip(pk[f1] - pk[f0], (const afg_vorbis_floor_packet *)at(dev.p, 0, pk[f0]),
                                    (const afg_vorbis_floor_curve *)at(dev.p, 1, cv[f0]), (const int32_t *)at(dev.p, 2, pt[f0]),
                                    (const uint8_t *)at(dev.p, 3, st[f0]), d_spec, up);
    }
};
}  // namespace

// per chunk: gather (host threads) -> upload + kernels on `up` -> download on `down`
int VorbisDecode::run(StageCtx &ctx, StageDev &dev)
{
    if (chunks.empty()) return AFG_OK;
    std::vector<Parsed> &parsed = ctx.parsed;
    const SampleOut &so = ctx.so;
    const bool wide = so.wide(), fetch = so.fetch(), ogg_staged = is_staged();
    const size_t es = so.es();
    StagingLease h_spec;
    DevBuf d_spec, d_pcm;
    if (wide && fetch) if (int rc = d_pcm64.alloc(std::max<size_t>(out_floats * es, 16))) return rc;
    if (!ogg_staged)
        if (int rc = staging_take(spec * sizeof(float), h_spec)) return rc;
    if (int rc = d_spec.alloc((ogg_staged ? staged->floats : spec) * sizeof(float))) return rc;
    if (int rc = d_pcm.alloc(out_floats * sizeof(float))) return rc;
    uint8_t *ogg_plane = ctx.plane_at(plane_off);
    FloorRecords fl;
    StageStreams s;
    hipError_t &e = s.e;
    s.take();
    const hipStream_t up = s.up, down = s.down;
    int rc = AFG_OK;
    if (int rc2 = fl.alloc(ctx)) return rc2;
    for (Chunk &c : chunks) {
        if (rc || e != hipSuccess) break;
        const float *hs = ogg_staged ? staged->spec + c.spec0 : (const float *)h_spec.p + c.spec0;
        const size_t npk_c = fl.pk[c.f1] - fl.pk[c.f0];
        if (npk_c) {
            parallel_for(c.f1 - c.f0, ctx.threads, [&](size_t k) {
                fl.gather(parsed[c.f0 + k].ogg, c.f0 + k, c.f0, ogg_staged ? staged->base[c.f0 + k] : c.spec0 + c.spec_at[k]);
            });
        }
        if (!ogg_staged) {
            float *hw = (float *)h_spec.p + c.spec0;
            parallel_for(c.f1 - c.f0, ctx.threads, [&](size_t k) {
                Parsed &p = parsed[c.f0 + k];
                if (ctx.fmt_of(c.f0 + k) != AFG_FORMAT_OGG || !p.ogg.n_spec) return;
                std::memcpy(hw + c.spec_at[k], p.ogg.spectra(), p.ogg.n_spec * sizeof(float));
                std::vector<float>().swap(p.ogg.spec);         // the big one: released here, by many threads
            });
        }
        e = hipMemcpyAsync((float *)d_spec.p + c.spec0, hs, c.spec_n * sizeof(float), hipMemcpyHostToDevice, up);
        if (e != hipSuccess) break;
        if (npk_c) {
            rc = fl.launch(c.f0, c.f1, (float *)d_spec.p, up, e);
            if (rc || e != hipSuccess) break;
        }
        // a staged plan addresses the staging layout from float 0; a gathered one is packed from its chunk's start
        rc = afg_vorbis_transform_hip(c.plan, (const float *)d_spec.p + (ogg_staged ? 0 : c.spec0), (float *)d_pcm.p + c.out0, up);
        if (rc) break;
        if (wide && (rc = dev.conv.launch(so, AFG_WAV_KIND_F32, d_pcm.p, 0, c.out0, c.out_n, d_pcm64.p, runs, up)) != AFG_OK) break;
        s.chain(up, down);
        if (e == hipSuccess && fetch)
            e = hipMemcpyAsync(ogg_plane + c.out0 * es, (const uint8_t *)(wide ? d_pcm64.p : d_pcm.p) + c.out0 * es, c.out_n * es, hipMemcpyDeviceToHost, down);
    }
    s.drain();
    s.release();
    if (rc) return rc;
    if (e != hipSuccess) { afg::set_error("Vorbis stage failed: %s", hipGetErrorString(e)); return AFG_ERR_HIP; }
    // files delivered as several runs (seek-style trims, damaged streams): close the runs up, in place
    for (size_t bi = 0, at = 0; bi < broken.size() && fetch; bi++) {
        const size_t i = broken[bi];
        while (at < pieces.size() && pieces[at].file != i) at++;
        uint8_t *dst = ctx.plane_at(ctx.out.files[i].pcm_off);
        for (; at < pieces.size() && pieces[at].file == i; at++) {
            const uint8_t *src = ogg_plane + pieces[at].from * es;
            if (dst != src) std::memmove(dst, src, (size_t)pieces[at].count * es);
            dst += pieces[at].count * es;
        }
    }
    ctx.tm.lap("vorbis gather | h2d | kernel | d2h (chunks overlapped)");
    return AFG_OK;
}

}  // namespace afg_front
