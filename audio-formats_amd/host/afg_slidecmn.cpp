// afg_slidecmn.cpp -- the host half of the sliding-window normalisation (include/afg.h; kernels in csrc/slidecmn.hip): the
// tile layout, the workspace size and the checks of slabs and parameters, which need no device; and
// afg_batch_decode_fbank_cmn -- afg_batch_decode_fbank, then one afg_slide_cmn_hip launch in place over every slab's own
// frames, with the records and the workspace in pooled buffers.
#include "afg_stage.h"
#include "../csrc/afg_common.h"

#include <algorithm>
#include <cstring>

namespace {

uint64_t tiles_of(const afg_cmn_slab &s)
{
    return ((uint64_t)s.n_frames + AFG_CMN_CHUNK - 1) / AFG_CMN_CHUNK;
}

int check_params(const afg_cmn_params *p)
{
    if (!p) { afg::set_error("afg_cmn_params: NULL"); return AFG_ERR_INVALID; }
    if (p->cmn_window < 1 || p->cmn_window > AFG_CMN_MAX_WINDOW) {
        afg::set_error("afg_cmn_params.cmn_window %u: 1 .. %u", p->cmn_window, (unsigned)AFG_CMN_MAX_WINDOW);
        return AFG_ERR_INVALID;
    }
    if (p->min_cmn_window < 1 || p->min_cmn_window > AFG_CMN_MAX_WINDOW) {
        afg::set_error("afg_cmn_params.min_cmn_window %u: 1 .. %u", p->min_cmn_window, (unsigned)AFG_CMN_MAX_WINDOW);
        return AFG_ERR_INVALID;
    }
    if (p->center > 1 || p->norm_vars > 1) {
        afg::set_error("afg_cmn_params: center %u and norm_vars %u must be 0 or 1", p->center, p->norm_vars);
        return AFG_ERR_INVALID;
    }
    if (p->cols < 1 || p->cols > AFG_CMN_MAX_COLS) {
        afg::set_error("afg_cmn_params.cols %u: 1 .. %u", p->cols, (unsigned)AFG_CMN_MAX_COLS);
        return AFG_ERR_INVALID;
    }
    if (p->layout > AFG_CMN_COL_MAJOR) {
        afg::set_error("afg_cmn_params.layout %u: AFG_CMN_FRAMES_MAJOR or AFG_CMN_COL_MAJOR", p->layout);
        return AFG_ERR_INVALID;
    }
    if (p->reserved[0] != 0 || p->reserved[1] != 0) { afg::set_error("afg_cmn_params.reserved: must be 0"); return AFG_ERR_INVALID; }
    return AFG_OK;
}

// One afg_slide_cmn_hip over `slabs`, in place on d_plane (plane_floats of it), with the records and the workspace in pooled
// buffers.  The object holds what its upload reads: it lives until `st` has drained.
struct CmnPlane {
    std::vector<afg_cmn_slab> recs;
    afg_front::DevBuf d_recs, d_work;
    int launch(const afg_cmn_params &prm, std::vector<afg_cmn_slab> &slabs, float *d_plane, uint64_t plane_floats, hipStream_t st)
    {
        recs.swap(slabs);
        if (recs.empty()) return AFG_OK;
        const uint64_t tiles = afg_cmn_layout(recs.data(), recs.size());
        if (tiles == 0) return AFG_OK;
        const uint64_t bytes = afg_cmn_work_bytes(tiles, prm.cols);
        if (int rc = d_work.alloc((size_t)bytes)) return rc;
        if (int rc = afg_front::upload_records(d_recs, recs, st)) return rc;
        return afg::slide_cmn_launch(recs.data(), recs.size(), (const afg_cmn_slab *)d_recs.p, tiles, &prm, d_plane, plane_floats, d_plane,
                                     plane_floats, d_work.p, bytes, st);
    }
};

}  // namespace

extern "C" uint64_t afg_cmn_layout(afg_cmn_slab *slabs, uint64_t n_slabs)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; slabs && k < n_slabs; k++) {
        slabs[k].first_tile = tiles;
        tiles += tiles_of(slabs[k]);
    }
    return tiles;
}

extern "C" uint64_t afg_cmn_work_bytes(uint64_t n_tiles, uint32_t cols)
{
    return n_tiles * cols * (uint64_t)(16 + 4 * AFG_CMN_CHUNK);  // (below 2^31 tiles and 2^10 columns behind the checks: no wrap)
}

extern "C" int afg_cmn_check_slabs(const afg_cmn_slab *slabs, uint64_t n_slabs, uint64_t n_tiles, const afg_cmn_params *params,
                                   uint64_t in_floats, uint64_t out_floats, int same_plane)
{
    try {
        if (int rc = check_params(params)) return rc;
        if (n_slabs == 0) return AFG_OK;
        if (!slabs) { afg::set_error("afg_cmn_check_slabs: NULL slabs"); return AFG_ERR_INVALID; }
        const bool col_major = params->layout == AFG_CMN_COL_MAJOR;
        std::vector<afg::Range> r;
        uint64_t tiles = 0;
        for (uint64_t k = 0; k < n_slabs; k++) {
            const afg_cmn_slab &s = slabs[k];
            const unsigned long long kk = (unsigned long long)k;
            if (s.reserved[0] != 0 || s.reserved[1] != 0 || s.reserved[2] != 0) {
                afg::set_error("afg_slide_cmn_hip: slab %llu: reserved must be 0", kk);
                return AFG_ERR_INVALID;
            }
            if (s.n_frames > 0x7fffffffu) { afg::set_error("afg_slide_cmn_hip: slab %llu: n_frames %u: at most 2^31 - 1", kk, s.n_frames); return AFG_ERR_INVALID; }
            if (s.first_tile != tiles) {
                afg::set_error("afg_slide_cmn_hip: slab %llu: first_tile %llu, afg_cmn_layout gives %llu", kk, (unsigned long long)s.first_tile,
                               (unsigned long long)tiles);
                return AFG_ERR_INVALID;
            }
            tiles += tiles_of(s);                                // below 2^26 a slab: no wrap before the launch's cap refuses
            if (tiles > ((uint64_t)1 << 62)) { afg::set_error("afg_slide_cmn_hip: slab %llu: too many tiles", kk); return AFG_ERR_INVALID; }
            if (s.n_frames == 0) continue;
            // rows of `len` floats, `pitch` apart: the frames, or with col-major the columns
            const uint64_t rows = col_major ? params->cols : s.n_frames, len = col_major ? s.n_frames : params->cols;
            if (rows > 1 && s.pitch < len) {
                afg::set_error("afg_slide_cmn_hip: slab %llu: pitch %llu below the %llu %s of a %s slab", kk, (unsigned long long)s.pitch,
                               (unsigned long long)len, col_major ? "frames" : "columns", col_major ? "col-major" : "frames-major");
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(s.in_off, rows, s.pitch, len, in_floats)) {
                afg::set_error("afg_slide_cmn_hip: slab %llu: it leaves the input (%llu floats)", kk, (unsigned long long)in_floats);
                return AFG_ERR_INVALID;
            }
            if (!afg::rows_inside(s.out_off, rows, s.pitch, len, out_floats)) {
                afg::set_error("afg_slide_cmn_hip: slab %llu: it leaves the output (%llu floats)", kk, (unsigned long long)out_floats);
                return AFG_ERR_INVALID;
            }
            const uint64_t span = (rows - 1) * s.pitch + len;    // (inside the planes: no wrap)
            r.push_back(afg::Range{ s.out_off, s.out_off + span, k, true });
            if (same_plane && s.in_off != s.out_off) r.push_back(afg::Range{ s.in_off, s.in_off + span, k, false });
        }
        if (tiles != n_tiles) {
            afg::set_error("afg_slide_cmn_hip: n_tiles %llu, afg_cmn_layout gives %llu", (unsigned long long)n_tiles, (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        uint64_t slab = 0, other = 0;
        if (afg::first_overlap(r, &slab, &other)) {
            afg::set_error("afg_slide_cmn_hip: slab %llu: it overlaps slab %llu without being in place", (unsigned long long)slab,
                           (unsigned long long)other);
            return AFG_ERR_INVALID;
        }
        return AFG_OK;
    } catch (...) {
        afg::set_error("out of host memory");
        return AFG_ERR_OOM;
    }
}

extern "C" int afg_batch_decode_fbank_cmn(const uint8_t *const *data, const size_t *length, int n_files, const afg_fbank_opts *opts,
                                          const afg_cmn_params *cmn, float *d_out, uint32_t *n_frames, afg_batch_result *out)
{
    return afg_front::tensor_entry([&]() -> int {
        // (all of this before any device call: it holds on a machine without a GPU too)
        if (int rc = afg_front::entry_args("afg_batch_decode_fbank_cmn", { { "opts", opts }, { "cmn", cmn }, { "d_out", d_out }, { "out", out } }, out)) return rc;
        if (opts->struct_size < sizeof(afg_fbank_opts)) {
            afg::set_error("afg_fbank_opts.struct_size too small");
            return AFG_ERR_INVALID;
        }
        const afg_fbank_opts &o = *opts;
        if (int rc = afg::fbank_check_params(&o.fbank, "afg_batch_decode_fbank_cmn")) return rc;   // cols and the layout come from them
        afg_cmn_params prm = *cmn;
        prm.cols = o.fbank.n_mels + (o.fbank.use_energy ? 1 : 0);
        prm.layout = o.fbank.layout == AFG_FBANK_MEL_MAJOR ? AFG_CMN_COL_MAJOR : AFG_CMN_FRAMES_MAJOR;
        if (int rc = check_params(&prm)) return rc;
        // the features and each file's own frames (every other check of the call is afg_batch_decode_fbank's)
        std::vector<uint32_t> own;
        if (!n_frames && n_files > 0) {
            own.resize((size_t)n_files);
            n_frames = own.data();
        }
        if (int rc = afg_batch_decode_fbank(data, length, n_files, opts, d_out, n_frames, out)) return rc;
        if (n_files == 0) return AFG_OK;
        const uint32_t n_out = o.n_out ? o.n_out : afg_fbank_frames(&o.fbank, o.frames);
        const uint64_t row_out = (uint64_t)prm.cols * n_out;
        std::vector<afg_cmn_slab> slabs;
        for (size_t i = 0; i < (size_t)n_files; i++)
            for (uint32_t k = 0; k < o.channels && n_frames[i] != 0; k++) {
                afg_cmn_slab s;
                std::memset(&s, 0, sizeof(s));
                s.in_off = s.out_off = (i * o.channels + k) * row_out;
                s.pitch = prm.layout == AFG_CMN_COL_MAJOR ? n_out : prm.cols;
                s.n_frames = n_frames[i];
                slabs.push_back(s);
            }
        CmnPlane plane;                                          // (declared in front of the drain: it holds what the upload reads)
        int rc;
        {
            afg_front::NullStreamDrain drain;
            rc = plane.launch(prm, slabs, d_out, (uint64_t)n_files * o.channels * row_out, nullptr);
            if (rc == AFG_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
                afg::set_error("afg_batch_decode_fbank_cmn: hipStreamSynchronize failed");
                rc = AFG_ERR_HIP;
            }
        }
        if (rc != AFG_OK) {                                      // the features stand, the normalisation does not: no result
            afg_batch_free(out);
            out->n_files = 0; out->items = nullptr; out->owner = nullptr;
        }
        return rc;
    });
}
