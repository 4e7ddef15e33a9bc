// cepstra.hip -- log-mel slabs to cepstral coefficients with their regression deltas (afg_cepstra_hip,
// afg_batch_decode_mfcc), for gfx950: a dense [n_ceps, n_mels] transform over the mel axis (a DCT-II with its lifter and
// scale folded in: afg_cep_dct), then the first and second time derivatives of ComputeDeltas(mode="replicate"), in one pass
// over the slab.  The definition -- every sum a chain of float32 fmaf in ascending index order from +0.0f, the differences
// and the final product rounded on their own -- is in include/afg.h; the Makefile builds this file with -ffp-contract=off
// like every other exact-mode kernel.  The host half (the table, the layout, the record checks, the batch entry) is
// host/afg_cepstra.cpp.
//
// One workgroup of 256 lanes (four wavefronts) per tile of 64 frames of one record (afg_cep_row), found by a search over the
// records' first tiles as melspec.hip does.  The work is small against the traffic (Whisper's slab with 13 coefficients and
// two delta planes: about 2 kFLOP for the 320 bytes read and 156 written per frame), so it runs on the vector unit and
// is laid out for the memory system:
//   lanes     run along frames: a load of x[m][t .. t + 63] is one contiguous 256-byte row, and so is every store
//   waves     split the coefficients in chunks of QB (4 while n_ceps <= 16, else 8); a wave's chunks are w, w + 4, ...  A
//             wave stages its chunk of the table in LDS as [m][QB] (rows past the table: +0.0f, their sums are not kept),
//             so that one ds_read_b128 -- every lane the same address: a broadcast -- brings the four entries of four
//             fmaf.  (Entries fetched one by one through the scalar cache cost eight scalar instructions per fmaf.)
//   statics   of the tile's frames and of a halo of H = delta_order * N frames on each side, clamped into [0, F): column j
//             of the wave's LDS rows is frame clamp(t0 - H + j).  The chain is in m order per output, so plain fmaf gives the
//             defined bits.  The slab is read once from memory; the other three waves find its lines in the L1
//   deltas    from LDS: d1 for the tile and a halo of N (when delta_order is 2) into a second LDS row, d2 from that.  Column
//             j of either row holds the value AT THE CLAMPED frame, so c[min(t + n, F - 1)] is the column of t + n and
//             nothing clamps twice.  No plane goes through memory a second time
// A short last tile of n frames computes n + 2 H columns only.  F = 1 and F below the halo need nothing special: every
// column clamps into the record.
//
// Bounds: every record is checked on the host before the launch (afg_cep_check_rows); the kernel relies on it.  It reads
// in[in_off + m * F + t] for m < n_mels and t < F only, dct[0 .. n_ceps * n_mels) only, and writes
// out[out_off + (p * n_ceps + q) * F + t] for p <= delta_order, q < n_ceps and t < F only.
#include "afg_records.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kTile = AFG_CEP_TILE;                         // frames per tile
constexpr uint32_t kMaxN = 8;
constexpr uint32_t kCols = kTile + 4 * kMaxN;                    // statics: the tile and 2 N on each side
constexpr uint32_t kDCols = kTile + 2 * kMaxN;                   // deltas: the tile and N on each side
static_assert(sizeof(afg_cep_params) == 32 && sizeof(afg_cep_row) == 32, "include/afg.h");

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int QB>
__global__ __launch_bounds__(kThreads) void cepstra_kernel(uint32_t n_rows, const afg_cep_row *__restrict__ rows, afg_cep_params prm, float g,
                                                           const float *__restrict__ in, const float *__restrict__ dct,
                                                           float *__restrict__ out)
{
    __shared__ float sh_c[kThreads / 64][QB][kCols];
    __shared__ float sh_d[kThreads / 64][QB][kDCols];
    extern __shared__ __attribute__((aligned(16))) float sh_t[];    // [waves][n_mels][QB]: every wave's chunk of the table
    const uint64_t tile = blockIdx.x;
    // the record of this tile: the last one whose first tile is <= tile (records without frames have no tiles)
    const uint32_t lo = afg::last_at_or_before(rows, n_rows, tile, &afg_cep_row::first_tile);
    const afg_cep_row r = rows[lo];
    if (r.first_tile > tile) return;
    const uint64_t first = (tile - r.first_tile) * kTile;        // first frame of the tile
    if (first >= r.frames) return;
    const uint32_t F = r.frames, t0 = (uint32_t)first;
    const uint32_t n = min(kTile, F - t0);
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n_mels = prm.n_mels, n_ceps = prm.n_ceps, order = prm.delta_order;
    const uint32_t N = order ? prm.delta_win : 0, H = order * N, H1 = order == 2 ? N : 0;
    const float *x = in + r.in_off;
    float *y = out + r.out_off;
    const int64_t last = (int64_t)F - 1;
    const uint32_t n_chunks = (n_ceps + QB - 1) / QB;
    float *const tw = sh_t + wave * (QB * n_mels);

    for (uint32_t c0 = 0; c0 < n_chunks; c0 += kThreads / 64) {  // (uniform over the workgroup: the barriers below)
        const uint32_t q0 = (c0 + wave) * QB;
        const bool active = q0 < n_ceps;
        if (active)
            for (uint32_t i = lane; i < QB * n_mels; i += 64) {
                const uint32_t k = i / n_mels, m = i - k * n_mels;
                tw[m * QB + k] = q0 + k < n_ceps ? dct[(q0 + k) * n_mels + m] : 0.0f;
            }
        __syncthreads();
        // ---- statics: column j is frame clamp(t0 - H + j)
        if (active) {
            for (uint32_t j = lane; j < n + 2 * H; j += 64) {
                const int64_t u = (int64_t)t0 - H + j;
                const uint64_t s = (uint64_t)(u < 0 ? 0 : u > last ? last : u);
                float acc[QB];
#pragma unroll
                for (int k = 0; k < QB; k++) acc[k] = 0.0f;
                const float *xs = x + s;
#pragma unroll 4
                for (uint32_t m = 0; m < n_mels; m++) {
                    const float v = xs[(uint64_t)m * F];
#pragma unroll
                    for (int k4 = 0; k4 < QB; k4 += 4) {
                        const f32x4 d = *(const f32x4 *)(tw + m * QB + k4);
                        acc[k4] = __builtin_fmaf(d.x, v, acc[k4]);
                        acc[k4 + 1] = __builtin_fmaf(d.y, v, acc[k4 + 1]);
                        acc[k4 + 2] = __builtin_fmaf(d.z, v, acc[k4 + 2]);
                        acc[k4 + 3] = __builtin_fmaf(d.w, v, acc[k4 + 3]);
                    }
                }
                const bool mine = j >= H && j < H + n;
#pragma unroll
                for (int k = 0; k < QB; k++) {
                    sh_c[wave][k][j] = acc[k];
                    if (mine && q0 + k < n_ceps) y[(uint64_t)(q0 + k) * F + (t0 + j - H)] = acc[k];
                }
            }
        }
        __syncthreads();
        // ---- deltas: column jd is frame clamp(t0 - H1 + jd); its statics' column is that frame's, js
        if (active && order >= 1) {
            for (uint32_t jd = lane; jd < n + 2 * H1; jd += 64) {
                const int64_t u = (int64_t)t0 - H1 + jd;
                const int64_t s = u < 0 ? 0 : u > last ? last : u;
                const uint32_t js = (uint32_t)(s - ((int64_t)t0 - H));   // in [N, n + 2 H - N)
                const bool mine = jd >= H1 && jd < H1 + n;
#pragma unroll
                for (int k = 0; k < QB; k++) {
                    float acc = 0.0f;
                    for (uint32_t d = 1; d <= N; d++) {
                        const float diff = sh_c[wave][k][js + d] - sh_c[wave][k][js - d];
                        acc = __builtin_fmaf((float)d, diff, acc);
                    }
                    const float v = acc * g;
                    sh_d[wave][k][jd] = v;
                    if (mine && q0 + k < n_ceps) y[((uint64_t)n_ceps + q0 + k) * F + (t0 + jd - H1)] = v;
                }
            }
        }
        __syncthreads();
        // ---- delta-deltas of the tile's frames, from the delta row
        if (active && order == 2 && lane < n) {
            const uint32_t js = lane + H1;
#pragma unroll
            for (int k = 0; k < QB; k++) {
                float acc = 0.0f;
                for (uint32_t d = 1; d <= N; d++) {
                    const float diff = sh_d[wave][k][js + d] - sh_d[wave][k][js - d];
                    acc = __builtin_fmaf((float)d, diff, acc);
                }
                const float v = acc * g;
                if (q0 + k < n_ceps) y[(2 * (uint64_t)n_ceps + q0 + k) * F + (t0 + lane)] = v;
            }
        }
        __syncthreads();                                         // the rows are free for the next chunk
    }
}

// what can be said without the records
int check_args(uint64_t n_rows, const afg_cep_row *d_rows, uint64_t n_tiles, const float *d_in, const float *d_dct, float *d_out)
{
    if (!d_rows || !d_dct || (n_tiles && (!d_in || !d_out))) {
        afg::set_error("afg_cepstra_hip: NULL device pointer");
        return AFG_ERR_INVALID;
    }
    if (((uintptr_t)d_in & 3u) != 0 || ((uintptr_t)d_dct & 3u) != 0 || ((uintptr_t)d_out & 3u) != 0 || ((uintptr_t)d_rows & 7u) != 0) {
        afg::set_error("afg_cepstra_hip: the planes must be 4-byte aligned, the records 8-byte aligned");
        return AFG_ERR_INVALID;
    }
    return afg::launch_caps("afg_cepstra_hip", "records", n_rows, n_tiles);
}

}  // namespace

int afg::cepstra_launch(const afg_cep_row *h_rows, uint64_t n_rows, const afg_cep_row *d_rows, uint64_t n_tiles, const afg_cep_params *params,
                        const float *d_in, uint64_t in_floats, const float *d_dct, uint64_t dct_floats, float *d_out, uint64_t out_floats,
                        hipStream_t stream)
{
    if (int rc = afg_cep_check_rows(nullptr, 0, 0, params, 0, 0, 0)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_dct, d_out)) return rc;
    if (int rc = afg_cep_check_rows(h_rows, n_rows, n_tiles, params, in_floats, dct_floats, out_floats)) return rc;
    if (n_tiles == 0) return AFG_OK;
    if (int rc = afg::require_device()) return rc;
    double sum = 0.0;
    for (uint32_t d = 1; d <= params->delta_win; d++) sum += (double)d * (double)d;
    const float g = params->delta_order ? (float)(1.0 / (2.0 * sum)) : 0.0f;
    // (the table chunks: at most 4 waves x 8 rows x 256 mels x 4 bytes = 32 KiB beside 22 KiB of static LDS)
    if (params->n_ceps <= 16)
        hipLaunchKernelGGL(cepstra_kernel<4>, dim3((uint32_t)n_tiles), dim3(kThreads), (size_t)kThreads / 64 * 4 * params->n_mels * sizeof(float), stream, (uint32_t)n_rows, d_rows, *params, g, d_in, d_dct,
                           d_out);
    else
        hipLaunchKernelGGL(cepstra_kernel<8>, dim3((uint32_t)n_tiles), dim3(kThreads), (size_t)kThreads / 64 * 8 * params->n_mels * sizeof(float), stream, (uint32_t)n_rows, d_rows, *params, g, d_in, d_dct,
                           d_out);
    AFG_HIP_CHECK(hipGetLastError());
    return AFG_OK;
}

extern "C" int afg_cepstra_hip(uint64_t n_rows, const afg_cep_row *d_rows, uint64_t n_tiles, const afg_cep_params *params, const float *d_in,
                               uint64_t in_floats, const float *d_dct, uint64_t dct_floats, float *d_out, uint64_t out_floats, void *hip_stream)
{
    if (int rc = afg_cep_check_rows(nullptr, 0, 0, params, 0, 0, 0)) return rc;
    if (n_rows == 0) return AFG_OK;
    if (int rc = check_args(n_rows, d_rows, n_tiles, d_in, d_dct, d_out)) return rc;
    if (int rc = afg::require_device()) return rc;
    return afg::with_host_records(d_rows, n_rows, (hipStream_t)hip_stream, [&](const afg_cep_row *h) {
        return afg::cepstra_launch(h, n_rows, d_rows, n_tiles, params, d_in, in_floats, d_dct, dct_floats, d_out, out_floats,
                                   (hipStream_t)hip_stream);
    });
}
