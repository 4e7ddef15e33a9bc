// afg_common.h -- shared plumbing of the C-ABI library (host side).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/afg.h"

namespace afg {

// thread-local detail string behind afg_last_error()
void set_error(const char *fmt, ...);

// Verifies a gfx950 device is present and selected; loud failure otherwise.
int require_device();

// Per-device state of the library (table copies, side streams, work counters) lives in arrays of this many slots --
// 8 MI355X in CPX partition mode show up as 64 devices.  device_slot() returns the calling thread's current device
// in *dev, or AFG_ERR_INVALID with a message naming the cap when its index does not fit.
#define AFG_MAX_DEVICES 64
int device_slot(int *dev, const char *who);

// Numeric mode of the float transform stages (afg_set_numeric_mode; env AFG_NUMERIC=exact|tolerance until it is called).
int numeric_mode();

// Alternative code paths the test-suite runs side by side with the default ones (afg.h: afg_dev_option).  Set through
// that call only -- the library reads no environment variable for them -- and -1 while unset.
enum DevOption { kDevCeltPath, kDevCeltDeSeq, kDevCeltDeDuo, kDevCeltSegRecs, kDevCeltWholeFrames, kDevVorbisSingle,
                 kDevMp3Chunks, kDevMp3FloatUpload, kDevVorbisHostFloor, kDevFlacHostRes32, kDevVorbisSegPackets, kDevBatchGroups, kDevStageChunkSamples, kDevResampleScratchBytes, kDevMelScratchBytes, kDevTrimScratchBytes, kDevCount };
long dev_option(DevOption which);

#define AFG_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) {                                                         \
            ::afg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),     \
                             __FILE__, __LINE__);                                        \
            return AFG_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

// Caller-owned room for plan tables: `host` is page-locked, `dev` device memory of the same size; tables of plans
// created with an arena are written to `host`, copied on `stream` and never allocated or waited for (the host
// pipeline creates plans while earlier chunks are in flight: a synchronous upload would queue behind their copies).
struct PlanArena {
    uint8_t *host = nullptr, *dev = nullptr;
    size_t cap = 0, used = 0;
    hipStream_t stream = nullptr;
};

// afg_mp3_plan_create with explicit block offsets per stream (NULL: packed); see mp3_transform.hip
int mp3_plan_create_at(afg_mp3_plan **plan, uint32_t n_streams, const uint32_t *granules, const uint8_t *channels,
                       const uint64_t *blk_base, uint32_t seg_granules, PlanArena *arena = nullptr);

// the MP3 transform in AFG_NUMERIC_TOLERANCE (mp3_tolerance.hip); d_segs / d_streams are the plan's device tables
void mp3_launch_tolerance(uint32_t n_segs, const void *d_segs, const void *d_streams, const float *d_coef,
                          const uint32_t *d_flags, float *d_pcm, float *d_state, hipStream_t stream);

// afg_vorbis_plan_create with an explicit input offset per stream (NULL: packed); see vorbis_transform.hip
int vorbis_plan_create_at(afg_vorbis_plan **plan, uint32_t n_streams, const uint32_t *packets, const uint8_t *channels,
                          const uint16_t *blocksize0, const uint16_t *blocksize1, const uint8_t *pflags,
                          const uint64_t *spec_base, uint32_t seg_packets);

// afg_collate_hip for a caller that still has the spans in host memory (h_spans: what d_spans was uploaded from, on
// `stream`): the checks run on them and nothing waits for the device (collate.hip)
int collate_launch(const afg_collate_span *h_spans, uint64_t n_spans, const afg_collate_span *d_spans, uint64_t n_tiles,
                   const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, hipStream_t stream);

// afg_resample_hip likewise, for a caller that still has the rows in host memory (resample.hip)
int resample_launch(const afg_resample_row *h_rows, uint64_t n_rows, const afg_resample_row *d_rows, uint64_t n_tiles,
                    const float *d_in, uint64_t in_floats, const float *d_taps, uint64_t taps_floats, float *d_out,
                    uint64_t out_floats, hipStream_t stream);

// afg_melspec_hip likewise (melspec.hip)
int melspec_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params,
                   const float *d_in, uint64_t in_floats, const float *d_basis, uint64_t basis_floats, const float *d_filters,
                   uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream);

// afg_melspec_fft_hip likewise (melspec_fft.hip), and the n_fft its path takes: 16 .. 2048 with prime factors 2, 3 and 5 only
int melspec_fft_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_mel_params *params,
                       const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters,
                       uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream);
bool mel_fft_n_ok(uint32_t n_fft);

// afg_stft_hip likewise (stft.hip), and max_frames of a row for its parameters (afg_mel_frames' formula)
uint32_t stft_frames(const afg_stft_params &p, uint32_t in_frames);
int stft_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_stft_params *params,
                const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, float *d_out, uint64_t out_floats,
                hipStream_t stream);

// afg_fbank_hip likewise (fbank.hip), and the check of its parameters alone (who: the caller's prefix)
int fbank_check_params(const afg_fbank_params *params, const char *who);
int fbank_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_fbank_params *params,
                 const float *d_in, uint64_t in_floats, const float *d_table, uint64_t table_floats, const float *d_filters,
                 uint64_t filters_floats, float *d_out, uint64_t out_floats, hipStream_t stream);

// afg_yin_hip likewise (yin.hip), the check of its parameters alone (who: the caller's prefix) and a row's frames
int yin_check_params(const afg_yin_params *params, const char *who);
uint32_t yin_frames_of(const afg_yin_params &params, uint32_t in_frames);
int yin_launch(const afg_mel_row *h_rows, uint64_t n_rows, const afg_mel_row *d_rows, uint64_t n_tiles, const afg_yin_params *params,
               const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, hipStream_t stream);

// afg_normalize_hip likewise (normalize.hip)
int normalize_launch(const afg_norm_group *h_groups, uint64_t n_groups, const afg_norm_group *d_groups, uint64_t n_tiles,
                     const afg_norm_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                     void *d_partials, afg_norm_stats *d_stats, hipStream_t stream);

// afg_slide_cmn_hip likewise (slidecmn.hip)
int slide_cmn_launch(const afg_cmn_slab *h_slabs, uint64_t n_slabs, const afg_cmn_slab *d_slabs, uint64_t n_tiles, const afg_cmn_params *params,
                     const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, void *d_work, uint64_t work_bytes,
                     hipStream_t stream);

// afg_cepstra_hip likewise (cepstra.hip)
int cepstra_launch(const afg_cep_row *h_rows, uint64_t n_rows, const afg_cep_row *d_rows, uint64_t n_tiles, const afg_cep_params *params,
                   const float *d_in, uint64_t in_floats, const float *d_dct, uint64_t dct_floats, float *d_out, uint64_t out_floats,
                   hipStream_t stream);

// afg_trim_hip likewise (trim.hip)
int trim_launch(const afg_trim_group *h_groups, uint64_t n_groups, const afg_trim_group *d_groups, uint64_t n_blocks, uint64_t n_tiles,
                const afg_trim_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_blocks,
                afg_trim_region *d_regions, hipStream_t stream);

// afg_filter_hip likewise (filter.hip).  filter_check_params and filter_tables are host only (host/afg_filter.cpp): the
// cascade's checks, the bound's cap included, and the kernel's tables -- per section kFilterSecDoubles doubles: the five
// coefficients at 0, the chunk's two homogeneous responses at kFilterH1 and kFilterH2, A^(16 i) for i = 0 .. 64 at kFilterPow
constexpr uint32_t kFilterH1 = 8, kFilterH2 = 24, kFilterPow = 40, kFilterSecDoubles = 300;
int filter_check_params(const afg_filter_params *params);
void filter_tables(const afg_filter_params *params, std::vector<double> &tab);
int filter_launch(const afg_filter_row *h_rows, uint64_t n_rows, const afg_filter_row *d_rows, const afg_filter_params *params,
                  const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats, double *d_state, hipStream_t stream);

// afg_loudness_hip likewise (loudness.hip).  loudness_check_params, loudness_kweight (the K-weighting of a rate, checked),
// loudness_step (100 ms in samples) and loudness_blocks (whole gating blocks of `valid` samples) are host only
// (host/afg_loudness.cpp)
int loudness_check_params(const afg_loudness_params *params);
int loudness_kweight(uint32_t samplerate, afg_filter_params *out);
constexpr uint32_t loudness_step(uint32_t samplerate) { return (samplerate + 5u) / 10u; }
constexpr uint32_t loudness_blocks(uint32_t valid, uint32_t step) { return valid >= 4u * step ? (valid - 4u * step) / step + 1u : 0u; }
int loudness_launch(const afg_loudness_group *h_groups, uint64_t n_groups, const afg_loudness_group *d_groups, const afg_loudness_counts *counts,
                    const afg_loudness_params *params, const float *d_in, uint64_t in_floats, float *d_out, uint64_t out_floats,
                    double *d_sub, double *d_blocks, afg_loudness_stats *d_stats, hipStream_t stream);

// afg_mix_hip likewise (mix.hip); the planes' addresses give afg_mix_check_groups its plane_at
int mix_launch(const afg_mix_group *h_groups, uint64_t n_groups, const afg_mix_group *d_groups, uint64_t n_tiles, const float *d_in,
               uint64_t in_floats, const float *d_noise, uint64_t noise_floats, float *d_out, uint64_t out_floats, void *d_partials,
               afg_mix_stats *d_stats, hipStream_t stream);

// Owns a device buffer filled from a host array at plan creation.
struct DeviceArray {
    void *ptr = nullptr;
    size_t bytes = 0;
    bool owned = true;                  // false: points into a PlanArena
    int upload(const void *host, size_t nbytes);
    void release();
};

}  // namespace afg
