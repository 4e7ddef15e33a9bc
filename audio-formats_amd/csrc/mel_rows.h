// mel_rows.h -- the afg_mel_row check that the three framing stages share (melspec.hip, melspec_fft.hip, stft.hip; host
// only, beside fft_frame.h): first_tile against the layout, the row inside the input, out_frames against the frames the row
// has, reflect padding, the slab inside the output.  The messages are the stage's: it passes its prefix and names.
#pragma once
#include "afg_records.h"

namespace afg {

// Every afg_mel_row of a framing stage (melspec.hip, melspec_fft.hip, stft.hip) against the planes and the tile table.
// who, layout: the stage's prefix and its layout function's name; tile: frames per tile; reflect_pad: the samples reflect
// padding folds (0: none, or zero padding); frame_floats: floats of one output frame; max_frames(in_frames): the frames a
// row of that many samples has.
template <typename MaxFrames>
int check_mel_rows(const char *who, const char *layout, const afg_mel_row *rows, uint64_t n_rows, uint64_t n_tiles, uint32_t tile,
                   uint32_t reflect_pad, uint64_t frame_floats, uint64_t in_floats, uint64_t out_floats, MaxFrames max_frames)
{
    uint64_t tiles = 0;
    for (uint64_t k = 0; k < n_rows; k++) {
        const afg_mel_row &r = rows[k];
        const unsigned long long kk = (unsigned long long)k;
        if (r.first_tile != tiles) {
            set_error("%s: row %llu: first_tile %llu, %s gives %llu", who, kk, (unsigned long long)r.first_tile, layout, (unsigned long long)tiles);
            return AFG_ERR_INVALID;
        }
        tiles += ((uint64_t)r.out_frames + tile - 1) / tile;
        if (r.in_frames && !rows_inside(r.in_off, 1, 0, r.in_frames, in_floats)) {
            set_error("%s: row %llu: the row leaves the input (%llu floats)", who, kk, (unsigned long long)in_floats);
            return AFG_ERR_INVALID;
        }
        if (r.out_frames == 0) continue;
        const uint32_t most = max_frames(r.in_frames);
        if (r.out_frames > most) {
            set_error("%s: row %llu: out_frames %u, but %u samples have %u frames", who, kk, r.out_frames, r.in_frames, most);
            return AFG_ERR_INVALID;
        }
        if (reflect_pad && r.in_frames <= reflect_pad) {
            set_error("%s: row %llu: reflect padding of %u samples needs more than %u samples in the row (%u)", who, kk, reflect_pad, reflect_pad,
                      r.in_frames);
            return AFG_ERR_INVALID;
        }
        const uint64_t need = frame_floats * r.out_frames;       // < 2^44
        if (!rows_inside(r.out_off, 1, 0, need, out_floats)) {
            set_error("%s: row %llu: the row's %llu floats leave the output (%llu floats)", who, kk, (unsigned long long)need, (unsigned long long)out_floats);
            return AFG_ERR_INVALID;
        }
    }
    if (tiles != n_tiles) {
        set_error("%s: n_tiles %llu, %s gives %llu", who, (unsigned long long)n_tiles, layout, (unsigned long long)tiles);
        return AFG_ERR_INVALID;
    }
    return AFG_OK;
}

}  // namespace afg
