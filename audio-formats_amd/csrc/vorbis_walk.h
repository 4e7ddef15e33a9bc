// vorbis_walk.h -- entry points of the tolerance-mode Vorbis walk (vorbis_walk.hip) used by the plan code in
// vorbis_transform.hip.
#pragma once
#include "vorbis_core.h"

namespace afg_vorbis {

constexpr int kWalkShapes = 12;
// The walk's kernel for a stream with blocksize_1 in {1024, 2048, 4096} and blocksize_0 <= 512 (or = blocksize_1); with
// size = log2(blocksize_1) - 10:  2 size + (channels - 1) for mono / stereo streams (one wavefront walks every channel of
// a segment); 6 + size for 3, 5 or 7 channels (a workgroup per segment, one wavefront per channel), 9 + size for an even
// number up to 16 (a workgroup per segment, one wavefront per pair of channels); -1 for every other stream.
int walk_shape(int channels, int blocksize0, int blocksize1);
// (the rule itself, usable in constant expressions: the plan sizes its per-launch counter block by it)
constexpr int walk_shape_of(int channels, int blocksize0, int blocksize1)
{
    // (equal block sizes: every packet is a long block between long blocks to the walk -- the plan rewrites its flags)
    if (channels < 1 || (blocksize0 > 512 && blocksize0 != blocksize1) || blocksize0 > blocksize1) return -1;
    const int size = blocksize1 == 1024 ? 0 : blocksize1 == 2048 ? 1 : blocksize1 == 4096 ? 2 : -1;
    if (size < 0) return -1;
    if (channels <= 2) return 2 * size + (channels - 1);
    // More than two channels: one workgroup of at most 8 wavefronts per segment.  4096-sample blocks: one wavefront per channel
    // whatever the count (a pair's transform areas, 18 KB, would leave room for three wavefronts per CU: 15.9 ms per C3-sized
    // batch of 6 channels, against 13.9 for round 5's column stores), so at most 8 channels; the other sizes 3, 5, 7 or an
    // even number up to 16.  Everything else stays on the bit-exact kernels.
    if (size == 2) return channels <= 8 ? 8 : -1;
    if (channels & 1) return channels <= 7 ? 6 + size : -1;
    return channels <= 16 ? 9 + size : -1;
}
// The (shape, channel count) pairs above two channels that walk_shape admits: each is a launch group of a plan, with a work
// counter of its own.  (blocksize_0 does not enter the key; 255: what a stream record's channel byte can hold.)
constexpr uint32_t walk_mc_groups()
{
    uint32_t n = 0;
    for (int bs1 = 1024; bs1 <= 4096; bs1 *= 2)
        for (int ch = 3; ch <= 255; ch++) n += walk_shape_of(ch, 256, bs1) >= 6;
    return n;
}
int walk_shape_channels(int shape);          // channels one wavefront of the shape walks
int walk_shape_blocksize(int shape);
size_t walk_table_floats(int shape);
// dst: walk_table_floats(shape) floats; window: the window of the shape's blocksize_1 as stb_vorbis2.d:866-873 builds it
void walk_build_tables(int shape, float *dst, const float *window);
// Segments of streams of one shape -- for the shapes with more than two channels: of ONE channel count, `nch` (else 0) --;
// `out` 16-byte aligned; *counter zeroed on `stream`.
int walk_launch(int shape, const VorbisSeg *segs, uint32_t n_segs, int nch, const VorbisStream *streams, const uint8_t *pflags,
                const uint64_t *spec_off, const uint64_t *out_off, const float *tables, const float *walk_tables,
                const float *spec, float *out, uint32_t *counter, hipStream_t stream);

}  // namespace afg_vorbis
