"""FLAC restore at the edges of its records: subframe indices beyond 2^24 in a sparse record table, block sizes that are no
multiple of 4 (down to one sample, and shorter than the LPC order), and guard bands around every buffer the kernels
touch.  Bit-exact against the CPU oracle, int32 and float, through the C ABI like test_flac_gpu.py.

Every batch is built and checked on the host first (batch_checks: the oracle ran over it, the frames tile the output, the
sizes / row widths / alignments the case is about are really there), then goes to the device."""
import functools

import numpy as np
import pytest

import oraclelib
import afgpu
from afgpu import synthetic

pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinel elements in front of and behind every output, and behind the residual plane
OUT_SENTINEL = 0x5A5AA5A5                    # no decoded sample or float of these batches has this pattern
RES_SENTINEL = 0x7F7F7F7F                    # large as int32 and as two int16: a pad value that reaches a sample shows
SUB = afgpu.FLAC_SUBFRAME_DTYPE.itemsize     # 68


def concat(parts):
    """batches one after the other in one call (as test_flac_multichannel_and_stereo_groups_in_one_call does)"""
    frames, subs, ress = [], [], []
    in_off = out_off = sf_off = 0
    for fr, sb, rs, tot in parts:
        fr = fr.copy()
        fr["in_off"] += np.uint64(in_off); fr["out_off"] += np.uint64(out_off); fr["sf_index"] += np.uint32(sf_off)
        frames.append(fr); subs.append(sb); ress.append(rs)
        in_off += len(rs); out_off += tot; sf_off += len(sb)
    return np.concatenate(frames), np.concatenate(subs), np.concatenate(ress), out_off


def batch_checks(frames, subs, res, total):
    """what every batch must be before it goes anywhere: legal records that tile the planes; returns the oracle's samples"""
    bs, ch = frames["block_size"].astype(np.int64), frames["channels"].astype(np.int64)
    assert (bs >= 1).all() and (ch >= 1).all() and (ch <= 8).all()
    out_off = frames["out_off"].astype(np.int64)
    assert out_off[0] == 0 and (out_off[1:] == out_off[:-1] + (bs * ch)[:-1]).all() and out_off[-1] + bs[-1] * ch[-1] == total
    assert (frames["sf_index"].astype(np.int64) == np.concatenate([[0], np.cumsum(ch)[:-1]])).all() and len(subs) == ch.sum()
    for f in range(len(frames)):
        o = subs["order"][int(frames["sf_index"][f]):int(frames["sf_index"][f]) + int(ch[f])]
        assert (o <= bs[f]).all() and (o <= 32).all()                     # the generator's clamp: records stay legal
    want_i, want_f = oraclelib.flac_transform(frames, subs, res, total, want_float=True)
    assert want_i.shape == (total,) and want_f.shape == (total,)
    assert not (want_i == np.int32(OUT_SENTINEL)).any() and not (want_f.view(np.int32) == np.int32(OUT_SENTINEL)).any()
    return want_i, want_f


def pack16(frames, subs, res, total, every=1):
    """the same batch with int16 rows (residuals clipped to fit, as test_flac_multichannel_kernel_bit_exact does) and its own
    oracle samples; None when no frame is long enough to be packed (flac_pack16 leaves frames below 8 samples as int32)"""
    res16 = np.clip(res, -30000, 30000).astype(np.int32)
    fr16, packed = synthetic.flac_pack16(frames, res16, every)
    eligible = (frames["block_size"] >= 8) & (np.arange(len(frames)) % every == 0)
    assert ((fr16["res16"] != 0) == eligible).all()                       # every frame that can hold int16 rows does
    if not eligible.any():
        return None
    want_i, want_f = oraclelib.flac_transform(fr16, subs, packed, total, want_float=True)
    plain = oraclelib.flac_transform(frames, subs, res16, total)
    assert (want_i == plain).all()                                        # the oracle reads both row widths alike
    return fr16, packed, want_i, want_f


def run_device(gpu, frames, d_sub, res, total, want_i, want_f, out="both", variants=None):
    """one call with guard bands: outputs of total + 2 * GUARD elements, every out_off shifted by GUARD, GUARD sentinel words
    behind the residual plane; asserts the samples and that the bands are untouched"""
    import torch
    fr = frames.copy()
    fr["out_off"] += np.uint64(GUARD)
    d_fr = torch.from_numpy(fr.view(np.uint8).copy()).to(gpu)
    d_res = torch.from_numpy(np.concatenate([np.ascontiguousarray(res, np.int32), np.full(GUARD, RES_SENTINEL, np.int32)])).to(gpu)
    bufs = {k: torch.full((total + 2 * GUARD,), OUT_SENTINEL, dtype=torch.int32, device=gpu) for k in ("int32", "float") if out in ("both", k)}
    d_f32 = bufs["float"].view(torch.float32) if "float" in bufs else None
    afgpu.flac_transform(len(fr), d_fr, d_sub, d_res, bufs.get("int32"), d_f32, None, variants=variants)
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        got = buf.cpu().numpy()
        want = want_i if k == "int32" else want_f.view(np.int32)
        body = got[GUARD:GUARD + total]
        bad = np.nonzero(body != want)[0]
        assert bad.size == 0, f"{k} output ({out}): {bad.size} of {total} samples differ, first at {int(bad[0])}"
        assert (got[:GUARD] == np.int32(OUT_SENTINEL)).all(), f"{k} output ({out}): a store in front of the first frame"
        assert (got[GUARD + total:] == np.int32(OUT_SENTINEL)).all(), f"{k} output ({out}): a store past the last frame"


# ---------------------------------------------------------------------------------------------------------------
# A1: subframe indices above 2^24.  afg_flac_frame.sf_index is 32 bits wide and global over a batch call; a few hundred
# long 6-8-channel files pass 2^24 subframes.
# ---------------------------------------------------------------------------------------------------------------
A1_KINDS = [1, 2, 3, 6, 8, "mixed"]
A1_BASES = [2 ** 24 - 40, 2 ** 24 + 5]       # the first: the frames of one wavefront straddle 2^24


@functools.lru_cache(maxsize=None)
def a1_batch(kind, rows16):
    """48 frames of 576 samples: a 32-frame group of orders 8 / 12 and a 16-frame group of orders 12 / 32 (both order buckets of
    either kernel); "mixed": the first group stereo, the second six channels"""
    c0, c1 = (2, 6) if kind == "mixed" else (kind, kind)
    seed = 400 + 10 * A1_KINDS.index(kind)
    frames, subs, res, total = concat([synthetic.flac_batch(seed, n_frames=32, block_size=576, channels=c0, orders=(8, 12)),
                                       synthetic.flac_batch(seed + 1, n_frames=16, block_size=576, channels=c1, orders=(12, 32))])
    want_i, want_f = batch_checks(frames, subs, res, total)
    assert (subs["order"] >= 8).all() and subs["order"][:32 * c0].max() == 12 and subs["order"][32 * c0:].max() == 32
    if rows16:
        frames, res, want_i, want_f = pack16(frames, subs, res, total)
        assert (frames["res16"] == 1).all()
    mask = afgpu.flac_variants(frames, subs)          # from the compact host records: the sparse table exists on the device only
    mc, st = (mask >> 8) & 0xf, mask & 0xff
    if kind == "mixed":
        assert st and mc
    elif kind > 2:
        assert mc & 0x3 and mc & 0xc and not st, hex(mask)     # both order buckets of the multi-channel kernel, nothing else
    else:
        assert st & 0x30 and st & 0xc0 and not mc, hex(mask)
    return frames, subs, res, total, want_i, want_f, mask


@pytest.mark.parametrize("with_mask", [False, True], ids=["all", "mask"])
@pytest.mark.parametrize("rows16", [False, True], ids=["rows32", "rows16"])
@pytest.mark.parametrize("base", A1_BASES, ids=["straddle", "above"])
@pytest.mark.parametrize("kind", A1_KINDS, ids=[f"ch{k}" for k in A1_KINDS])
def test_flac_subframe_index_above_2_24(gpu, kind, base, rows16, with_mask):
    """The records of a small batch sit at index `base` .. of a zero-filled subframe table (1.15 GB, device only) and every
    frame's sf_index is `base` higher: the samples are those of the compact batch.  A kernel that carries the index in
    fewer than 32 bits reads other records and decodes other samples."""
    import torch
    frames, subs, res, total, want_i, want_f, mask = a1_batch(kind, rows16)
    if torch.cuda.mem_get_info(gpu)[0] < 4 << 30:
        pytest.skip("less than 4 GiB of device memory free")
    n_sub = len(subs)
    # A zero record is a valid order-0 subframe, and the table is allocated from index 0: every index a kernel could
    # form by dropping high bits of a frame's sf_index (+ channel) is smaller than the true one and so lies inside the
    # allocation.  A truncating kernel reads in-bounds decoys and produces wrong samples, never an out-of-bounds access.
    d_sub = torch.zeros((base + n_sub) * SUB, dtype=torch.uint8, device=gpu)
    d_sub[base * SUB:] = torch.from_numpy(subs.view(np.uint8).copy()).to(gpu)
    fr = frames.copy()
    fr["sf_index"] += np.uint32(base)
    assert int((fr["sf_index"].astype(np.int64) + fr["channels"]).max()) == base + n_sub and int(fr["sf_index"].max()) >= 2 ** 24
    run_device(gpu, fr, d_sub, res, total, want_i, want_f, "both", mask if with_mask else None)


# ---------------------------------------------------------------------------------------------------------------
# A2: block sizes that are no multiple of 4 -- the scalar tail of the int32 row loads, interleaved 16-byte stores at 4- and
# 8-byte aligned offsets, int16 rows padded to 8, frames shorter than a 64-sample tile and shorter than their LPC order.
# ---------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [1, 2, 3, 5, 7, 9, 63, 64, 65, 127, 129, 1001, 4095, 4097]
EDGE_CHANNELS = [1, 2, 3, 5, 6, 8]
ORDER_SETS = [(2, 4), (5, 8), (9, 12), (12, 32), (1, 7, 31)]          # one per order bucket of the kernels, and a spread
ALL_ASSIGNMENTS = {afgpu.FLAC_INDEPENDENT, afgpu.FLAC_LEFT_SIDE, afgpu.FLAC_RIGHT_SIDE, afgpu.FLAC_MID_SIDE}


def flac_kw(bps):
    """24 bits: sums that need the 64-bit accumulator; stereo: the four channel assignments alike"""
    return dict(bps=bps, assignment_p=(0.25, 0.25, 0.25, 0.25), **(dict(residual_scale=3000.0) if bps == 24 else {}))


def run_all_ways(gpu, frames, subs, res, total, want_i, want_f, every=1):
    """int32 rows and int16 rows x both outputs (the general step), int32 only and float only (mono / stereo: the common step)"""
    import torch
    d_sub = torch.from_numpy(subs.view(np.uint8).copy()).to(gpu)
    p16 = pack16(frames, subs, res, total, every)
    for out in ("both", "int32", "float"):
        run_device(gpu, frames, d_sub, res, total, want_i, want_f, out)
        if p16 is not None:
            run_device(gpu, p16[0], d_sub, p16[1], total, p16[2], p16[3], out)
    return p16


@functools.lru_cache(maxsize=None)
def edge_batch(bs, ch):
    """33 .. 70 frames of one block size (a ragged last 32-frame group); orders, sample width cycled over the cases"""
    k = 7 * EDGE_SIZES.index(bs) + EDGE_CHANNELS.index(ch)
    orders, bps, n_frames = ORDER_SETS[k % 5], (16, 24)[k % 2], 33 + (11 * k) % 38
    n_frames += n_frames == 64                                             # (never whole groups only)
    frames, subs, res, total = synthetic.flac_batch(1000 + k, n_frames=n_frames, block_size=bs, channels=ch, orders=orders, **flac_kw(bps))
    want_i, want_f = batch_checks(frames, subs, res, total)
    assert 33 <= n_frames <= 70 and n_frames % 32 and (frames["block_size"] == bs).all() and (frames["channels"] == ch).all()
    assert subs["order"].max() == min(max(orders), bs)                    # small blocks: orders clamped to the block
    if ch == 2:
        assert set(frames["assignment"].tolist()) == ALL_ASSIGNMENTS
    if bps == 24:
        assert subs["use64"].all()
    return frames, subs, res, total, want_i, want_f


@pytest.mark.parametrize("ch", EDGE_CHANNELS)
@pytest.mark.parametrize("bs", EDGE_SIZES)
def test_flac_block_size_not_a_multiple_of_4(gpu, bs, ch):
    frames, subs, res, total, want_i, want_f = edge_batch(bs, ch)
    p16 = run_all_ways(gpu, frames, subs, res, total, want_i, want_f)
    assert (p16 is not None) == (bs >= 8)


@functools.lru_cache(maxsize=None)
def order32_batch(bs, ch):
    bps = 24 if ch in (2, 8) else 16
    frames, subs, res, total = synthetic.flac_batch(2000 + bs + ch, n_frames=40, block_size=bs, channels=ch, orders=(32,), **flac_kw(bps))
    want_i, want_f = batch_checks(frames, subs, res, total)
    assert (subs["order"] == 32).all()
    return frames, subs, res, total, want_i, want_f


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
@pytest.mark.parametrize("bs", [33, 65])
def test_flac_order_32_in_a_block_hardly_longer(gpu, bs, ch):
    """32 warm-up samples and one (bs 33) or 33 (bs 65: one of them in the second tile) predicted ones"""
    frames, subs, res, total, want_i, want_f = order32_batch(bs, ch)
    assert run_all_ways(gpu, frames, subs, res, total, want_i, want_f) is not None


# block sizes of the concatenated batch: five frames each, short and long ones alternating so that a wavefront's 32 frames hold
# int32 rows (below 8 samples) and int16 rows side by side
MIX_SIZES = [1, 9, 2, 63, 3, 64, 5, 65, 7, 127, 129, 1001, 4095, 4097]
MIX_KINDS = [1, 2, 3, 5, 6, 8, "mixed"]


@functools.lru_cache(maxsize=None)
def mixed_size_batch(kind):
    i = MIX_KINDS.index(kind)
    bps = (16, 24)[i % 2]
    parts = []
    for j, bs in enumerate(MIX_SIZES):
        ch = EDGE_CHANNELS[j % 6] if kind == "mixed" else kind
        parts.append(synthetic.flac_batch(3000 + 20 * i + j, n_frames=5, block_size=bs, channels=ch, orders=ORDER_SETS[(i + j) % 5], **flac_kw(bps)))
    frames, subs, res, total = concat(parts)
    want_i, want_f = batch_checks(frames, subs, res, total)
    assert set(frames["block_size"].tolist()) == set(EDGE_SIZES) and len(frames) == 70
    # the alignments of a frame's rows and of its samples: every residue mod 4 that the channel count allows
    residues = {0, 1, 2, 3} if kind == "mixed" or kind % 2 else {0, 2} if kind % 4 else {0}
    assert set((frames["out_off"] % 4).tolist()) == residues and set((frames["in_off"] % 4).tolist()) == residues
    return frames, subs, res, total, want_i, want_f


@pytest.mark.parametrize("kind", MIX_KINDS, ids=[f"ch{k}" for k in MIX_KINDS])
def test_flac_block_sizes_mixed_in_one_call(gpu, kind):
    """frames of every size above in one call: in_off and out_off at every alignment, tiles of a wavefront that end at 32 different
    places, and -- int16 rows -- both row widths inside one wavefront"""
    frames, subs, res, total, want_i, want_f = mixed_size_batch(kind)
    fr16 = run_all_ways(gpu, frames, subs, res, total, want_i, want_f)[0]
    assert fr16["res16"][:32].any() and not fr16["res16"][:32].all()
