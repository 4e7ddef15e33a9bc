"""The QOA frame decoder of include/afg.h (afg_qoa_transform_hip) as integer arithmetic in NumPy int64, with every 32-bit
wrap written out -- a second statement of the format beside oracle/qoa_lms.c, sharing no code with it or with the kernel.

A frame (include/afg.h; the public QOA specification): an 8-byte header, then per channel 16 bytes of LMS state -- four
history values and four weights, big-endian int16 -- then 64-bit big-endian slices, channel-interleaved: slice s of
channel c is word s * channels + c.  A slice holds a 4-bit scalefactor in its top bits and 20 residual codes of 3 bits
below it, first sample highest.  Per sample:

    prediction = wrap32(sum of weight[i] * history[i]) >> 13         (arithmetic shift)
    value      = clamp_int16(prediction + dequant[scalefactor][code])
    weight[i]  = wrap32(weight[i] + (history[i] < 0 ? -delta : delta)),  delta = dequant >> 4
    history    = history[1:] + [value]

and the float output is float32(value) * float32(1.0 / 32767).  A record with samples == 0 writes nothing.
"""
import numpy as np

SLICE_LEN = 20

# dequant[scalefactor][code]: round(scalefactor_value * {0.75, -0.75, 2.5, -2.5, 4.5, -4.5, 7, -7}) of the specification,
# scalefactor_value = round((s + 1) ** 2.75), written out
DEQUANT = np.array([
    [1, -1, 3, -3, 5, -5, 7, -7],
    [5, -5, 18, -18, 32, -32, 49, -49],
    [16, -16, 53, -53, 95, -95, 147, -147],
    [34, -34, 113, -113, 203, -203, 315, -315],
    [63, -63, 210, -210, 378, -378, 588, -588],
    [104, -104, 345, -345, 621, -621, 966, -966],
    [158, -158, 528, -528, 950, -950, 1477, -1477],
    [228, -228, 760, -760, 1368, -1368, 2128, -2128],
    [316, -316, 1053, -1053, 1895, -1895, 2947, -2947],
    [422, -422, 1405, -1405, 2529, -2529, 3934, -3934],
    [548, -548, 1828, -1828, 3290, -3290, 5117, -5117],
    [696, -696, 2320, -2320, 4176, -4176, 6496, -6496],
    [868, -868, 2893, -2893, 5207, -5207, 8099, -8099],
    [1064, -1064, 3548, -3548, 6386, -6386, 9933, -9933],
    [1286, -1286, 4288, -4288, 7718, -7718, 12005, -12005],
    [1536, -1536, 5120, -5120, 9216, -9216, 14336, -14336]], np.int64)


def wrap32(v):
    """int64 values reduced to two's-complement 32 bits"""
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def step(h, w, deq):
    """One sample of every row: h, w int64 [rows, 4] (history, weights; updated in place), deq int64 [rows] the dequantised
    residual.  Returns the reconstructed values."""
    pred = wrap32((w * h).sum(axis=1)) >> 13
    value = np.clip(pred + deq, -32768, 32767)
    delta = (deq >> 4)[:, None]
    w[:] = wrap32(w + np.where(h < 0, -delta, delta))
    h[:, :3] = h[:, 1:]
    h[:, 3] = value
    return value


def decode(frames, data, out_total, stats=None):
    """frames: afgpu.QOA_FRAME_DTYPE records over the byte plane `data`.  Returns (written, int16 values, float32 values),
    each of out_total entries: `written` marks the entries some frame wrote, the values are 0 elsewhere.
    stats (a dict, optional) receives "max_abs_weight": per record, the largest weight magnitude any of its channels
    reached, after the wrap."""
    data = np.ascontiguousarray(data, np.uint8)
    out_total = int(out_total)
    written = np.zeros(out_total, bool)
    vals = np.zeros(out_total, np.int16)
    # one row per (frame, channel), longest first: the rows still running at sample t are a prefix
    fc = [(int(fr["samples"]), f, c) for f, fr in enumerate(frames) for c in range(int(fr["channels"])) if int(fr["samples"])]
    fc.sort(key=lambda x: -x[0])
    n = len(fc)
    peak = np.zeros(len(frames), np.int64)
    if n:
        length = np.array([x[0] for x in fc], np.int64)
        fidx = np.array([x[1] for x in fc], np.int64)
        chan = np.array([x[2] for x in fc], np.int64)
        nch = frames["channels"].astype(np.int64)[fidx]
        base = frames["byte_off"].astype(np.int64)[fidx]
        out0 = frames["out_off"].astype(np.int64)[fidx] + chan
        max_slices = -(-int(length[0]) // SLICE_LEN)
        h = np.zeros((n, 4), np.int64)
        w = np.zeros((n, 4), np.int64)
        words = np.zeros((n, max_slices), np.uint64)
        for r in range(n):
            at = int(base[r]) + 8 + 16 * int(chan[r])
            state = data[at:at + 16].view(">i2").astype(np.int64)
            h[r], w[r] = state[:4], state[4:]
            nsl = -(-int(length[r]) // SLICE_LEN)
            first = int(base[r]) + 8 + 16 * int(nch[r])
            body = data[first:first + 8 * nsl * int(nch[r])].view(">u8").astype(np.uint64)
            words[r, :nsl] = body[int(chan[r])::int(nch[r])]
        wmax = np.abs(w).max(axis=1)
        neg_len = -length
        for t in range(int(length[0])):
            m = int(np.searchsorted(neg_len, -t, side="left"))          # rows with length > t
            word = words[:m, t // SLICE_LEN]
            sf = (word >> np.uint64(60)).astype(np.int64)
            code = ((word >> np.uint64(57 - 3 * (t % SLICE_LEN))) & np.uint64(7)).astype(np.int64)
            deq = DEQUANT[sf, code]
            value = step(h[:m], w[:m], deq)
            np.maximum(wmax[:m], np.abs(w[:m]).max(axis=1), out=wmax[:m])
            at = out0[:m] + t * nch[:m]
            assert not written[at].any() and len(np.unique(at)) == m, "two frames write the same output value"
            written[at] = True
            vals[at] = value
        np.maximum.at(peak, fidx, wmax)
    if stats is not None:
        stats["max_abs_weight"] = peak
    return written, vals, vals.astype(np.float32) * np.float32(1.0 / 32767)
