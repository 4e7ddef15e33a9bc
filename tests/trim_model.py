"""The silence trim of include/afg.h restated in numpy: the blocks' powers of a group of rows in the definition's fixed order
(a lane per sample index mod 64, sequential in a lane, a tree of 6 halvings over the 64 lanes, the rows one after the other),
the frames of k blocks, the threshold, the region's index arithmetic and the shifted, zero-padded output.  The device is
compared with this bit for bit."""
import numpy as np

LANES, TILE = 64, 4096
REF_MAX, REF_ABS = 0, 1
GROUP_DTYPE = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("in_stride", np.uint64), ("out_stride", np.uint64),
                        ("first_block", np.uint64), ("first_tile", np.uint64), ("rows", np.uint32), ("valid", np.uint32),
                        ("out_rows", np.uint32), ("out_frames", np.uint32)])
REGION_DTYPE = np.dtype([("begin", np.uint32), ("end", np.uint32), ("ref_power", np.float64)])
assert GROUP_DTYPE.itemsize == 64 and REGION_DTYPE.itemsize == 16
F32, F64 = np.float32, np.float64


def params(top_db=60.0, frame_length=2048, hop=512, reference=REF_MAX, abs_power=1.0, lead=0, trail=0, ratio=None):
    """the parameters as a dict; ratio = 10 ** (-top_db / 10) in double unless given"""
    k = frame_length // hop
    assert hop >= 1 and frame_length % hop == 0 and (k == 1 or (k % 2 == 0 and k <= 64)) and frame_length <= 65536
    return dict(frame_length=int(frame_length), hop=int(hop), reference=int(reference), lead=int(lead), trail=int(trail),
                ratio=float(10.0 ** (-float(top_db) / 10.0) if ratio is None else ratio), abs_power=float(abs_power))


def block_powers(rows, hop):
    """S_j of a group given as [rows, valid] float32: float64 [ceil(valid / hop)]"""
    rows = np.asarray(rows, F32)
    assert rows.ndim == 2
    n_rows, valid = rows.shape
    nb = -(-valid // hop)
    if nb == 0:
        return np.zeros(0, F64)
    steps = -(-hop // LANES)
    x = np.zeros((n_rows, nb * hop), F32)                        # (a lane that adds +0.0 * +0.0 keeps its bits: a sum is never -0.0)
    x[:, :valid] = rows
    x = x.reshape(n_rows, nb, hop)
    if steps * LANES != hop:
        x = np.concatenate([x, np.zeros((n_rows, nb, steps * LANES - hop), F32)], axis=2)
    x = x.reshape(n_rows, nb, steps, LANES)                      # sample i of a block: step i // 64 of lane i % 64
    q = np.zeros((n_rows, nb, LANES), F64)
    with np.errstate(all="ignore"):
        for s in range(steps):                                   # sequential in a lane, all lanes at once
            d = x[:, :, s, :].astype(F64)
            q = q + d * d
        while q.shape[-1] > 1:                                   # 6 halvings: v[l] = v[l] + v[l + d] for l % (2 d) == 0
            q = q[..., 0::2] + q[..., 1::2]
        S = np.zeros(nb, F64)
        for r in range(n_rows):                                  # the rows in ascending order, from +0.0
            S = S + q[r, :, 0]
    return S


def frame_powers(S, k):
    """P_f of the len(S) frames: the S_j of blocks [f - k / 2, f + k / 2) cut to the blocks there are (block f alone for
    k == 1), added in ascending j from +0.0"""
    nb = S.size
    P = np.zeros(nb, F64)
    f = np.arange(nb)
    with np.errstate(all="ignore"):
        for off in ([0] if k == 1 else range(-(k // 2), k // 2)):
            j = f + off
            ok = (j >= 0) & (j < nb)
            P = np.where(ok, P + S[np.clip(j, 0, max(nb - 1, 0))], P)
    return P


def region(rows, prm):
    """(begin, end, ref_power, S, P) of a group given as [rows, valid] float32"""
    rows = np.asarray(rows, F32)
    n_rows, valid = rows.shape
    hop, k = prm["hop"], prm["frame_length"] // prm["hop"]
    S = block_powers(rows, hop)
    P = frame_powers(S, k)
    ref = F64(0.0)
    for p in P:                                                  # P > m ? P : m from +0.0: a NaN never wins
        ref = p if p > ref else ref
    with np.errstate(all="ignore"):
        if prm["reference"] == REF_ABS:
            thr = F64(prm["ratio"]) * F64(prm["abs_power"])
            thr = thr * F64(n_rows * prm["frame_length"])
        else:
            thr = F64(prm["ratio"]) * ref
        loud = np.flatnonzero(P > thr)                           # (a NaN compares false: silent)
    if loud.size == 0:
        return 0, 0, ref, S, P
    b = int(loud[0]) * hop
    e = min(valid, (int(loud[-1]) + 1) * hop)
    begin = b - prm["lead"] if b > prm["lead"] else 0
    end = min(valid, e + prm["trail"])
    return begin, end, ref, S, P


def trim(plane_in, plane_out, groups, prm):
    """every group of `groups` (GROUP_DTYPE records or dicts): returns (a copy of plane_out with the groups' slabs written,
    the REGION_DTYPE records, the blocks' powers of all groups one after the other)"""
    out = plane_out.copy()
    regions = np.zeros(len(groups), REGION_DTYPE)
    powers = []
    for i, g in enumerate(groups):
        n_rows, valid = int(g["rows"]), int(g["valid"])
        a, sa = int(g["in_off"]), int(g["in_stride"])
        x = np.stack([plane_in[a + r * sa:a + r * sa + valid] for r in range(n_rows)]) if valid else np.zeros((n_rows, 0), F32)
        begin, end, ref, S, _ = region(x, prm)
        regions[i]["begin"], regions[i]["end"], regions[i]["ref_power"] = begin, end, ref
        powers.append(S)
        o, so, T = int(g["out_off"]), int(g["out_stride"]), int(g["out_frames"])
        c = min(T, end - begin)
        for r in range(int(g["out_rows"])):
            y = out[o + r * so:o + r * so + T]
            y[:] = 0.0
            if r < n_rows:
                y[:c] = x[r, begin:begin + c]
    return out, regions, (np.concatenate(powers) if powers else np.zeros(0, F64))


def layout(groups, prm):
    """afg_trim_layout: fills first_block and first_tile, returns (n_blocks, n_tiles)"""
    blocks = tiles = 0
    for g in groups:
        g["first_block"], g["first_tile"] = blocks, tiles
        blocks += -(-int(g["valid"]) // prm["hop"])
        tiles += -(-int(g["out_frames"]) // TILE) * int(g["out_rows"])
    return blocks, tiles


def same_bits(got, want):
    """flat indices where two arrays of one 4- or 8-byte type differ as bit patterns"""
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    a, b = np.ascontiguousarray(got).view(u).ravel(), np.ascontiguousarray(want).view(u).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.flatnonzero(a != b)
