"""Hand-made granule records for afg_mp3_requant_hip (test infrastructure): the values, scales, tables, stereo plans and
plane layouts that files out of tests/mp3_bitstream.py reach rarely or never.  tests/test_mp3_requant_model.py holds the
inputs to their coverage (`branches`) on the CPU; tests/test_mp3_requant_edges_gpu.py holds the kernel to `expected`.

The model is mp3_requant_model.requant_numpy, which writes a granule's spectra at its q_off; `expected` moves them to
coef_off and leaves SENTINEL everywhere else."""
import functools

import numpy as np

import afgpu
import mp3_requant_model as model

SENTINEL = 0x7fc0dead                               # a quiet NaN with a payload: what d_coef holds before the launch
NO_SDESC = 0xffffffff                               # AFG_MP3_NO_SDESC (include/afg.h)
F32 = np.float32
# The range of L3_decode_scalefactors (minimp3.d:646-720): a band scale is 2^(gain_exp / 4) * 2^(-(iscf << scf_shift) / 4)
# with gain_exp = global_gain - 214 - (2 with mid/side) in -216 .. 41 and iscf << scf_shift at most (15 + (7 << 1)) << 2 =
# 116.  Smallest: 2^-54 * 2^-29 (both exact in L3_ldexp_q2).  Largest: 2^(41/4), which L3_ldexp_q2 forms as
# 2048 * (g_expfrac[3] * 2^30) in float32.
SCALE_MIN = F32(2.0 ** -83)
SCALE_MAX = F32(2048) * (F32(5.53767716e-10) * F32(2 ** 30))
SPECIAL = (0, 1, 128, 129, 1023, 1024, model.MAX_ABS)
CLASSES = ("zero", "table", "formula_lt1024", "formula_ge1024", "sign_taken_shifted", "sign_not_shifted", "sign_taken_unshifted",
           "sign_not_unshifted", "v8206", "mode0", "mode1", "mode2", "ms_zero_pair", "intensity_zero_line", "fl_zero", "fl_one",
           "fl_negative", "fr_zero", "fr_one", "fr_negative", "ro0_yes", "ro0_no", "ro1_yes", "ro1_no", "t0_ne_t1", "ro0_ne_ro1",
           "offsets_differ", "nch0", "nch1", "nch2")


def line_modes(g, sd, bol):
    """the stereo mode of each of the 576 line pairs of a two-channel granule, and the descriptor's fl / fr there"""
    if g["stereo"] != 2:
        return np.full(576, int(g["stereo"]), np.uint8), None, None
    d = sd[int(g["sdesc"])]
    b = bol[int(g["table"][0]) & 31]
    return d["type"][b], d["fl"][b], d["fr"][b]


def branches(q, gr, sd):
    """How many lines of an input set fall into each class of CLASSES (nch0 / nch1 / nch2 count records, offsets_differ
    too).  The sign classes are `2 * x & 64` of L3_pow_43 set or clear, below 1024 (x shifted left by 3) and from 1024 up;
    the modes are per line pair of two-channel granules, the reorder bits and table classes per line of them too
    (ro0 also of mono granules); the tables are this module's own, not the product's."""
    bol = model.tables_from_bands()[0]
    n = dict.fromkeys(CLASSES, 0)
    flat = q.reshape(-1)
    for g in gr:
        nch = int(g["nch"])
        n[f"nch{nch}"] += 1
        if nch == 0:
            continue
        n["offsets_differ"] += int(g["q_off"] != g["coef_off"])
        v = flat[int(g["q_off"]):int(g["q_off"]) + 576 * nch].astype(np.int64).reshape(nch, 576)
        a = np.abs(v)
        n["zero"] += int((a == 0).sum())
        n["table"] += int(((a > 0) & (a < 129)).sum())
        n["formula_lt1024"] += int(((a >= 129) & (a < 1024)).sum())
        n["formula_ge1024"] += int((a >= 1024).sum())
        n["v8206"] += int((a == model.MAX_ABS).sum())
        lo, hi = a[(a >= 129) & (a < 1024)] << 3, a[a >= 1024]
        n["sign_taken_shifted"] += int(((2 * lo & 64) != 0).sum())
        n["sign_not_shifted"] += int(((2 * lo & 64) == 0).sum())
        n["sign_taken_unshifted"] += int(((2 * hi & 64) != 0).sum())
        n["sign_not_unshifted"] += int(((2 * hi & 64) == 0).sum())
        ro = [bool(t & 0x80) for t in g["table"]]
        n["ro0_yes" if ro[0] else "ro0_no"] += 576
        if nch == 1:
            continue
        n["ro1_yes" if ro[1] else "ro1_no"] += 576
        n["t0_ne_t1"] += 576 * int((g["table"][0] & 31) != (g["table"][1] & 31))
        n["ro0_ne_ro1"] += 576 * int(ro[0] != ro[1])
        mode, fl, fr = line_modes(g, sd, bol)
        for m in range(3):
            n[f"mode{m}"] += int((mode == m).sum())
        n["ms_zero_pair"] += int(((mode == 1) & (a[0] == 0) & (a[1] == 0)).sum())
        if fl is not None:
            it = mode == 2
            n["intensity_zero_line"] += int((it & (a[0] == 0)).sum())
            for name, f in (("fl", fl), ("fr", fr)):
                n[name + "_zero"] += int((it & (f == 0)).sum())
                n[name + "_one"] += int((it & (f == 1)).sum())
                n[name + "_negative"] += int((it & (f < 0)).sum())
    return n


def draw_values(rng):
    """576 signed values: a third zeros, the rest log-uniform over 1 .. 8206; on random lines the switch points of requant
    and L3_pow_43 and both sides of the sign step, below 1024 (x << 3: (x & 7) == 3 | 4) and above ((x & 63) == 31 | 32)"""
    mag = np.floor(np.exp(rng.uniform(0, np.log(model.MAX_ABS + 1), 576))).astype(np.int64).clip(1, model.MAX_ABS)
    mag[rng.random(576) < 1 / 3] = 0
    lo, hi = 8 * rng.integers(17, 128, 2), 64 * rng.integers(16, 128, 2)
    put = list(SPECIAL) + list(SPECIAL[1:]) + [lo[0] + 3, lo[1] + 4, hi[0] + 31, hi[1] + 32]
    mag[rng.choice(576, len(put), replace=False)] = put
    assert mag.max() <= model.MAX_ABS
    return (mag * np.where(rng.random(576) < 0.5, -1, 1)).astype(np.int16)


def draw_scales(rng):
    """40 band scales: a small odd factor times a power of two inside [SCALE_MIN, SCALE_MAX], both ends among them"""
    s = (rng.choice([1, 3, 5, 7, 9, 11, 13, 15], 40) * 2.0 ** rng.integers(-83, 7, 40)).astype(F32)
    where = rng.choice(40, 2, replace=False)
    s[where[0]], s[where[1]] = SCALE_MIN, SCALE_MAX
    assert (s >= SCALE_MIN).all() and (s <= SCALE_MAX).all()
    return s


def draw_factors(rng, n):
    """intensity factors: 0, 1, negative and ordinary ones"""
    kind = rng.integers(0, 4, n)
    plain = (rng.uniform(0.05, 1.45, n)).astype(F32)
    return np.where(kind == 0, F32(0), np.where(kind == 1, F32(1), np.where(kind == 2, -plain, plain))).astype(F32)


def table_byte(t):
    """bit 7, the reorder bit, goes with the kinds short and mixed, as in the parser's records"""
    return t | (0x80 if t >= 8 else 0)


def draw_tables(rng, n):
    """n (table[0], table[1]) pairs: every index but REFUSED in either place; equal pairs, and unequal ones with all four
    combinations of the reorder bit"""
    legal = [t for t in range(24) if t != model.REFUSED]
    longs, shorts = [t for t in legal if t < 8], [t for t in legal if t >= 8]
    pairs = [(t, t) for t in legal] + [(t, legal[(i + 7) % len(legal)]) for i, t in enumerate(legal)]
    while len(pairs) < n:
        k = len(pairs) % 5
        a, b = ((longs, longs), (longs, shorts), (shorts, longs), (shorts, shorts), (legal, legal))[k]
        t0, t1 = int(rng.choice(a)), int(rng.choice(b))
        if k < 4 and t0 == t1:
            continue
        pairs.append((t0, t1))
    return [pairs[i] for i in rng.permutation(len(pairs))[:n]]


@functools.lru_cache(maxsize=None)
def hand_made(seed, n_records=200):
    """One launch: (q int16 [blocks, 576], granule records, stereo descriptors, floats of the coefficient plane, mask of the
    floats the launch writes).  Blocks of q and of the plane are laid out in two independent shuffled orders with 1 .. 3
    blocks between granules; what lies between holds values in q and must stay untouched in the plane."""
    rng = np.random.default_rng(seed)
    bol = model.tables_from_bands()[0]
    n0, n1 = max(1, n_records // 10), max(1, n_records * 3 // 20)       # one record in ten unused, three in twenty mono
    nch = np.array([0] * n0 + [1] * n1 + [2] * (n_records - n0 - n1))[rng.permutation(n_records)]
    gr = np.zeros(n_records, afgpu.MP3_QGRANULE_DTYPE)

    def lay_out():
        at, off = int(rng.integers(1, 4)), np.zeros(n_records, np.int64)
        for r in rng.permutation(n_records):
            off[r] = at * 576
            at += max(int(nch[r]), 1) + int(rng.integers(1, 4))         # an unused slot points at a block of its own
        return off, at
    gr["q_off"], q_blocks = lay_out()
    gr["coef_off"], coef_blocks = lay_out()
    q = np.stack([draw_values(rng) for _ in range(q_blocks)])

    stereo_of = [r for r in range(n_records) if nch[r] == 2]
    tables = draw_tables(rng, len(stereo_of))
    n_sd = max(8, len(stereo_of) // 3 - 4)                              # every descriptor is used, a few by two granules
    sd = np.zeros(n_sd, afgpu.MP3_SDESC_DTYPE)
    sd["type"] = rng.integers(0, 3, (n_sd, 40))
    for k in range(3):
        sd["type"][k] = k                                               # one descriptor of each single type throughout
    sd["fl"], sd["fr"] = draw_factors(rng, n_sd * 40).reshape(n_sd, 40), draw_factors(rng, n_sd * 40).reshape(n_sd, 40)
    sd = sd[rng.permutation(n_sd)]
    for r in range(n_records):
        g = gr[r]
        g["nch"], g["sdesc"] = nch[r], NO_SDESC
        g["scale"][0], g["scale"][1] = draw_scales(rng), draw_scales(rng)
        if nch[r] == 2:
            k = stereo_of.index(r)
            g["table"] = [table_byte(t) for t in tables[k]]
            g["stereo"] = k % 3
            if g["stereo"] == 2:
                g["sdesc"] = (k // 3) % n_sd
        else:                                                           # mono (and unused) records: no stereo processing
            legal = [t for t in range(24) if t != model.REFUSED]
            g["table"] = [table_byte(legal[r % len(legal)]), table_byte(int(rng.choice(legal)))]
    mask = np.zeros(coef_blocks * 576, bool)
    for g in gr:
        mask[int(g["coef_off"]):int(g["coef_off"]) + 576 * int(g["nch"])] = True
    assert int(mask.sum()) == 576 * int(nch.sum())                      # no two granules share a block
    assert (bol[gr["table"] & 31].max(axis=-1) < 40).all()
    for a in (q, gr, sd, mask):
        a.setflags(write=False)
    return q, gr, sd, coef_blocks * 576, mask


def expected(q, gr, sd, coef_floats):
    """the words of the coefficient plane after the launch: the model's spectra at coef_off, SENTINEL elsewhere.  Checks
    that no product of the model is subnormal, infinite or NaN, so that the comparison rests on normal arithmetic alone."""
    spectra = model.requant_numpy(q, gr, sd)
    mag = np.abs(spectra)
    assert np.isfinite(spectra).all() and ((mag == 0) | (mag >= np.finfo(F32).tiny)).all()
    out = np.full(coef_floats, SENTINEL, np.uint32)
    for g in gr:
        for c in range(int(g["nch"])):
            at = int(g["coef_off"]) + 576 * c
            out[at:at + 576] = spectra[int(g["q_off"]) // 576 + c].view(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def expected_hand_made(seed):
    q, gr, sd, coef_floats, mask = hand_made(seed)
    want = expected(q, gr, sd, coef_floats)
    assert ((want != SENTINEL) <= mask).all() and (want[~mask] == SENTINEL).all()
    want.setflags(write=False)
    return want


def describe(q, gr, sd, index):
    """what the float `index` of the coefficient plane is: granule record, channel, line as stored and as read, the value
    read, the channel's table byte and the stereo mode of the line"""
    bol, dst, _ = model.tables_from_bands()
    for r, g in enumerate(gr):
        at = int(index) - int(g["coef_off"])
        if 0 <= at < 576 * int(g["nch"]):
            c, stored = divmod(at, 576)
            t = int(g["table"][c])
            src = int(np.nonzero(dst[t & 31] == stored)[0][0]) if t & 0x80 else stored
            v = [int(q.reshape(-1)[int(g["q_off"]) + 576 * k + src]) for k in range(int(g["nch"]))]
            mode = int(line_modes(g, sd, bol)[0][src]) if g["nch"] == 2 else 0
            return dict(index=int(index), granule=r, channel=c, line=stored, read_from=src, v=v, abs_v=abs(v[c]), table=hex(t),
                        tables=[hex(int(x)) for x in g["table"]], stereo=int(g["stereo"]), mode=mode)
    near = int(np.argmin([abs(int(index) - int(g["coef_off"])) for g in gr]))
    return dict(index=int(index), outside_every_granule=True, nearest_granule=near, nch=int(gr[near]["nch"]),
                floats_from_its_block=int(index) - int(gr[near]["coef_off"]))


def same_words(got, want, q, gr, sd):
    """got == want word for word; the first mismatches are reported as `describe` names them"""
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [dict(describe(q, gr, sd, i), got=hex(int(got[i])), want=hex(int(want[i]))) for i in bad[:6]])


def rebased(rng, q, gr):
    """the granules of a parsed file (coef_off == q_off, in order) moved into shuffled, gapped planes with q_off != coef_off:
    (q plane, records, floats of the coefficient plane, for every record the block its spectra came from)"""
    gr = gr.copy()
    src = gr["q_off"] // 576
    ends = []
    for key in ("q_off", "coef_off"):
        at = int(rng.integers(1, 4)) + (key == "coef_off")
        for r in rng.permutation(len(gr)):
            gr[key][r] = at * 576
            at += int(gr["nch"][r]) + int(rng.integers(1, 4))
        ends.append(at)
    plane = rng.integers(-model.MAX_ABS, model.MAX_ABS + 1, (ends[0], 576)).astype(np.int16)
    for g, s in zip(gr, src):
        b = int(g["q_off"]) // 576
        plane[b:b + int(g["nch"])] = q[int(s):int(s) + int(g["nch"])]
    assert (gr["q_off"] != gr["coef_off"]).any()
    return plane, gr, ends[1] * 576, src
